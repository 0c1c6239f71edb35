"""The contract of smm_interp_build (include/smm_hip.h) restated in numpy: the cell by np.searchsorted, the fraction by one
subtraction each and one division, the weights multiplied left to right -- every operation on float64 arrays, so every
product is rounded.  Plus the grids and point sets that the CPU and the GPU tests share."""
import numpy as np
import scipy.sparse as sp

METHODS = ("linear", "nearest")
POLICIES = ("error", "clamp", "zero")
COUNTS = (0, 1, 2, 3, 63, 64, 65, 255, 257, 1001)
EPS = np.finfo(np.float64).eps


class OutsideError(ValueError):
    """Points outside the grid under the policy "error"; .count is their number."""

    def __init__(self, count):
        super().__init__(f"{count} points lie outside the grid")
        self.count = count


def as_points(points):
    p = np.asarray(points, dtype=np.float64)
    return p.reshape(-1, 1) if p.ndim == 1 else p


def as_axes(axes):
    if isinstance(axes, np.ndarray) and axes.ndim == 1:
        axes = [axes]
    return [np.asarray(a, dtype=np.float64) for a in axes]


def strides(axes):
    """Column stride of every axis: row-major, axis 0 slowest."""
    m = [a.size for a in as_axes(axes)]
    return [int(np.prod(m[t + 1:], dtype=np.int64)) for t in range(len(m))]


def cells(points, axes):
    """(c, f, out): cell index (n x dim, int64), fraction BEFORE any policy (n x dim) and the per-point outside flag."""
    p, axes = as_points(points), as_axes(axes)
    n, dim = p.shape
    c = np.zeros((n, dim), dtype=np.int64)
    f = np.zeros((n, dim))
    out = np.zeros(n, dtype=bool)
    for t, a in enumerate(axes):
        x = p[:, t]
        ct = np.clip(np.searchsorted(a, x, side="right") - 1, 0, a.size - 2)
        c[:, t] = ct
        with np.errstate(invalid="ignore"):
            f[:, t] = (x - a[ct]) / (a[ct + 1] - a[ct])
        out |= (x < a[0]) | (x > a[-1])
    return c, f, out


def outside_count(points, axes):
    return int(cells(points, axes)[2].sum())


def restate(points, axes, method="linear", outside="error"):
    """(indptr int32, indices int32, data float64) of the interpolation operator; OutsideError under "error"."""
    assert method in METHODS and outside in POLICIES
    p, axes = as_points(points), as_axes(axes)
    n, dim = p.shape
    assert dim == len(axes) and np.all(np.isfinite(p))
    c, f, out = cells(p, axes)
    if outside == "error" and out.any():
        raise OutsideError(int(out.sum()))
    for t, a in enumerate(axes):                                   # CLAMP (ZERO keeps CLAMP's columns)
        f[p[:, t] < a[0], t] = 0.0
        f[p[:, t] > a[-1], t] = 1.0
    st = strides(axes)
    if method == "nearest":
        cols = np.zeros(n, dtype=np.int64)
        for t in range(dim):
            cols += (c[:, t] + (f[:, t] > 0.5)) * st[t]
        vals = np.ones(n)
        if outside == "zero":
            vals[out] = 0.0
        return np.arange(n + 1, dtype=np.int32), cols.astype(np.int32), vals
    E = 1 << dim
    cols = np.zeros((n, E), dtype=np.int64)
    vals = np.zeros((n, E))
    for e in range(E):
        w = None
        for t in range(dim):
            up = (e >> (dim - 1 - t)) & 1
            cols[:, e] += (c[:, t] + up) * st[t]
            wt = f[:, t] if up else 1.0 - f[:, t]
            w = wt if w is None else w * wt                        # ((w_0 * w_1) * w_2) * w_3
        vals[:, e] = w
    if outside == "zero":
        vals[out, :] = 0.0
    return (np.arange(n + 1, dtype=np.int64) * E).astype(np.int32), cols.ravel().astype(np.int32), np.ascontiguousarray(vals.ravel())


def restate_csr(points, axes, method="linear", outside="error"):
    ptr, idx, val = restate(points, axes, method, outside)
    K = int(np.prod([a.size for a in as_axes(axes)], dtype=np.int64))
    return sp.csr_matrix((val, idx, ptr), shape=(ptr.size - 1, K))


# ------------------------------------------------------------------------------ grids
def nonuniform(m, seed, lo=-1.0, hi=2.0):
    """m strictly ascending nodes from lo to hi with spacings that vary by a factor of up to 20."""
    steps = np.random.default_rng(seed).uniform(0.05, 1.0, m - 1)
    a = lo + (hi - lo) * np.concatenate([[0.0], np.cumsum(steps)]) / steps.sum()
    a[-1] = hi
    assert np.all(a[1:] > a[:-1])
    return a


def grid(name, dim):
    """The named grids of the tests, as a list of dim axes."""
    if name == "single_cell":
        return [np.array([0.25, 1.5]) + t for t in range(dim)]
    if name == "three_nodes":
        return [np.array([-1.0, 0.5, 0.75]) * (t + 1) for t in range(dim)]
    if name == "deep":                                             # 1000 non-uniform nodes on axis 0: ten search steps
        return [nonuniform(1000, 7)] + [nonuniform(4 + t, 8 + t) for t in range(1, dim)]
    if name == "mixed":
        return [nonuniform(m, 20 + t, -3.0 + t, 5.0 * (t + 1)) for t, m in enumerate((2, 37, 3, 5)[:dim])]
    if name == "uniform":
        return [np.linspace(0.0, 1.0 + t, 6 + 3 * t) for t in range(dim)]
    raise KeyError(name)


GRIDS = ("single_cell", "three_nodes", "deep", "mixed", "uniform")


# ------------------------------------------------------------------------------ points
def inside(n, axes, seed):
    """n points uniformly inside the grid."""
    axes = as_axes(axes)
    rng = np.random.default_rng(seed)
    return np.stack([a[0] + (a[-1] - a[0]) * rng.random(n) for a in axes], axis=1).clip([a[0] for a in axes], [a[-1] for a in axes])


def on_nodes(n, axes, seed):
    """n points that are nodes of the grid (every coordinate a node of its axis)."""
    rng = np.random.default_rng(seed)
    return np.stack([a[rng.integers(0, a.size, n)] for a in as_axes(axes)], axis=1)


def edges(axes, outside):
    """Points whose coordinates sit on the first / last node of an axis, one ulp inside them and (outside=True) one ulp
    outside them, the other coordinates random inside; plus points one ulp below and above an interior node."""
    axes = as_axes(axes)
    dim = len(axes)
    rows = []
    base = inside(8 * dim + 8, axes, 99)
    k = 0
    for t, a in enumerate(axes):
        special = [a[0], a[-1], np.nextafter(a[0], np.inf), np.nextafter(a[-1], -np.inf)]
        if a.size > 2:
            special += [np.nextafter(a[a.size // 2], -np.inf), np.nextafter(a[a.size // 2], np.inf), a[a.size // 2]]
        if outside:
            special += [np.nextafter(a[0], -np.inf), np.nextafter(a[-1], np.inf), a[0] - 1.0, a[-1] + 10.0]
        for x in special:
            r = base[k % base.shape[0]].copy()
            r[t] = x
            rows.append(r)
            k += 1
    if outside and dim > 1:                                        # outside in two axes at once, on opposite sides
        r = base[0].copy()
        r[0], r[1] = np.nextafter(axes[0][0], -np.inf), axes[1][-1] + 1.0
        rows.append(r)
    return np.array(rows)


def midpoints(axes):
    """Points exactly half-way between neighbouring nodes where that is exact in float64 (f == 0.5: NEAREST's tie)."""
    axes = as_axes(axes)
    p = np.stack([0.5 * (a[0] + a[1]) for a in axes])
    return p.reshape(1, -1)
