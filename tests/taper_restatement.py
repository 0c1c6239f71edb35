"""The contract of smm_taper_build (include/smm_hip.h) restated in numpy, by brute force over all pairs: no cells, no
search -- independent of how the library finds its candidates.  Every operation is one IEEE double operation in exactly
the stated order, so the library's pattern and values are compared bit for bit.  Also the named point sets that the CPU
and GPU tests share."""
import functools

import numpy as np
import scipy.sparse as sp

KINDS = ("boxcar", "gaspari_cohn")
EDGE_FACTOR = 1.0 + 2.0 ** -20          # the library's cell edge is cutoff * EDGE_FACTOR while the cell cap does not bind


def as_points(x):
    x = np.asarray(x, dtype=np.float64)
    return x.reshape(-1, 1) if x.ndim == 1 else x


def d2_matrix(a, b):
    """d2[i, j] = +0.0, then for t = 0 .. dim-1: df = a[i,t] - b[j,t]; d2 = d2 + df * df."""
    a, b = as_points(a), as_points(b)
    d2 = np.zeros((a.shape[0], b.shape[0]), dtype=np.float64)
    for t in range(a.shape[1]):
        df = a[:, None, t] - b[None, :, t]
        d2 = d2 + df * df
    return d2


def gc_near(z):
    """The branch for z <= 1, in the contract's order."""
    p = -0.25 * z + 0.5
    p = p * z + 0.625
    p = p * z - (5.0 / 3.0)
    p = p * z
    return p * z + 1.0


def gc_far(z):
    """The branch for z > 1, in the contract's order."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        p = (1.0 / 12.0) * z - 0.5
        p = p * z + 0.625
        p = p * z + (5.0 / 3.0)
        p = p * z - 5.0
        p = p * z + 4.0
        return p - 2.0 / (3.0 * z)


def weight(d2, cutoff, kind):
    """The stored value for squared distances d2 (any shape)."""
    d2 = np.asarray(d2, dtype=np.float64)
    if kind == "boxcar":
        return np.ones_like(d2)
    assert kind == "gaspari_cohn"
    c = 0.5 * cutoff
    z = np.sqrt(d2) / c
    p = np.where(z <= 1.0, gc_near(z), gc_far(z))
    return np.where(p < 0.0, 0.0, p)


def gaspari_cohn_textbook(z):
    """Gaspari & Cohn (1999), eq. 4.10, in its power form (z = distance / half-width, 0 <= z < 2)."""
    z = np.asarray(z, dtype=np.float64)
    near = -0.25 * z ** 5 + 0.5 * z ** 4 + 0.625 * z ** 3 - (5.0 / 3.0) * z ** 2 + 1.0
    with np.errstate(divide="ignore"):
        far = z ** 5 / 12.0 - 0.5 * z ** 4 + 0.625 * z ** 3 + (5.0 / 3.0) * z ** 2 - 5.0 * z + 4.0 - 2.0 / (3.0 * z)
    return np.where(z <= 1.0, near, far)


def pattern(d2, cutoff):
    """(indptr int32, indices int32, mask) of the entries d2 < cutoff * cutoff, rows ascending."""
    keep = d2 < cutoff * cutoff
    indptr = np.zeros(d2.shape[0] + 1, dtype=np.int32)
    indptr[1:] = np.cumsum(keep.sum(axis=1))
    return indptr, np.nonzero(keep)[1].astype(np.int32), keep


def restate(a, b, cutoff, kind, d2=None):
    """(indptr int32, indices int32, data float64) of the taper of a against b (None: a itself)."""
    a = as_points(a)
    b = a if b is None else as_points(b)
    d2 = d2_matrix(a, b) if d2 is None else d2
    indptr, indices, keep = pattern(d2, cutoff)
    return indptr, indices, weight(d2[keep], cutoff, kind)


def restate_csr(a, b, cutoff, kind):
    a = as_points(a)
    nb = a.shape[0] if b is None else as_points(b).shape[0]
    indptr, indices, data = restate(a, b, cutoff, kind)
    return sp.csr_matrix((data, indices, indptr), shape=(a.shape[0], nb))


def dense_taper(a, cutoff, kind="gaspari_cohn"):
    d2 = d2_matrix(a, a)
    return np.where(d2 < cutoff * cutoff, weight(d2, cutoff, kind), 0.0)


# ------------------------------------------------------------------------------ point sets
COUNTS = (1, 2, 63, 64, 65, 257, 1000)
DENSITIES = ("diagonal", "thirty", "all")


def uniform(n, dim, seed=0):
    return np.random.default_rng(1000 * dim + seed).random((n, dim))


def density_cutoff(n, dim, density):
    """Cutoff for n uniform points of the unit box: only the diagonal, about 30 neighbours, or every pair."""
    if density == "diagonal":
        return 1e-9
    if density == "all":
        return 2.0                                              # > sqrt(3), the unit cube's diagonal
    share = min(30.0 / n, 1.0)
    return {1: share / 2.0, 2: (share / np.pi) ** 0.5, 3: (share * 0.75 / np.pi) ** (1.0 / 3.0)}[dim]


def _embed(x, dim, rest=0.25):
    """Points on a line along the first coordinate, the other coordinates constant."""
    out = np.full((len(x), dim), rest, dtype=np.float64)
    out[:, 0] = x
    return out


def boundary_points(dim, cutoff=0.1, lo=0.3):
    """b points on the cell boundaries lo + k * edge (and their neighbours in float64 on both sides), with partners at
    distance nextafter(cutoff, 0) on both sides: the pairs that a cell search of 'own cell +- 1' with a rounded quotient
    would be in danger of losing.  The smallest coordinate is lo itself, so the library's grid starts there."""
    edge = cutoff * EDGE_FACTOR
    near = np.nextafter(cutoff, 0.0)
    xs = [lo]
    for k in range(1, 7):
        x = lo + k * edge
        for v in (np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)):
            xs += [v, v + near, v + cutoff]
            if k >= 2:
                xs += [v - near, v - cutoff]
    return _embed(np.array(xs, dtype=np.float64), dim, rest=0.0)


@functools.lru_cache(maxsize=None)
def point_set(name, dim):
    """(a, b, cutoff) of a named case; b None means the square case b = a."""
    rng = np.random.default_rng(77 + dim)
    if name == "rows32":                                        # every row has 32 entries: the last length of seg_sort's short class
        return _embed(np.arange(20, 60) + 0.5, dim), _embed(np.arange(100.0), dim), 16.25
    if name == "rows33":                                        # 33: the first of its LDS class
        return _embed(np.arange(20.0, 60.0), dim), _embed(np.arange(100.0), dim), 16.5
    if name == "long_rows":                                     # 3 rows of 8200 > SEG_LDS entries: sorted in global memory
        return uniform(3, dim, 1), uniform(8200, dim, 2), 2.0
    if name == "coincident":
        p = uniform(50, dim, 3)
        return np.concatenate([p, p[::-1]]), None, 0.2
    if name == "integer_grid":                                  # pairs at exactly the cutoff are excluded
        side = {1: 50, 2: 12, 3: 6}[dim]
        g = np.stack(np.meshgrid(*[np.arange(side, dtype=np.float64)] * dim, indexing="ij"), axis=-1).reshape(-1, dim)
        return g, None, 2.0
    if name == "cell_boundaries":
        return boundary_points(dim), None, 0.1
    if name == "offset_1e6":
        return 1e6 + 10.0 * uniform(300, dim, 4), None, 1.0
    if name == "negative":
        return -5.0 + 10.0 * uniform(300, dim, 5) * np.array([1.0, -1.0, 1.0][:dim]), None, 1.0
    if name == "two_clusters":                                  # 1e9 cutoffs apart: the cell cap decides the edge
        p = 3.0 * rng.random((80, dim))
        p[40:, 0] += 1e9
        return p, None, 1.0
    if name == "anisotropic":                                   # a box of 1e6 x 1 x 1
        return uniform(500, dim, 6) * np.array([1e6, 1.0, 1.0][:dim]), None, 2000.0
    if name == "rectangular":
        return uniform(37, dim, 7), uniform(300, dim, 8), 0.3
    raise KeyError(name)


NAMED_SETS = ("rows32", "rows33", "long_rows", "coincident", "integer_grid", "cell_boundaries", "offset_1e6", "negative",
              "two_clusters", "anisotropic", "rectangular")


@functools.lru_cache(maxsize=None)
def uniform_d2(n, dim):
    """The squared distances of the uniform set of n points (shared by the three densities and both kinds)."""
    p = uniform(n, dim)
    d2 = d2_matrix(p, p)
    d2.setflags(write=False)
    return d2


@functools.lru_cache(maxsize=None)
def named_d2(name, dim):
    a, b, _ = point_set(name, dim)
    d2 = d2_matrix(a, a if b is None else b)
    d2.setflags(write=False)
    return d2
