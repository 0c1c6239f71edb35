"""sparse_matrix_multiply() -- the reference's public entry point, served by the MI355X engine.

Drop-in for reference sparse_matrix_mult/matrix_ops.py:271-387: same name, same arguments,
same argument meaning, same return types, same raised errors.  What differs:
  * the work is done by libsmm_hip.so (hand-written HIP, gfx950) through the v2 C ABI of
    include/smm_hip.h; operands go host->HBM once, results come back into numpy buffers this
    module owns (no create_sparsemat/memmove round trip, no leaked input structs:
    reference :187-202, :339-340);
  * nothing is printed at import (reference :89-90,133,137);
  * a failure inside the library RAISES (SmmError) instead of being printed and turned into
    an all-zero result (reference :377-387) -- silent zeros would hide a missing GPU.  The
    one swallowed case the reference's callers can observe on purpose, an unknown
    output_format, is kept: message printed, zeros returned.
"""
import os

import numpy as np
from scipy.sparse import csr_matrix, isspmatrix_csr

from ._lib import SMM_VG_MAX_BINS
from .engine import COV_MODELS, INTERP_METHODS, INTERP_OUTSIDE, TAPER_KINDS, SolveInfo, default_context
# the operand and plan cache (operand_cache.py): the entry points lease their operands through with_leases and take
# their plans from plan_for; the public names below are re-exported as the same objects
from .operand_cache import PinnedOperand, cache_stats, clear_cache, plan_for, set_operand_cache, with_leases  # noqa: F401

_INT32_MAX = np.iinfo(np.int32).max

# SMM_EXACT=1 (or set_exact(True)): add products in exactly the reference's order, so float64
# values are bit-identical to the reference's loop; the default lets the waves of a workgroup
# add concurrently -- values agree to rounding (tested to 1e-10 relative), ~3x faster.
# indptr / indices are bit-exact either way.
_exact = os.environ.get("SMM_EXACT", "0") not in ("", "0")


# Mirror epilogue, opt-in: with set_full_symmetric(True) the DENSE results that hold only
# the upper triangle -- output_format='dense' with symmetric=True, and the triple product with
# compute_full_matrix None/0 -- come back as the full symmetric matrix (lower triangle = mirror image of
# the upper one, filled on the device).  compute_full_matrix='mirror' asks for the same for one triple
# product.  The default stays the reference's behaviour (lower triangle 0.0), and compute_full_matrix=1
# keeps reproducing the reference exactly (off-diagonal doubled).  CSR results (output_format='sparse',
# symmetric=True) are mirrored too: row i of the full matrix holds the mirrored entries (columns < i) in ascending
# column order, then the reference's upper-triangle row in its first-touch order; any row length (segments of up to
# 8192 mirrored entries are sorted in LDS, longer ones placed by rank).
_full_symmetric = False


def set_full_symmetric(flag):
    """Return dense upper-triangle results as full symmetric matrices; returns the old setting."""
    global _full_symmetric
    old, _full_symmetric = _full_symmetric, bool(flag)
    return old


# Device-resident results, opt-in: the reference copies every result out of the library into fresh host
# arrays (sparsemat_to_csr / darray_to_numpy, matrix_ops.py:205-240); at BASELINE configs[1] that copy is 40 GB and
# 0.8 s behind 32 ms of GPU work.  With set_result_device(True) (or SMM_RESULT_DEVICE=1) the same call leaves the
# result in HBM: 'dense' and the triple product return a torch.Tensor (float64, cuda), 'sparse' a DeviceCSRResult
# (indptr int64 / indices int32 / data float64 torch tensors, first-touch order as ever) with .to_scipy() for the
# reference's return type.  The default is the reference's behaviour: caller-owned host objects.
_result_device = os.environ.get("SMM_RESULT_DEVICE", "0") not in ("", "0")


def set_result_device(flag):
    """Leave results in HBM as torch tensors (see DeviceCSRResult); returns the old setting."""
    global _result_device
    old, _result_device = _result_device, bool(flag)
    return old


class DeviceCSRResult:
    """A CSR result resident in HBM: .indptr (int64), .indices (int32), .data (float64) are torch CUDA tensors,
    .shape / .nnz as scipy's.  Columns inside a row are in the reference's first-touch order (not sorted)."""
    __slots__ = ("indptr", "indices", "data", "shape")

    def __init__(self, indptr, indices, data, shape):
        self.indptr, self.indices, self.data, self.shape = indptr, indices, data, tuple(shape)

    @property
    def nnz(self):
        return int(self.indices.numel())

    def to_scipy(self):
        """The reference's return type (copies the result to the host)."""
        return _result_csr(self.indptr.cpu().numpy(), self.indices.cpu().numpy(), self.data.cpu().numpy(), self.shape)

    def to_torch_sparse_csr(self):
        """torch.sparse_csr_tensor over the same values (torch wants one index dtype: both int64; columns unsorted)."""
        import torch
        return torch.sparse_csr_tensor(self.indptr, self.indices.to(torch.int64), self.data, size=self.shape,
                                       check_invariants=False)


def set_exact(flag):
    """Select bit-exact (reference-order) accumulation for later calls; returns the old setting."""
    global _exact
    old, _exact = _exact, bool(flag)
    return old


def pin_operand(matrix):
    """Upload `matrix` once and keep it (and everything derived from it) in HBM until unpin().  A DeviceCSRResult -- a
    result left in HBM under set_result_device(True) -- is pinned where it is: its row pointer is narrowed to int32 on the
    device and the three tensors are borrowed (and kept alive) by the operand; nothing is copied to the host or hashed."""
    if isinstance(matrix, DeviceCSRResult):
        return _pin_device_result(matrix)
    matrix = _as_csr(matrix)                              # (a KroneckerOperand is refused, with the pointer to kronecker_product)
    return PinnedOperand(default_context(), matrix)


def _pin_device_result(res):
    rows, cols = res.shape
    nnz = res.nnz
    if nnz >= _INT32_MAX or rows >= _INT32_MAX or cols >= _INT32_MAX:
        raise ValueError(f"pin_operand: a {rows} x {cols} result with {nnz} entries does not fit an operand "
                         "(int32 row pointers and columns: dimensions and nnz must be below 2^31 - 1)")
    ctx = default_context()
    if nnz == 0:
        return PinnedOperand._adopt(ctx, None, (rows, cols))
    import torch
    indices = _to_device(ctx, res.indices, True, "pin_operand", "the result")
    indptr = res.indptr.to(torch.int32)                  # (on the device; csr_from_torch waits for torch's stream)
    return PinnedOperand._adopt(ctx, ctx.csr_from_torch(rows, cols, indptr, indices.contiguous(), res.data.contiguous()))


# ------------------------------------------------------------------ numpy, tensors and the library's device
def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def _torch_device(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def _to_device(ctx, x, is_torch, what, name):
    """x as a tensor on the library's device: a numpy array is uploaded, a tensor must be there already."""
    dev = _torch_device(ctx)
    if not is_torch:
        import torch
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    if x.device != dev:
        raise ValueError(f"{what}: {name} is on {x.device}, the library works on {dev}")
    return x


def _as_kind(z, on_device, ctx=None):
    """z, numpy or a tensor the library made, as the kind the caller gets: a tensor on the library's device (of ctx, or
    of the default context, which is not touched otherwise) or a numpy array."""
    if on_device == _is_torch(z):
        return z
    if not on_device:
        return z.cpu().numpy()
    return _to_device(default_context() if ctx is None else ctx, z, False, None, None)


def _dense_zeros(shape, on_device):
    if on_device:
        import torch
        return torch.zeros(shape, dtype=torch.float64, device=_torch_device(default_context()))
    return np.zeros(shape, dtype=np.float64)


def _on_device(ctx, call):
    """call() with its result left in HBM (torch tensors).  The library works on the context's own stream: torch's
    current stream is drained first (its allocator may hand out memory that kernels queued there still use) and the
    context is synchronised before the result is returned -- which also reports anything the kernels' bounds clamps
    recorded (SMM_ERR_INTERNAL)."""
    import torch
    torch.cuda.current_stream(_torch_device(ctx)).synchronize()
    out = call()
    ctx.synchronize()
    return out


# ------------------------------------------------------------------ points given by coordinates
def _points(x, what, name):
    """(points, n, dim, is_torch): a C-contiguous float64 n x dim numpy array, or a float64 CUDA tensor (1-D or 2-D, any
    strides: _points_on_device decides what is used in place).  1-D means points on a line.  ValueError before any device
    work; how many coordinates a point may have is the caller's check."""
    is_torch = _is_torch(x)
    if is_torch:
        import torch
        if x.dtype != torch.float64 or not x.is_cuda:
            raise ValueError(f"{what}: a torch {name} must be a float64 CUDA tensor")
        ndim = x.dim()
    else:
        x = np.asarray(x, dtype=np.float64)
        ndim = x.ndim
    if ndim not in (1, 2):
        raise ValueError(f"{what}: {name} must be 1-D (points on a line) or 2-D (n x dim), got {ndim} dimensions")
    n, dim = int(x.shape[0]), (1 if ndim == 1 else int(x.shape[1]))
    if not is_torch:
        x = np.ascontiguousarray(x.reshape(n, dim))
    return x, n, dim, is_torch


def _row_layout(shape, strides, dim):
    """(copy_needed, ld) of n points of dim coordinates held in a device view of this shape and these strides (in
    elements).  The kernels read coordinate t of point i at x + i * ld + t, so a view is used in place iff its column
    stride is 1 (2-D) and its row stride is at least dim; anything else -- an expanded view with row stride 0, a
    transpose -- is copied contiguous, and then ld = dim.  A strided 1-D view (x[::2]) stays in place."""
    if (len(shape) == 2 and strides[1] != 1) or strides[0] < dim:
        return True, dim
    return False, int(strides[0])


def _points_on_device(ctx, x, dim, is_torch, what, name):
    """(tensor, ld): the points of _points on the library's device, in place where _row_layout allows it."""
    t = _to_device(ctx, x, is_torch, what, name)
    copy_needed, ld = _row_layout(tuple(t.shape), t.stride(), dim)
    return (t.contiguous() if copy_needed else t), ld


def _deliver_operand(ctx, build, shape, pin, torch_input, to_device):
    """The DeviceCSR that build() returns, which the library owns, as the caller's result: adopted where it is by a
    PinnedOperand (pin), copied device to device into a DeviceCSRResult (to_device), or downloaded into a scipy CSR.  The
    handle is closed unless it is adopted.  build() runs under _on_device when it reads a caller's tensor (torch_input)
    or when the result stays in HBM."""
    if to_device and not pin:
        import torch

        def call():
            handle = build()
            try:
                indptr, indices = handle.pattern_torch()
                data = torch.empty(handle.nnz, dtype=torch.float64, device=_torch_device(ctx))
                handle.values_into(data)
                return DeviceCSRResult(indptr.to(torch.int64), indices, data, shape)
            finally:
                handle.close()

        return _on_device(ctx, call)
    handle = _on_device(ctx, build) if torch_input else build()
    if pin:
        return PinnedOperand._adopt(ctx, handle)
    try:
        return _result_csr(*handle.to_host(), shape)
    finally:
        handle.close()


def localization_taper(coords, cutoff, coords_b=None, taper="gaspari_cohn", pin=False):
    """The localisation matrix L of a set of points, built on the GPU: L[i, j] = w(|coords[i] - coords_b[j]|) for every
    pair closer than `cutoff` -- the `mask` of sparse_triple_product and masked_matrix_multiply and the weights of
    sampled_dense_product(..., scale_by_mask=True).

    coords   : n x dim (dim 1, 2 or 3) or 1-D (n points on a line); a numpy array (cast to float64) or a float64 CUDA
               tensor on the library's device with unit column stride (a column slice of a wider tensor is used in place).
    coords_b : the same kinds, nb x dim; None means coords itself: L is square and symmetric bit for bit.
    cutoff   : finite and positive.  Entry (i, j) is stored iff the squared distance, summed coordinate by coordinate in
               float64, is < cutoff * cutoff (strict).  Distances are Euclidean: for a sphere pass unit-sphere xyz and a
               chord cutoff.
    taper    : "gaspari_cohn" (Gaspari & Cohn 1999, eq. 4.10, half-width cutoff / 2: 1 at distance 0, 0 at the cutoff;
               a correlation function in up to three dimensions) or "boxcar" (1.0 everywhere).
    pin      : False returns a scipy CSR (int32 indices, canonical).  True returns a PinnedOperand that adopts the
               library's operand where it is -- no copy to the host: pass it wherever a matrix is accepted.
    Pattern and values are bit-identical to the order written out in include/smm_hip.h, whatever the grid of cells that
    finds the candidates.  Argument errors are ValueError before any device call; NaN or infinite coordinates are refused
    by the library (SmmError).  Without points the result is empty and no device is touched.  Nothing is printed.
    """
    what = "localization_taper"
    if not isinstance(taper, str) or taper not in TAPER_KINDS:
        raise ValueError(f"{what}: unknown taper {taper!r}, expected one of {sorted(TAPER_KINDS)}")
    try:
        cutoff = float(cutoff)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: cutoff must be a finite positive number") from None
    if not (cutoff > 0.0 and np.isfinite(cutoff)):
        raise ValueError(f"{what}: cutoff must be a finite positive number, got {cutoff}")
    def points(x, name):
        x, n, dim, is_torch = _points(x, what, name)
        if dim < 1 or dim > 3:
            raise ValueError(f"{what}: {name} has {dim} coordinates per point, expected 1, 2 or 3")
        return x, n, dim, is_torch

    a, na, dim, a_torch = points(coords, "coords")
    if coords_b is None:
        b, nb, b_torch = a, na, a_torch
    else:
        b, nb, dim_b, b_torch = points(coords_b, "coords_b")
        if dim_b != dim:
            raise ValueError(f"{what}: coords has {dim} coordinates per point, coords_b has {dim_b}")
    if na >= _INT32_MAX or nb >= _INT32_MAX:
        raise ValueError(f"{what}: at most 2^31 - 2 points on either side, got {na} and {nb}")
    if na == 0 or nb == 0:
        return PinnedOperand._adopt(None, None, (na, nb)) if pin else csr_matrix((na, nb), dtype=np.float64)
    ctx = default_context()
    if not (a_torch or b_torch):
        def build():
            return ctx.taper_host(a, None if b is a else b, cutoff, taper)
    else:
        da, lda = _points_on_device(ctx, a, dim, a_torch, what, "coords")
        db, ldb = (da, lda) if b is a else _points_on_device(ctx, b, dim, b_torch, what, "coords_b")

        def build():
            return ctx.taper_into(da, lda, db, ldb, na, nb, dim, cutoff, taper)
    # (a taper stays a scipy CSR under set_result_device(True): to_device is never asked for)
    return _deliver_operand(ctx, build, (na, nb), pin, a_torch or b_torch, False)


# ------------------------------------------------------------------ parametric covariance on a pattern
def _cov_lengths(length, dim, what):
    """(lengths float64[dim], scalar): `length` as one correlation length per coordinate, and whether it was given as one
    number.  ValueError for anything the library would refuse."""
    try:
        arr = np.asarray(length, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: length must be a positive number, or one per coordinate") from None
    scalar = arr.ndim == 0
    if scalar:
        arr = np.full(dim, float(arr))
    elif arr.shape != (dim,):
        raise ValueError(f"{what}: length must be a scalar or hold one number per coordinate ({dim}), got shape {arr.shape}")
    if not np.all(np.isfinite(arr) & (arr > 0.0)):
        raise ValueError(f"{what}: every length must be finite and positive, got {arr.tolist()}")
    return np.ascontiguousarray(arr), scalar


def covariance_on_pattern(pattern, coords, model, length, variance=1.0, coords_b=None, scale_by_pattern=False, derivative=None,
                          pin=False):
    """A parametric covariance evaluated at the stored positions of `pattern`, on the GPU: Q[i, j] = variance * c(h) with
    h = |(coords[i] - coords_b[j]) / length|, and optionally dQ/dlength on the same positions -- the prior of a
    likelihood search over variances and correlation lengths, and the dQ of its gradient's trace term.

    pattern  : na x nb; scipy CSR, anything csr_matrix() accepts, or a PinnedOperand -- a taper from localization_taper,
               Q's pattern, or H's for cross-covariances.  It is used as stored (rows may be unsorted and repeat columns)
               and is never written, nor is anything cached for it.
    coords   : na x dim (dim 1, 2 or 3) or 1-D; numpy (cast to float64) or a float64 CUDA tensor on the library's device
               with unit column stride (a column slice of a wider tensor is used in place), as in localization_taper.
    coords_b : the same kinds, nb x dim; None means coords itself.
    model    : "spherical", "exponential", "gaussian", "matern32" or "matern52"; the formulas, operation by operation, are
               in include/smm_hip.h.  c(0) = 1 in each; the spherical one is exactly 0 from h = 1 on.
    length   : a positive number, or one per coordinate (anisotropy).
    variance : finite; the value at distance 0.
    scale_by_pattern : multiply every result by the pattern's stored value: with a Gaspari-Cohn taper L as the pattern this
               is Q = L o C, compactly supported and still positive semidefinite, and dQ = L o dC.
    derivative : None; "length" -- with respect to the common length, which needs a scalar `length` --; or a coordinate's
               index t -- with respect to length[t].  The call then returns the pair (Q, dQ) from one pass.
    pin      : False returns scipy CSR matrices (DeviceCSRResults under set_result_device(True)) with the pattern's
               structure.  True returns PinnedOperands over the arrays the kernel wrote, by the path of
               pin_operand(DeviceCSRResult): nothing is copied to the host.
    A new length is a new call that writes new arrays; nothing is refreshed in place.  Coordinates are not screened: a NaN
    gives NaN at its entries.  Argument errors are ValueError before any device call; a pattern without entries returns
    without one.  Nothing is printed.
    """
    what = "covariance_on_pattern"
    pattern = _as_csr(pattern)
    if not isinstance(model, str) or model not in COV_MODELS:
        raise ValueError(f"{what}: unknown model {model!r}, expected one of {sorted(COV_MODELS)}")

    def points(x, name):
        x, n, dim, is_torch = _points(x, what, name)
        if dim < 1 or dim > 3:
            raise ValueError(f"{what}: {name} has {dim} coordinates per point, expected 1, 2 or 3")
        return x, n, dim, is_torch

    a, na, dim, a_torch = points(coords, "coords")
    if coords_b is None:
        b, nb, b_torch = a, na, a_torch
    else:
        b, nb, dim_b, b_torch = points(coords_b, "coords_b")
        if dim_b != dim:
            raise ValueError(f"{what}: coords has {dim} coordinates per point, coords_b has {dim_b}")
    shape = (int(pattern.shape[0]), int(pattern.shape[1]))
    if (na, nb) != shape:
        raise ValueError(f"{what}: the pattern is {shape[0]} x {shape[1]}, the points are {na} and {nb}")
    lengths, scalar = _cov_lengths(length, dim, what)
    try:
        variance = float(variance)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: variance must be a finite number") from None
    if not np.isfinite(variance):
        raise ValueError(f"{what}: variance must be a finite number, got {variance}")
    if derivative is None or (isinstance(derivative, str) and derivative == "length"):
        if derivative is not None and not scalar:
            raise ValueError(f'{what}: derivative="length" is with respect to one common length: pass a scalar length, '
                             "or a coordinate's index")
    elif isinstance(derivative, (int, np.integer)) and not isinstance(derivative, bool):
        if not 0 <= derivative < dim:
            raise ValueError(f"{what}: derivative {derivative} is not a coordinate of {dim}-dimensional points")
        derivative = int(derivative)
    else:
        raise ValueError(f'{what}: derivative must be None, "length" or a coordinate\'s index, got {derivative!r}')
    both = derivative is not None
    if pattern.nnz == 0:
        empty = [PinnedOperand._adopt(None, None, shape) if pin else _zero_result(shape) for _ in range(1 + both)]
        return tuple(empty) if both else empty[0]
    ctx = default_context()
    args = dict(model=model, length=lengths, variance=variance, wrt=derivative, scale=scale_by_pattern)

    def body(lp):
        if not (a_torch or b_torch or _result_device or pin):
            data = ctx.cov_host(lp.handle, a, None if b is a else b, **args)
            return [_result_csr(*_mask_pattern(pattern), d, shape) for d in data if d is not None]
        import torch
        da, lda = _points_on_device(ctx, a, dim, a_torch, what, "coords")
        db, ldb = (da, lda) if b is a else _points_on_device(ctx, b, dim, b_torch, what, "coords_b")

        def call():
            data = [torch.empty(lp.handle.nnz, dtype=torch.float64, device=da.device) for _ in range(1 + both)]
            ctx.cov_into(lp.handle, da, lda, db, ldb, dim, d_val=data[0], d_dval=data[1] if both else None, **args)
            indptr, indices = lp.handle.pattern_torch()
            indptr = indptr.to(torch.int64)
            # (each result owns its pattern tensors: a caller may sort or pin one of the pair and not the other)
            return [DeviceCSRResult(indptr if i == 0 else indptr.clone(), indices if i == 0 else indices.clone(), d, shape)
                    for i, d in enumerate(data)]

        out = _on_device(ctx, call)
        if pin:
            return [_pin_device_result(r) for r in out]
        return out if _result_device else [r.to_scipy() for r in out]

    out = with_leases(ctx, (pattern,), body)
    return tuple(out) if both else out[0]


# ------------------------------------------------------------------ empirical variogram on a pattern
class VariogramResult:
    """What empirical_variogram returns, numpy arrays on the host: .edges (nb + 1), and per bin .count (int64, the pairs),
    .sum_lag (the sum of their distances), .sum_sq (the sum of their squared increments, over all k columns of the values),
    .lag = sum_lag / count and .gamma = sum_sq / (2 k count) -- both NaN in a bin without pairs."""
    __slots__ = ("edges", "count", "sum_lag", "sum_sq", "lag", "gamma")

    def __init__(self, edges, count, sum_lag, sum_sq, k):
        self.edges, self.count, self.sum_lag, self.sum_sq = edges, count, sum_lag, sum_sq
        pairs = np.where(count > 0, count, 1).astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            self.lag = np.where(count > 0, sum_lag / pairs, np.nan)
            self.gamma = np.where(count > 0, sum_sq / (2.0 * k * pairs), np.nan) if k > 0 else np.full(count.shape, np.nan)

    def __repr__(self):
        return f"VariogramResult({self.count.size} bins, {int(self.count.sum())} pairs)"


def _variogram_edges(bin_edges, what):
    """The bin edges as float64[nb + 1]; ValueError for anything the library would refuse."""
    try:
        edges = np.array(bin_edges, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: bin_edges must be a sequence of numbers") from None
    if edges.ndim != 1 or not 2 <= edges.size <= SMM_VG_MAX_BINS + 1:
        raise ValueError(f"{what}: bin_edges must be 1-D with 2 to {SMM_VG_MAX_BINS + 1} entries (1 to {SMM_VG_MAX_BINS} bins), "
                         f"got shape {edges.shape}")
    if not np.all(np.isfinite(edges)):
        raise ValueError(f"{what}: every bin edge must be finite, got {edges.tolist()}")
    if edges[0] < 0.0:
        raise ValueError(f"{what}: the first bin edge must be >= 0, got {edges[0]}")
    if not np.all(edges[:-1] < edges[1:]):
        raise ValueError(f"{what}: bin_edges must ascend strictly, got {edges.tolist()}")
    return np.ascontiguousarray(edges)


def empirical_variogram(pattern, coords, values, bin_edges, upper=True):
    """The empirical variogram of `values` at the points `coords`, on the GPU: over the pairs (i, j) that `pattern` stores,
    binned by their distance h into [bin_edges[b], bin_edges[b+1]), the number of pairs, the mean distance and
    gamma = mean of (values[i] - values[j])^2 / 2 -- the look at the data that suggests a model and a first length for
    covariance_on_pattern and the likelihood search.  Nothing is searched: the pairs are the pattern's entries, usually a
    localization_taper of the same coordinates with the largest lag of interest as its cutoff.

    pattern   : n x n; scipy CSR, anything csr_matrix() accepts, or a PinnedOperand.  It is used as stored (rows may be
                unsorted and repeat columns: a repeated entry counts again) and is never written, nor is anything cached
                for it.  Its values are not read.
    coords    : n x dim (dim 1, 2 or 3) or 1-D; numpy (cast to float64) or a float64 CUDA tensor on the library's device with
                unit column stride (a column slice of a wider tensor is used in place), as in localization_taper.
    values    : n, or n x k (k variables, or k realisations of one: gamma averages over them); the same kinds.
    bin_edges : 2 to 33 finite numbers, strictly ascending, the first >= 0.  A pair belongs to bin b iff
                bin_edges[b] <= h < bin_edges[b+1]; pairs outside [bin_edges[0], bin_edges[-1]) are left out.
    upper     : True counts the stored entries with j > i, so each pair of a symmetric pattern once and the diagonal never;
                False counts every stored entry.
    Returns a VariogramResult of numpy arrays.  The sums are taken in the fixed order written out in include/smm_hip.h: no
    atomics, two calls give the same bits.  Values are not screened: a NaN makes gamma NaN in the bins its pairs fall in; a
    NaN coordinate takes its pairs out of every bin.  Argument errors are ValueError before any device call; a pattern
    without entries returns zero counts without one.  Nothing is printed.
    """
    what = "empirical_variogram"
    pattern = _as_csr(pattern)
    a, n, dim, a_torch = _points(coords, what, "coords")
    if dim < 1 or dim > 3:
        raise ValueError(f"{what}: coords has {dim} coordinates per point, expected 1, 2 or 3")
    y, ny, k, y_torch = _points(values, what, "values")
    shape = (int(pattern.shape[0]), int(pattern.shape[1]))
    if shape[0] != shape[1]:
        raise ValueError(f"{what}: the pattern must be square, got {shape[0]} x {shape[1]}")
    if n != shape[0] or ny != n:
        raise ValueError(f"{what}: the pattern is {shape[0]} x {shape[1]}, coords holds {n} points and values {ny} rows")
    edges = _variogram_edges(bin_edges, what)
    if not isinstance(upper, (bool, np.bool_)):
        raise ValueError(f"{what}: upper must be True or False, got {upper!r}")
    upper = bool(upper)
    nb = edges.size - 1
    if pattern.nnz == 0:
        return VariogramResult(edges, np.zeros(nb, dtype=np.int64), np.zeros(nb), np.zeros(nb), k)
    ctx = default_context()

    def body(lp):
        if not (a_torch or y_torch):
            return ctx.variogram_host(lp.handle, a, y, edges, upper)
        da, lda = _points_on_device(ctx, a, dim, a_torch, what, "coords")
        dy, ldy = _points_on_device(ctx, y, k, y_torch, what, "values")
        return _on_device(ctx, lambda: ctx.variogram_device(lp.handle, da, lda, dim, dy, ldy, k, edges, upper))

    count, sum_h, sum_sq = with_leases(ctx, (pattern,), body)
    return VariogramResult(edges, count, sum_h, sum_sq, k)


# ------------------------------------------------------------------ observation operator from coordinates
def _interp_axes(axes, what):
    """The grid as a list of 1-D float64 arrays; `axes` is a sequence of 1-D arrays, or one array for a line.  ValueError
    for anything the library would refuse."""
    if _is_torch(axes):
        raise ValueError(f"{what}: axes are host arrays (a sequence of 1-D numpy arrays), not tensors")
    if isinstance(axes, np.ndarray) and axes.ndim == 1 and axes.dtype != object:
        axes = [axes]
    try:
        axes = [np.asarray(a, dtype=np.float64) for a in axes]
    except (TypeError, ValueError):
        raise ValueError(f"{what}: axes must be a sequence of 1-D arrays of numbers") from None
    if not 1 <= len(axes) <= 4:
        raise ValueError(f"{what}: the grid has {len(axes)} axes, expected 1 to 4")
    for t, a in enumerate(axes):
        if a.ndim != 1:
            raise ValueError(f"{what}: axis {t} must be 1-D, got {a.ndim} dimensions")
        if a.size < 2:
            raise ValueError(f"{what}: axis {t} has {a.size} nodes, an axis needs at least 2")
        if not np.all(np.isfinite(a)):
            raise ValueError(f"{what}: axis {t} has nodes that are not finite")
        if not np.all(a[1:] > a[:-1]):
            raise ValueError(f"{what}: axis {t} is not strictly ascending")
    return axes


def interpolation_operator(points, axes, method="linear", outside="error", pin=False):
    """The observation operator H of a rectilinear grid, built on the GPU: the n x K matrix that interpolates a field given
    on the grid's K nodes to n points -- the matrix_h of triple_product_apply, innovation_solve and innovation_logdet.

    points  : n x dim (dim 1 to 4) or 1-D (n points on a line); a numpy array (cast to float64) or a float64 CUDA tensor
              on the library's device with unit column stride (a column slice of a wider tensor is used in place).
    axes    : a sequence of dim 1-D arrays, or one array for a line: the nodes of every axis, finite and strictly
              ascending, at least 2 each, spacing free.  K = the product of their lengths; node (j_0, ..., j_{dim-1}) is
              column (j_0 * m_1 + j_1) * m_2 + ... -- `field.ravel()` of a C-ordered field[j_0, ..., j_{dim-1}].  With time
              as axis 0 these are the columns of KroneckerOperand(D, E).
    method  : "linear" -- 2^dim multilinear weights per row, at the corners of the point's cell -- or "nearest" -- one
              entry 1.0 at the nearest node (a tie goes to the lower node).
    outside : what a point outside [first node, last node] in some axis does.  "error" (default): the call fails
              (SmmError) and says how many there are.  "clamp": constant extrapolation from the edge.  "zero": the row
              keeps its columns and holds zeros -- the observation sees nothing.
    pin     : False returns a scipy CSR (int32 indices, canonical), or a DeviceCSRResult under set_result_device(True).
              True returns a PinnedOperand that adopts the library's operand where it is -- no copy to the host.
    Pattern and values are bit-identical to the order written out in include/smm_hip.h; the row pointer is i * 2^dim (or
    i).  Argument errors are ValueError before any device call; NaN or infinite coordinates are refused by the library
    (SmmError).  Without points the result is empty and no device is touched.  Nothing is printed.
    """
    what = "interpolation_operator"
    for value, table, name in ((method, INTERP_METHODS, "method"), (outside, INTERP_OUTSIDE, "policy")):
        if not isinstance(value, str) or value not in table:
            raise ValueError(f"{what}: unknown {name} {value!r}, expected one of {sorted(table)}")
    axes = _interp_axes(axes, what)
    points, n, dim, is_torch = _points(points, what, "points")
    if dim != len(axes):
        raise ValueError(f"{what}: points has {dim} coordinates per point, the grid has {len(axes)} axes")
    K = 1
    for a in axes:
        K *= a.size
    per_row = 1 if method == "nearest" else 2 ** dim
    if K >= _INT32_MAX or n >= _INT32_MAX:
        raise ValueError(f"{what}: {n} points on {K} nodes: both must be below 2^31 - 1 (an operand's dimensions)")
    if n * per_row > _INT32_MAX - 1:
        raise ValueError(f"{what}: {n} rows of {per_row} entries do not fit one operand (int32 row pointers, at most 2^31 - 2)")
    shape = (n, K)
    if n == 0:
        return PinnedOperand._adopt(None, None, shape) if pin else _zero_result(shape)
    ctx = default_context()
    if not is_torch:
        def build():
            return ctx.interp_host(points, axes, method, outside)
    else:
        d_points, ldp = _points_on_device(ctx, points, dim, True, what, "points")

        def build():
            return ctx.interp_into(d_points, ldp, n, dim, axes, method, outside)
    return _deliver_operand(ctx, build, shape, pin, is_torch, _result_device)


# ------------------------------------------------------------------ Kronecker operand Q = D (x) E
def _kron_shape(d, e, what):
    """((p r, p' r'), nnz(D) nnz(E)) of D (x) E; ValueError where a dimension does not fit an operand."""
    shape = (int(d.shape[0]) * int(e.shape[0]), int(d.shape[1]) * int(e.shape[1]))
    if shape[0] >= _INT32_MAX or shape[1] >= _INT32_MAX:
        raise ValueError(f"{what}: D (x) E would be {shape[0]} x {shape[1]}; both dimensions must be below 2^31 - 1")
    return shape, int(d.nnz) * int(e.nnz)


class KroneckerOperand:
    """Q = D (x) E held as its two factors and never formed: D is p x p' (the temporal covariance), E is r x r' (the spatial
    one); row t * r + j of Q is the pair (t, j), column t' * r' + j' the pair (t', j').  Accepted as matrix_a of
    sparse_dense_multiply (transpose=False), as matrix_q of triple_product_apply and innovation_solve, and -- for entries of
    a product on a given pattern -- as matrix_q of sparse_triple_product(..., mask=L) and as matrix_b of
    masked_matrix_multiply; every other call wants the explicit matrix of kronecker_product(D, E).

    D, E : scipy CSR, anything csr_matrix() accepts, or PinnedOperands.
    .shape, .nnz (of the explicit matrix), .factors == (D, E), .to_scipy() (scipy.sparse.kron of the factors, on the host).
    """
    __slots__ = ("factors", "shape", "nnz")

    def __init__(self, D, E):
        d, e = _as_csr(D), _as_csr(E)
        self.factors = (d, e)
        self.shape, self.nnz = _kron_shape(d, e, "KroneckerOperand")

    def to_scipy(self):
        from scipy.sparse import kron
        d, e = (f.to_scipy() if isinstance(f, PinnedOperand) else f for f in self.factors)
        return csr_matrix(kron(d, e, format="csr"))

    def _square(self, what):
        for name, f in zip("DE", self.factors):
            if f.shape[0] != f.shape[1]:
                raise ValueError(f"{what}: Q must be square, but its factor {name} is {f.shape[0]} x {f.shape[1]}")

    def _canonical_factors(self, what):
        """(D, E) with strictly ascending rows, as the masked products search them: a scipy factor that is not canonical is
        canonicalised on a host copy (as masks are), a PinnedOperand must be canonical."""
        out = []
        for name, f in zip("DE", self.factors):
            if isinstance(f, PinnedOperand):
                if f.nnz and not f._handle.is_canonical():
                    raise ValueError(f"{what}: the pinned factor {name} is not canonical (rows must hold strictly ascending "
                                     "columns): pin it after sum_duplicates()")
            elif not f.has_canonical_format:
                f = f.copy()
                f.sum_duplicates()
            out.append(f)
        return tuple(out)


def kronecker_product(D, E, pin=False):
    """The explicit Kronecker product D (x) E as one CSR matrix, built on the GPU from the two factors.

    D : p x p', E : r x r' (scipy CSR, anything csr_matrix() accepts, or a PinnedOperand).  The result is (p r) x (p' r'):
    row t * r + j holds, for a over row t of D and b over row j of E in stored order, column D.idx[a] * r' + E.idx[b] with
    value D.val[a] * E.val[b] (one rounded multiply; explicitly stored zeros stay entries).  For canonical factors this is
    scipy.sparse.kron(D, E, format="csr") bit for bit in indptr, indices and data.
    pin : False returns a scipy CSR (int32 indices), or a DeviceCSRResult under set_result_device(True).  True returns a
          PinnedOperand that adopts the library's operand where it is -- no copy to the host: pass it wherever a matrix is
          accepted.
    ValueError before any device call: a result dimension of 2^31 - 1 or more, or more than 2^31 - 2 entries (operand row
    pointers are int32) -- a Q that large is used through KroneckerOperand(D, E), which never forms it.  A factor without
    entries gives the empty matrix and no device is touched.  Nothing is printed.
    """
    what = "kronecker_product"
    D, E = _as_csr(D), _as_csr(E)
    shape, nnz = _kron_shape(D, E, what)
    if nnz > _INT32_MAX - 1:
        raise ValueError(f"{what}: nnz(D) * nnz(E) = {D.nnz} * {E.nnz} = {nnz} entries do not fit one operand (int32 row "
                         "pointers, at most 2^31 - 2); use KroneckerOperand(D, E), which applies the factors without forming Q")
    if nnz == 0:
        return PinnedOperand._adopt(None, None, shape) if pin else _zero_result(shape)
    ctx = default_context()

    return with_leases(ctx, (D, E), lambda ld, le: _deliver_operand(ctx, lambda: ctx.kron_build(ld.handle, le.handle), shape, pin,
                                                                    False, _result_device))


def _zero_result(shape, sparse=True):
    """An all-zero product: on the device under set_result_device(True), else a scipy CSR (sparse) or numpy array."""
    if not sparse:
        return _dense_zeros(shape, _result_device)
    if not _result_device:
        return csr_matrix(shape)
    import torch
    dev = _torch_device(default_context())
    return DeviceCSRResult(torch.zeros(shape[0] + 1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                           torch.empty(0, dtype=torch.float64, device=dev), shape)


def _product_on_device(ctx, la, lb, triple, dense, symmetric, full, mirror):
    """The product of two leased operands with the result left in HBM (torch tensors), through _on_device; the flags are
    those sparse_matrix_multiply worked out."""
    import torch
    dev = _torch_device(ctx)
    a, b = la.handle, lb.handle

    def call():
        if triple:
            out = torch.empty((a.rows, a.rows), dtype=torch.float64, device=dev)
            ctx.triple_into(a, b, out.data_ptr(), full=full, exact=_exact, mirror=mirror)
            return out
        if dense:
            out = torch.empty((a.rows, b.cols), dtype=torch.float64, device=dev)
            ctx.dense_into(a, b, out.data_ptr(), symmetric=symmetric, exact=_exact, mirror=mirror)
            return out
        if mirror:
            return DeviceCSRResult(*ctx.spgemm_mirrored_torch(a, b, exact=_exact), (a.rows, b.cols))
        plan, release = plan_for(ctx, la, lb, symmetric, _exact)
        try:
            indptr = torch.empty(a.rows + 1, dtype=torch.int64, device=dev)
            indices = torch.empty(plan.nnz, dtype=torch.int32, device=dev)
            data = torch.empty(plan.nnz, dtype=torch.float64, device=dev)
            plan.numeric_into(indptr.data_ptr(), indices.data_ptr(), data.data_ptr())
        finally:
            release()
        return DeviceCSRResult(indptr, indices, data, (a.rows, b.cols))

    return _on_device(ctx, call)


def _as_csr(x):
    # reference :307-310: anything csr_matrix() accepts; no sort, no dedup
    if isinstance(x, KroneckerOperand):
        raise ValueError("a KroneckerOperand is accepted as matrix_a of sparse_dense_multiply, as matrix_q of "
                         "triple_product_apply, innovation_solve and sparse_triple_product(..., mask=) and as matrix_b of "
                         "masked_matrix_multiply only; build the explicit matrix with kronecker_product(D, E)")
    return x if (isspmatrix_csr(x) or isinstance(x, PinnedOperand)) else csr_matrix(x)


def _hq_operands(matrix_h, matrix_q, what):
    """(H, Q, kron) of a call on H Q H^T: H as CSR or PinnedOperand, Q the same or -- kron -- a KroneckerOperand with square
    factors.  ValueError unless Q is square and H's columns are Q's rows."""
    matrix_h = _as_csr(matrix_h)
    kron = isinstance(matrix_q, KroneckerOperand)
    if kron:
        matrix_q._square(what)
    else:
        matrix_q = _as_csr(matrix_q)
    if matrix_q.shape[0] != matrix_q.shape[1]:
        raise ValueError(f"{what}: Q must be square, got {matrix_q.shape[0]} x {matrix_q.shape[1]}")
    if matrix_h.shape[1] != matrix_q.shape[0]:
        raise ValueError("Matrix dimensions are incompatible for multiplication.")
    return matrix_h, matrix_q, kron


def _q_operands(matrix_q, kron, canonical_for=None):
    """What a call leases for Q: the matrix, or the two factors of a KroneckerOperand -- as they are, or canonical for the
    masked product `canonical_for`, which searches their rows.  The engine's twin methods then take the handles as
    fn(h, *q, ...)."""
    if not kron:
        return (matrix_q,)
    return matrix_q._canonical_factors(canonical_for) if canonical_for else matrix_q.factors


def _result_csr(indptr, indices, data, shape):
    """reference sparsemat_to_csr (:205-228): nzmax==0 -> empty matrix; int32 index arrays.  A result
    with nnz >= 2^31 -- which the reference's int32 structs cannot represent -- carries int64
    indptr AND indices (engine.spgemm_host widens the indices while it copies them out): scipy's kernels
    take one index dtype per matrix."""
    if len(indices) == 0:
        return csr_matrix(shape)
    if indices.dtype == np.int32:
        indptr = indptr.astype(np.int32)
    out = csr_matrix(shape, dtype=np.float64)
    # assign the arrays directly: the constructor would be free to check/copy, and must not
    # sort -- the reference returns first-touch order
    out.data, out.indices, out.indptr = data, indices, indptr
    return out


def sparse_matrix_multiply(matrix_a, matrix_b, output_format='sparse', symmetric=False, imem_size=None,
                           use_triple_product=False, compute_full_matrix=None):
    """Multiply two sparse matrices on the GPU.

    matrix_a, matrix_b : scipy CSR, or anything csr_matrix() accepts.
    output_format      : 'sparse' -> scipy.sparse.csr_matrix, 'dense' -> numpy.ndarray.
    symmetric          : keep only the upper triangle (i <= j) of a square result.
    imem_size          : the reference's CPU scratch hint; validated, then ignored.
    use_triple_product : return matrix_a @ matrix_b @ matrix_a.T as a dense array (upper
                         triangle unless compute_full_matrix=1); output_format/symmetric are
                         then ignored, as in the reference (:325).
    compute_full_matrix: None/0/1, see above (1 reproduces the reference exactly).
    """
    if imem_size is None:                                    # reference :288-295
        imem_size = 5
    else:
        try:
            imem_size = int(imem_size)
        except ValueError:
            raise ValueError(f"imem_size must be an integer or None, got {type(imem_size)}")

    if compute_full_matrix is None:                          # reference :298-304
        compute_full_matrix = 0
    else:
        if isinstance(compute_full_matrix, str) and compute_full_matrix == 'mirror' and use_triple_product:
            compute_full_matrix = 'mirror'                  # extension: S itself, lower triangle mirrored
        elif compute_full_matrix not in (0, 1):
            raise ValueError("compute_full_matrix must be None, 0, or 1")
        else:
            compute_full_matrix = int(compute_full_matrix)

    matrix_a = _as_csr(matrix_a)
    matrix_b = _as_csr(matrix_b)

    if matrix_a.shape[1] != matrix_b.shape[0]:               # reference :312-313
        raise ValueError("Matrix dimensions are incompatible for multiplication.")

    out_shape = (matrix_a.shape[0], matrix_b.shape[1])
    if matrix_a.nnz == 0 or matrix_b.nnz == 0:               # reference :315-319
        return _zero_result(out_shape, output_format == 'sparse')

    if symmetric and out_shape[0] != out_shape[1]:           # reference :321-322
        raise ValueError("For symmetric output, the resulting matrix must be square.")

    if not use_triple_product and output_format not in ('sparse', 'dense'):
        # reference :367-368 raises inside its try and :377-387 prints and returns zeros
        print("An error occurred during matrix multiplication: Invalid output_format. Choose 'sparse' or 'dense'.")
        return np.zeros(out_shape)

    ctx = default_context()
    symmetric, dense, full = bool(symmetric), output_format == 'dense', compute_full_matrix == 1
    if use_triple_product:
        mirror = compute_full_matrix == 'mirror' or (_full_symmetric and compute_full_matrix == 0)
    else:
        mirror = symmetric and _full_symmetric

    def product(la, lb):
        a, b = la.handle, lb.handle
        if _result_device:
            return _product_on_device(ctx, la, lb, use_triple_product, dense, symmetric, full, mirror)
        if use_triple_product:                                   # reference :325-336
            return ctx.triple_host(a, b, full=full, exact=_exact, mirror=mirror)
        if dense:                                                # reference :353-365
            return ctx.dense_host(a, b, symmetric=symmetric, exact=_exact, mirror=mirror)
        if mirror:
            # opt-in mirror epilogue: the full symmetric CSR (row i = mirrored entries in ascending column
            # order, then the reference's upper-triangle row in its first-touch order)
            return _result_csr(*ctx.spgemm_host_mirrored(a, b, exact=_exact), out_shape)
        plan, release = plan_for(ctx, la, lb, symmetric, _exact)  # reference :338-351
        try:
            indptr, indices, data = plan.numeric_host()
        finally:
            release()
        return _result_csr(indptr, indices, data, out_shape)

    result = with_leases(ctx, (matrix_a, matrix_b), product)

    if _result_device and not isinstance(result, (np.ndarray, csr_matrix)):
        empty = result.nnz == 0 if isinstance(result, DeviceCSRResult) else not bool(result.any())
        if empty:
            print("Multiplication resulted in a zero matrix.")
        return result
    if isinstance(result, np.ndarray):                       # reference :370-373
        # (the first row decides almost always; a full scan of a 20 GB result costs 0.7 s)
        if not (result[:1].any() or result.any()):
            print("Multiplication resulted in a zero matrix.")
    elif result.nnz == 0:
        print("Multiplication resulted in a zero matrix.")
    return result


def sparse_triple_product(matrix_h, matrix_q, compute_full_matrix=False, mask=None):
    """S = H @ Q @ H.T with a SPARSE result, computed on the GPU without any n x n or n x K array.

    matrix_h : n x K, matrix_q : K x K (scipy CSR, anything csr_matrix() accepts, or a PinnedOperand).
    Returns an n x n scipy CSR (a DeviceCSRResult under set_result_device(True)) holding the upper triangle k >= i
    with columns in ascending order; compute_full_matrix=True returns the full symmetric matrix (the upper triangle
    mirrored -- not the reference's doubled off-diagonal of use_triple_product with compute_full_matrix=1).  The
    pattern is structural: (i, k) is stored iff row i of H @ Q and row k of H share a stored column.  Under
    set_exact(True) the values are bit-identical to sparse_matrix_multiply(H, Q, use_triple_product=True) at the
    stored positions; otherwise within 1e-10 relative.  For an S that is nearly full the dense triple product is
    the faster tool.

    mask (n x n; scipy CSR, anything csr_matrix() accepts, or a PinnedOperand): S only at the positions of the mask
    with k >= i (its values are ignored; positions without a structural contribution hold +0.0), without building the
    structural pattern.  compute_full_matrix=True mirrors that upper part; mask entries below the diagonal are ignored.

    With a mask, matrix_q may be a KroneckerOperand(D, E) (square factors, p * r == K): the entries of H (D (x) E) H^T are
    then built from the factors, and neither Q nor H Q is ever formed.  The values are those of the same call on
    kronecker_product(D, E) -- bit for bit under set_exact(True).  The factors' rows are searched, so a scipy factor that is
    not canonical is canonicalised on a host copy and a pinned one that is not canonical is a ValueError.  Without a mask a
    KroneckerOperand is refused: the structural pattern needs the explicit matrix of kronecker_product(D, E).
    """
    what = "sparse_triple_product"
    if mask is None and isinstance(matrix_q, KroneckerOperand):
        raise ValueError("sparse_triple_product: a KroneckerOperand as matrix_q needs a pattern -- pass mask= (the structural "
                         "pattern would need the symbolic phase of a Q that is never formed); without a mask, build the "
                         "explicit matrix with kronecker_product(D, E)")
    matrix_h, matrix_q, kron = _hq_operands(matrix_h, matrix_q, what)
    n = matrix_h.shape[0]
    out_shape = (n, n)
    full = bool(compute_full_matrix)
    if mask is not None:
        mask = _as_csr(mask)
        _check_mask_shape(mask, out_shape, what)
        if mask.nnz == 0:
            return _zero_result(out_shape)
        if matrix_h.nnz == 0 or matrix_q.nnz == 0:
            return _zeros_on_mask(mask, out_shape, upper=True, mirror=full)
    elif matrix_h.nnz == 0 or matrix_q.nnz == 0:
        return _zero_result(out_shape)
    ctx = default_context()
    mats = (matrix_h,) + _q_operands(matrix_q, kron, what) + (() if mask is None else (_canonical_mask(mask),))

    def body(lh, *rest):
        h, m = lh.handle, (rest[-1].handle if mask is not None else None)
        q = (rest[0].handle, rest[1].handle) if kron else rest[0].handle
        if _result_device:
            return _on_device(ctx, lambda: DeviceCSRResult(*ctx.triple_sparse_torch(h, q, full=full, exact=_exact, mask=m), out_shape))
        return _result_csr(*ctx.triple_sparse_host(h, q, full=full, exact=_exact, mask=m), out_shape)

    return with_leases(ctx, mats, body)


# ------------------------------------------------------------------ products on a given pattern
def _check_mask_shape(mask, shape, what):
    if tuple(mask.shape) != tuple(shape):
        raise ValueError(f"{what}: the mask is {mask.shape[0]} x {mask.shape[1]}, expected {shape[0]} x {shape[1]}")


def _canonical_mask(mask):
    """The mask with strictly ascending rows.  A scipy mask that is not canonical is canonicalised on a host copy
    (duplicates merged, columns sorted; explicitly stored zeros stay positions); a PinnedOperand must be canonical."""
    if isinstance(mask, PinnedOperand):
        if mask.nnz and not mask._handle.is_canonical():
            raise ValueError("the mask PinnedOperand is not canonical (rows must hold strictly ascending columns): "
                             "pin mask.sorted_indices() after sum_duplicates()")
        return mask
    if not mask.has_canonical_format:
        mask = mask.copy()
        mask.sum_duplicates()
    return mask


def _mask_pattern(mask):
    """(indptr, indices) of a canonical mask as int32 host arrays."""
    if isinstance(mask, PinnedOperand):
        if not mask.nnz:
            return np.zeros(mask.shape[0] + 1, dtype=np.int32), np.empty(0, dtype=np.int32)
        indptr, indices, _ = mask._handle.to_host()
        return indptr, indices
    nnz = int(mask.indptr[-1])
    return mask.indptr.astype(np.int32), mask.indices[:nnz].astype(np.int32)


def _pattern_result(ctx, indptr, indices, data, shape):
    """A result on a host pattern: scipy CSR, or a DeviceCSRResult under set_result_device(True) (data may be a
    torch tensor already)."""
    if _result_device:
        return DeviceCSRResult(*(_as_kind(x, True, ctx) for x in (indptr.astype(np.int64), indices, data)), shape)
    return _result_csr(indptr, indices, data, shape)


def _zeros_on_mask(mask, shape, upper=False, mirror=False, scale=False):
    """The product on a pattern when an operand has no entries: the canonical mask's pattern filled with +0.0, built on
    the host -- no device unless the result lives there or a pinned mask must be read.  upper: only the positions with
    column >= row (the masked triple product), mirrored into the lower triangle too with mirror.  scale: w * (+0.0) for
    the mask's stored weights (sampled_dense_product's scale_by_mask)."""
    ctx = default_context() if (_result_device or isinstance(mask, PinnedOperand)) else None
    mask = _canonical_mask(mask)
    indptr, indices = _mask_pattern(mask)
    if upper:
        rows = np.repeat(np.arange(shape[0], dtype=np.int64), np.diff(indptr))
        keep = indices >= rows
        up = csr_matrix((np.ones(int(keep.sum())), (rows[keep], indices[keep])), shape=shape)
        if mirror:
            up = (up + up.T).tocsr()
        up.sort_indices()
        indptr, indices = up.indptr.astype(np.int32), up.indices.astype(np.int32)
    data = np.zeros(len(indices), dtype=np.float64)
    if scale:
        weights = mask._handle.to_host()[2] if isinstance(mask, PinnedOperand) else mask.data[:len(indices)]
        with np.errstate(invalid="ignore"):
            data = np.asarray(weights, dtype=np.float64) * data      # (w * +0.0: the weight's sign stays, inf gives NaN)
    return _pattern_result(ctx, indptr, indices, data, shape)


def _values_on_mask(ctx, mask, lease, data, shape):
    """The result of a product on a pattern: `data`, a numpy array or a tensor left in HBM, in the order of the canonical
    mask (leased as `lease`).  A pinned mask whose result stays in HBM hands its pattern over device to device; every
    other case goes through the host pattern."""
    if _result_device and isinstance(mask, PinnedOperand):
        import torch
        indptr, indices = lease.handle.pattern_torch()
        return DeviceCSRResult(indptr.to(torch.int64), indices, data, shape)
    if _is_torch(data) and not _result_device:
        data = data.cpu().numpy()
    return _pattern_result(ctx, *_mask_pattern(mask), data, shape)


def masked_matrix_multiply(matrix_a, matrix_b, mask):
    """C = (A @ B) evaluated only at the positions of `mask` (GraphBLAS masked mxm / SDDMM with sparse operands).

    matrix_a : m x K, matrix_b : K x n, mask : m x n (scipy CSR, anything csr_matrix() accepts, or a PinnedOperand).
    C's pattern is exactly the mask's (canonicalised: columns strictly ascending); the mask's values are ignored and
    its explicitly stored zeros are positions.  A position where no product A[i,k] * B[k,j] exists holds +0.0 and is
    stored (C.eliminate_zeros() drops such entries).  Under set_exact(True) every value that
    sparse_matrix_multiply(A, B) stores is reproduced bit for bit; otherwise within 1e-10 relative.  A pair (k, j)
    that row i of A does not store is never multiplied.  Returns a scipy CSR (a DeviceCSRResult under
    set_result_device(True)).  Nothing is printed.

    matrix_b may be a KroneckerOperand(D, E) with p * r == K (the mask is then m x p' r'): the entries of A (D (x) E) are built
    from the factors and Q is never formed; the values are those of the same call on kronecker_product(D, E), bit for bit
    under set_exact(True).  Factors that are not canonical: as in sparse_triple_product.
    """
    matrix_a = _as_csr(matrix_a)
    kron = isinstance(matrix_b, KroneckerOperand)
    if not kron:
        matrix_b = _as_csr(matrix_b)
    mask = _as_csr(mask)
    if matrix_a.shape[1] != matrix_b.shape[0]:
        raise ValueError("Matrix dimensions are incompatible for multiplication.")
    out_shape = (matrix_a.shape[0], matrix_b.shape[1])
    _check_mask_shape(mask, out_shape, "masked_matrix_multiply")
    if mask.nnz == 0:
        return _zero_result(out_shape)
    if matrix_a.nnz == 0 or matrix_b.nnz == 0:
        return _zeros_on_mask(mask, out_shape)
    ctx = default_context()
    mask = _canonical_mask(mask)
    into, host = (ctx.spgemm_masked_kron_into, ctx.spgemm_masked_kron_host) if kron else (ctx.spgemm_masked_into, ctx.spgemm_masked_host)

    def body(la, *rest):
        lm, b = rest[-1], [lease.handle for lease in rest[:-1]]
        if not _result_device:
            return _values_on_mask(ctx, mask, lm, host(la.handle, *b, lm.handle, exact=_exact), out_shape)
        import torch

        def call():
            data = torch.empty(lm.handle.nnz, dtype=torch.float64, device=_torch_device(ctx))
            into(la.handle, *b, lm.handle, data.data_ptr(), exact=_exact)
            return data

        return _values_on_mask(ctx, mask, lm, _on_device(ctx, call), out_shape)

    return with_leases(ctx, (matrix_a,) + _q_operands(matrix_b, kron, "masked_matrix_multiply") + (mask,), body)


# ------------------------------------------------------------------ sparse x dense
def _dense_operand(x, rows, what, name="X"):
    """(X, k, is_torch): X a float64 C-contiguous numpy array, or a float64 CUDA tensor with unit column stride; 1-D or
    2-D with `rows` rows.  ValueError before any device work (`name`: what the messages call the operand)."""
    is_torch = _is_torch(x)
    if is_torch:
        import torch
        if x.dtype != torch.float64 or not x.is_cuda:
            raise ValueError(f"{what}: a torch {name} must be a float64 CUDA tensor")
        if x.dim() <= 2 and (x.stride(-1) != 1 or (x.dim() == 2 and x.stride(0) < x.shape[1])):
            x = x.contiguous()
    else:
        x = np.asarray(x, dtype=np.float64)
        x = np.ascontiguousarray(x) if x.ndim else x          # (ascontiguousarray would make a 0-d X 1-D)
    ndim = x.dim() if is_torch else x.ndim
    if ndim not in (1, 2):
        raise ValueError(f"{what}: {name} must be 1-D or 2-D, got {ndim} dimensions")
    if x.shape[0] != rows:
        raise ValueError(f"{what}: {name} has {x.shape[0]} rows, expected {rows}")
    return x, (1 if ndim == 1 else int(x.shape[1])), is_torch


def _dense_apply(ctx, x, k, is_torch, out_rows, what, host_call, device_call):
    """One sparse x dense product: numpy in and out through host_call(x) -> y, or on the device (torch X, or
    set_result_device(True)) through device_call(d_x, ldx, k, d_y, ldy) into a torch result."""
    if not (is_torch or _result_device):
        return host_call(x)
    import torch
    x = _to_device(ctx, x, is_torch, what, "X")
    y = torch.empty((out_rows,) if x.dim() == 1 else (out_rows, k), dtype=torch.float64, device=x.device)
    device_call(x, 1 if x.dim() == 1 else x.stride(0), k, y, k)
    return y


def sparse_dense_multiply(matrix_a, x, transpose=False):
    """Y = A @ X, or A.T @ X with transpose=True, for a sparse A and a dense X, on the GPU.

    matrix_a : scipy CSR, anything csr_matrix() accepts, or a PinnedOperand (the operand cache applies); or a
               KroneckerOperand(D, E): Y = (D (x) E) X through the factors, E first (transpose=False only; under
               set_exact(True) bit-identical to scipy's D @ (E @ X[t]) stacked over t, not to kron(D, E) @ X).
    x        : a numpy array (cast to float64, C-contiguous) or a float64 CUDA tensor on the library's device; 1-D or
               2-D.  A 1-D X gives a 1-D result.
    Returns numpy for numpy input; a torch tensor on the device for torch input or under set_result_device(True).
    Under set_exact(True) the result is bit-identical to scipy's A @ X / A.T @ X (each element starts at +0.0 and adds
    the row's products in stored order); otherwise within 1e-10 of (|A| |X|)[i, j].  A pair that row i does not store is
    never multiplied.  A.T comes from a transpose built on the device once and kept with the operand.
    """
    kron = isinstance(matrix_a, KroneckerOperand)
    if kron and transpose:
        raise ValueError("sparse_dense_multiply: a KroneckerOperand has no transpose flag: (D (x) E)^T = D^T (x) E^T, so pass "
                         "KroneckerOperand(D.T, E.T)")
    if not kron:
        matrix_a = _as_csr(matrix_a)
    m, kx = matrix_a.shape[::-1] if transpose else matrix_a.shape
    x, k, is_torch = _dense_operand(x, kx, "sparse_dense_multiply")
    out_shape = (m,) if len(x.shape) == 1 else (m, k)
    if matrix_a.nnz == 0 or k == 0 or m == 0:
        return _dense_zeros(out_shape, is_torch or _result_device)
    ctx = default_context()
    host, into = (ctx.kron_apply_host, ctx.kron_apply_into) if kron else (ctx.spmm_host, ctx.spmm_into)
    flags = {"exact": _exact} if kron else {"transpose": transpose, "exact": _exact}

    def body(*leases):
        a = [lease.handle for lease in leases]
        return _dense_apply(ctx, x, k, is_torch, m, "sparse_dense_multiply",
                            lambda xh: host(*a, xh, **flags), lambda *dev: into(*a, *dev, **flags))

    return with_leases(ctx, _q_operands(matrix_a, kron), body)


def triple_product_apply(matrix_h, matrix_q, x):
    """Y = H @ (Q @ (H.T @ X)) = S X with S = H Q H^T never formed, on the GPU.

    matrix_h : n x K, matrix_q : K x K (need not be symmetric); scipy CSR, anything csr_matrix() accepts, or a
    PinnedOperand.  matrix_q may be a KroneckerOperand(D, E) with square factors and p * r == K: Q = D (x) E is then applied
    through its factors (sparse_dense_multiply's order) and never formed.  x : n x k or n, as in sparse_dense_multiply (numpy or a float64 CUDA tensor).  Returns the same kind
    and shape as x (a torch tensor under set_result_device(True)).  Under set_exact(True) bit-identical to scipy's
    H @ (Q @ (H.T @ X)); otherwise within rounding.  X is processed in column blocks whose two K x block intermediates fit
    the context's budget (Context.tune_spmm; blocking changes no bit).
    """
    what = "triple_product_apply"
    matrix_h, matrix_q, kron = _hq_operands(matrix_h, matrix_q, what)
    n = matrix_h.shape[0]
    x, k, is_torch = _dense_operand(x, n, what)
    out_shape = (n,) if len(x.shape) == 1 else (n, k)
    if matrix_h.nnz == 0 or matrix_q.nnz == 0 or k == 0 or n == 0:
        return _dense_zeros(out_shape, is_torch or _result_device)
    ctx = default_context()
    host, into = (ctx.triple_apply_kron_host, ctx.triple_apply_kron_into) if kron else (ctx.triple_apply_host, ctx.triple_apply_into)

    def body(*leases):
        hq = [lease.handle for lease in leases]
        return _dense_apply(ctx, x, k, is_torch, n, what,
                            lambda xh: host(*hq, xh, exact=_exact), lambda *dev: into(*hq, *dev, exact=_exact))

    return with_leases(ctx, (matrix_h,) + _q_operands(matrix_q, kron), body)


# ------------------------------------------------------------------ (X Y^T) on a pattern
def _dense_2d(x, rows, what, name):
    """_dense_operand for an operand that must be 2-D: (X, k, is_torch)."""
    ndim = x.dim() if _is_torch(x) else np.ndim(x)
    if ndim != 2:
        raise ValueError(f"{what}: {name} must be 2-D, got {ndim} dimensions")
    return _dense_operand(x, rows, what, name)


def sampled_dense_product(x, y, mask, scale_by_mask=False):
    """C = (X @ Y.T) evaluated only at the positions of `mask`, on the GPU (SDDMM with dense operands; the dense
    counterpart of masked_matrix_multiply).

    x    : m x k, y : n x k (None means y = x, the covariance case X @ X.T); each a 2-D numpy array (cast to float64,
           C-contiguous) or a float64 CUDA tensor on the library's device.  One row holds one state variable's ensemble
           members.  A strided tensor with unit column stride (a column slice of a wider tensor) is used in place.
    mask : m x n; scipy CSR, anything csr_matrix() accepts, or a PinnedOperand (the operand cache applies).
    C's pattern is exactly the mask's (canonicalised: columns strictly ascending, duplicates merged); explicitly stored
    zeros are positions.  With scale_by_mask every value is multiplied by the mask's stored value -- C = mask * (X @ Y.T)
    elementwise, merged duplicates carrying their summed weight (the localised covariance Q = L o (E E^T)); without it
    the mask's values are ignored.  Under set_exact(True) C[i,j] is bit-identical to s = 0.0; s += X[i,e] * Y[j,e] for
    e = 0 .. k-1 (times the weight); otherwise within 1e-10 of (|X| @ |Y|.T)[i,j] (times |weight|), in a summation order
    that depends on k only: the same (i, j) gives the same bits whatever the mask.  X[i,:] and Y[j,:] are read only for
    the positions that name them.  Returns a scipy CSR (a DeviceCSRResult under set_result_device(True)).  Nothing is
    printed.
    """
    what = "sampled_dense_product"
    mask = _as_csr(mask)
    m, n = mask.shape
    x, k, x_torch = _dense_2d(x, m, what, "X")
    if y is None:
        if m != n:
            raise ValueError(f"{what}: Y has {m} rows, expected {n}")
        y, y_torch = x, x_torch
    else:
        y, ky, y_torch = _dense_2d(y, n, what, "Y")
        if ky != k:
            raise ValueError(f"{what}: X has {k} columns, Y has {ky}")
    out_shape = (m, n)
    if mask.nnz == 0:
        return _zero_result(out_shape)
    if k == 0:
        return _zeros_on_mask(mask, out_shape, scale=scale_by_mask)
    ctx = default_context()
    mask = _canonical_mask(mask)

    def body(lm):
        if not (x_torch or y_torch or _result_device):
            data = ctx.sddmm_host(lm.handle, x, None if y is x else y, scale=scale_by_mask, exact=_exact)
            return _values_on_mask(ctx, mask, lm, data, out_shape)
        import torch
        dx = _to_device(ctx, x, x_torch, what, "X")
        dy = dx if y is x else _to_device(ctx, y, y_torch, what, "Y")

        def call():
            data = torch.empty(lm.handle.nnz, dtype=torch.float64, device=dx.device)
            ctx.sddmm_into(lm.handle, dx, dx.stride(0), dy, dy.stride(0), k, data, scale=scale_by_mask, exact=_exact)
            return data

        return _values_on_mask(ctx, mask, lm, _on_device(ctx, call), out_shape)

    return with_leases(ctx, (mask,), body)


# ------------------------------------------------------------------ CG on (H Q H^T + R) Z = D
CG_LANES = 2048          # SMM_CG_LANES of include/smm_hip.h: the dot product's number of partial sums


def _cg_dot(u, v):
    """Column-wise dot(u, v) in the library's fixed order: CG_LANES partial sums over strided rows, then a halving tree."""
    n, k = u.shape
    s = np.zeros((CG_LANES, k))
    for i0 in range(0, n, CG_LANES):
        m = min(CG_LANES, n - i0)
        s[:m] = s[:m] + u[i0:i0 + m] * v[i0:i0 + m]
    h = CG_LANES // 2
    while h:
        s = s[:h] + s[h:2 * h]
        h //= 2
    return s[0]


def _cg_on_host(apply, d, tol, maxiter, record=False):
    """The iteration of smm_innovation_solve in numpy, for the systems that never reach the device (S = 0): apply(P)
    is (S + R) P.  Returns (Z, info); with record, info.alpha and info.beta are the maxiter x k histories by the contract
    of smm_innovation_solve_coef."""
    n, k = d.shape
    info = SolveInfo(k, maxiter if record else None)
    x, r, p = np.zeros((n, k)), d.copy(), d.copy()
    with np.errstate(all="ignore"):
        rho = _cg_dot(r, r)
        thr = (tol * tol) * rho
        info.rhs_sq[:] = rho
        info.residual_sq[:] = rho
        live = ~(rho <= thr)
        info.status[live] = SolveInfo.ITERATION_LIMIT
        for it in range(1, maxiter + 1):
            if not live.any():
                break
            w = apply(p)
            pw = _cg_dot(p, w)
            broke = live & ~(pw > 0)
            info.status[broke], info.iterations[broke] = SolveInfo.BREAKDOWN, it - 1
            live = live & ~broke
            j = np.flatnonzero(live)
            alpha = rho[j] / pw[j]
            if record:
                info.alpha[it - 1, j] = alpha
            x[:, j] = x[:, j] + alpha * p[:, j]
            r[:, j] = r[:, j] - alpha * w[:, j]
            rho_new = _cg_dot(r[:, j], r[:, j])
            info.residual_sq[j], info.iterations[j] = rho_new, it
            done = rho_new <= thr[j]
            info.status[j[done]] = SolveInfo.CONVERGED
            live[j[done]] = False
            j, rho_new = j[~done], rho_new[~done]
            beta = rho_new / rho[j]
            if record:
                info.beta[it - 1, j] = beta
            p[:, j] = r[:, j] + beta * p[:, j]
            rho[j] = rho_new
    return x, info


def _innovation_operands(matrix_h, matrix_q, matrix_r, what):
    """(H, Q, R, kron, n) of a call on H Q H^T + R: H and Q as CSR or PinnedOperand (Q a KroneckerOperand when kron), R the
    same, built from its diagonal when a vector, or None (also for an R without entries).  ValueError for shapes that do
    not fit."""
    matrix_h, matrix_q, kron = _hq_operands(matrix_h, matrix_q, what)
    n = matrix_h.shape[0]
    if matrix_r is not None:
        if not (isspmatrix_csr(matrix_r) or isinstance(matrix_r, PinnedOperand) or hasattr(matrix_r, "tocsr")):
            dense_r = np.asarray(matrix_r, dtype=np.float64)
            if dense_r.ndim == 1:                        # the diagonal; zeros stay stored
                if dense_r.shape[0] != n:
                    raise ValueError(f"{what}: the diagonal of R has {dense_r.shape[0]} entries, expected {n}")
                matrix_r = csr_matrix((dense_r, np.arange(n, dtype=np.int32), np.arange(n + 1, dtype=np.int32)), shape=(n, n))
        matrix_r = _as_csr(matrix_r)
        if tuple(matrix_r.shape) != (n, n):
            raise ValueError(f"{what}: R must be {n} x {n}, got {matrix_r.shape[0]} x {matrix_r.shape[1]}")
        if matrix_r.nnz == 0:
            matrix_r = None
    return matrix_h, matrix_q, matrix_r, kron, n


def _innovation_leased(matrix_h, matrix_q, matrix_r, kron):
    """The operands an innovation call leases: H, Q or its two factors, then R unless it is None."""
    return (matrix_h,) + _q_operands(matrix_q, kron) + (() if matrix_r is None else (matrix_r,))


def _innovation_handles(leases, kron):
    """(h, q, r) of the leases of _innovation_leased: q a list of one handle or two, r None without R."""
    handles = [lease.handle for lease in leases]
    nq = 2 if kron else 1
    return handles[0], handles[1:1 + nq], (handles[1 + nq] if len(handles) > 1 + nq else None)


def _innovation_tol(tol, what):
    try:
        tol = float(tol)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: tol must be a finite positive number") from None
    if not (tol > 0.0 and np.isfinite(tol)):
        raise ValueError(f"{what}: tol must be a finite positive number, got {tol}")
    return tol


def _host_r_apply(matrix_r):
    """P -> R P on the host, for the systems whose S has no entries (R: CSR, PinnedOperand or None)."""
    if matrix_r is None:
        return np.zeros_like
    if isinstance(matrix_r, PinnedOperand):
        ctx = default_context()
        return lambda p: 0.0 + with_leases(ctx, (matrix_r,), lambda lr: ctx.spmm_host(lr.handle, p, exact=True))
    return lambda p: 0.0 + np.asarray(matrix_r @ p)


def innovation_solve(matrix_h, matrix_q, matrix_r, d, tol=1e-8, maxiter=None):
    """(Z, info) with (H Q H^T + R) Z = D by conjugate gradients on the GPU; S = H Q H^T is never formed.

    matrix_h : n x K, matrix_q : K x K; scipy CSR, anything csr_matrix() accepts, or a PinnedOperand.  matrix_q may be a
               KroneckerOperand(D, E) (square factors, p * r == K): Q = D (x) E is applied through its factors, never formed.
    matrix_r : n x n in the same forms, a 1-D array of the n diagonal entries, or None for S alone.  S + R is expected
               to be symmetric positive definite.
    d        : n x k or n, numpy or a float64 CUDA tensor as in triple_product_apply.  Every column is its own CG from
               x0 = 0; all columns share each sparse x dense product.  Z has d's kind and shape (a torch tensor under
               set_result_device(True)).
    tol      : a column converges when the recurrence's ||r||^2 <= tol^2 ||d||^2.  maxiter : None means n.
    info     : a SolveInfo with per-column arrays iterations, status (0 converged, 1 iteration limit, 2 breakdown: p^T (S + R) p
               was not positive), residual_sq and rhs_sq.  Non-convergence is reported there, not raised.
    Dot products are summed in a fixed order (include/smm_hip.h); under set_exact(True) Z and info are bit-identical to
    that recipe in IEEE double, otherwise fused multiply-adds are used and two runs still agree bit for bit.  The vectors
    of a block of columns are sized by Context.tune_spmm's apply budget.
    """
    matrix_h, matrix_q, matrix_r, kron, n = _innovation_operands(matrix_h, matrix_q, matrix_r, "innovation_solve")
    d, k, is_torch = _dense_operand(d, n, "innovation_solve", "D")
    tol = _innovation_tol(tol, "innovation_solve")
    if maxiter is None:
        maxiter = n
    if int(maxiter) != maxiter or maxiter < 0:
        raise ValueError(f"innovation_solve: maxiter must be a non-negative integer, got {maxiter}")
    maxiter = int(maxiter)
    on_device = is_torch or _result_device
    if k == 0 or n == 0:
        return _dense_zeros(tuple(d.shape), on_device), SolveInfo(k)
    if matrix_h.nnz == 0 or matrix_q.nnz == 0:           # S = 0: R Z = D, iterated on the host
        z, info = _cg_on_host(_host_r_apply(matrix_r), _as_kind(d, False).reshape(n, k), tol, maxiter)
        return _as_kind(z.reshape(tuple(d.shape)), on_device), info
    ctx = default_context()
    host, into = (ctx.innovation_solve_kron_host, ctx.innovation_solve_kron_into) if kron else (ctx.innovation_solve_host, ctx.innovation_solve_into)

    def body(*leases):
        h, q, r = _innovation_handles(leases, kron)
        if not on_device:
            return host(h, *q, r, d, tol, maxiter, exact=_exact)
        import torch
        b = _to_device(ctx, d, is_torch, "innovation_solve", "D")
        z = torch.empty(tuple(b.shape), dtype=torch.float64, device=b.device)
        info = into(h, *q, r, b, 1 if b.dim() == 1 else b.stride(0), k, z, k, tol, maxiter, exact=_exact)
        return z, info

    return with_leases(ctx, _innovation_leased(matrix_h, matrix_q, matrix_r, kron), body)


# ------------------------------------------------------------------ log det(H Q H^T + R) by stochastic Lanczos quadrature
def _probe_signs(n, k, seed):
    """The probes of smm_probe_fill in numpy uint64 (include/smm_hip.h): n x k float64 of +-1.0."""
    u = np.uint64
    i = np.arange(1, n + 1, dtype=u)[:, None]
    c = np.arange(k, dtype=u)[None, :]
    z = np.array([int(seed) % (1 << 64)], dtype=u) + c * u(0xD1B54A32D192ED03) + i * u(0x9E3779B97F4A7C15)
    z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
    z = z ^ (z >> u(31))
    return np.where((z >> u(63)).astype(bool), -1.0, 1.0)


def _slq_column(alpha, beta, m, n):
    """(sample, theta): n * sum_i V[0, i]^2 ln(theta_i) of the m x m Lanczos tridiagonal that m CG iterations give
    (T[j, j] = 1/alpha_j + beta_{j-1}/alpha_{j-1}, T[j, j+1] = sqrt(beta_j)/alpha_j), and its eigenvalues (Ritz values).
    A Ritz value <= 0 makes the sample NaN; m = 0 gives (NaN, empty)."""
    if m == 0:
        return np.nan, np.empty(0)
    a, b = np.asarray(alpha[:m], np.float64), np.asarray(beta[:m], np.float64)
    with np.errstate(all="ignore"):
        diag = 1.0 / a
        diag[1:] = diag[1:] + b[:m - 1] / a[:m - 1]
        off = np.sqrt(b[:m - 1]) / a[:m - 1]
        T = np.diag(diag) + np.diag(off, 1) + np.diag(off, -1)
        if not np.all(np.isfinite(T)):
            return np.nan, np.empty(0)
        theta, V = np.linalg.eigh(T)
        return float(n * np.sum(V[0] ** 2 * np.log(theta))), theta


def _info_columns(info, cols):
    """The SolveInfo of a slice of columns (histories included)."""
    out = SolveInfo(0)
    for f in ("iterations", "status", "residual_sq", "rhs_sq"):
        setattr(out, f, np.ascontiguousarray(getattr(info, f)[cols]))
    if info.alpha is not None:
        out.alpha, out.beta = np.ascontiguousarray(info.alpha[:, cols]), np.ascontiguousarray(info.beta[:, cols])
    return out


class LogdetResult:
    """What innovation_logdet returns: logdet, stderr, samples, lambda_min, lambda_max, info, positive_definite, and --
    None unless asked for -- Z, info_d (with d) and solutions (with return_solutions)."""

    def __init__(self):
        self.logdet = self.stderr = self.lambda_min = self.lambda_max = np.nan
        self.samples = np.empty(0)
        self.info = self.Z = self.info_d = self.solutions = None
        self.positive_definite = True

    def __repr__(self):
        return (f"LogdetResult(logdet={self.logdet!r}, stderr={self.stderr!r}, probes={len(self.samples)}, "
                f"lambda_min={self.lambda_min!r}, lambda_max={self.lambda_max!r}, positive_definite={self.positive_definite})")


def _slq_result(res, info, n):
    """Fill res from the probe columns' SolveInfo: the tridiagonal quadrature of every probe, on the host."""
    k = len(info.iterations)
    res.info = info
    res.samples = np.full(k, np.nan)
    lo, hi = np.inf, -np.inf
    for c in range(k):
        if info.status[c] == SolveInfo.BREAKDOWN:
            res.positive_definite = False
            continue
        res.samples[c], theta = _slq_column(info.alpha[:, c], info.beta[:, c], int(info.iterations[c]), n)
        if theta.size:
            lo, hi = min(lo, float(theta[0])), max(hi, float(theta[-1]))
    res.lambda_min, res.lambda_max = (lo, hi) if lo <= hi else (np.nan, np.nan)
    res.logdet = float(np.mean(res.samples)) if res.positive_definite else np.nan
    res.stderr = float(np.std(res.samples, ddof=1) / np.sqrt(k)) if k > 1 else np.nan
    return res


def innovation_logdet(matrix_h, matrix_q, matrix_r, probes=32, seed=0, tol=1e-8, maxiter=None, d=None, return_solutions=False):
    """ln det(H Q H^T + R) by stochastic Lanczos quadrature read off the batched CG of innovation_solve; Psi = H Q H^T + R
    is never formed.  Returns a LogdetResult.

    matrix_h, matrix_q, matrix_r : as in innovation_solve (scipy CSR, PinnedOperand, a KroneckerOperand for Q, a vector for
               R's diagonal, R = None for S alone).  Psi is expected to be symmetric positive definite.
    probes   : the number of probes z_c with entries +-1, filled on the device by the hash of include/smm_hip.h from
               (seed, row, c): the same seed gives the same probes, and column c does not depend on `probes`.
    tol, maxiter : of the CG on Psi x = z_c; maxiter None means min(n, 1000), at most 65536 (it sizes the recorded histories).
    d        : optional right-hand sides, n or n x m, numpy or a float64 CUDA tensor.  Their columns go in front of the probes
               in the same batch, so Z = Psi^-1 d -- the quadratic form of a likelihood -- costs no extra products.  Columns
               never mix: under set_exact(True) Z and info_d are the bits of innovation_solve(H, Q, R, d).
    Result fields:
      logdet    the mean of samples;  stderr  their sample standard deviation / sqrt(probes) (NaN for a single probe)
      samples   per probe, n * sum_i V[0, i]^2 ln(theta_i): theta and V from numpy.linalg.eigh of the probe's m x m
                Lanczos tridiagonal (m its CG iterations), T[j, j] = 1/alpha_j + beta_{j-1}/alpha_{j-1},
                T[j, j+1] = T[j+1, j] = sqrt(beta_j)/alpha_j
      lambda_min, lambda_max  the extreme Ritz values over all probes (lambda_max converges to Psi's from below within a
                few iterations; lambda_min stays somewhat above Psi's)
      info      the SolveInfo of the probe columns, with the recorded alpha and beta (maxiter x probes)
      Z, info_d with d: of d's kind and shape, as innovation_solve returns them
      solutions with return_solutions: Psi^-1 times the probes, n x probes -- the input of the trace terms
                tr(Psi^-1 dPsi/dtheta); a torch tensor under set_result_device(True), numpy otherwise
      positive_definite  False when a probe broke down (status 2): logdet is then NaN -- the matrix is not positive
                definite; this is reported, not raised.  A probe that hit the iteration limit (status 1) contributes its
                m-point quadrature and info.converged is False.
    alpha and beta come from the device and follow the bit-for-bit contract of innovation_solve (fixed summation order; under
    set_exact(True) the numpy recipe's bits; otherwise two runs agree bit for bit).  The tridiagonal eigen-decompositions run
    on the host on purpose -- at most probes * maxiter^2 flops on matrices of a few hundred rows -- and are LAPACK's
    (numpy.linalg.eigh): samples, logdet and the Ritz values are deterministic on one machine but not part of that contract.
    n = 0 gives logdet 0.0.  H or Q without entries leaves Psi = R, iterated on the host without a device; R = None is then
    a ValueError (the matrix is singular).
    """
    what = "innovation_logdet"
    matrix_h, matrix_q, matrix_r, kron, n = _innovation_operands(matrix_h, matrix_q, matrix_r, what)
    try:
        ok = int(probes) == probes and probes >= 1
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{what}: probes must be a positive integer, got {probes!r}")
    probes = int(probes)
    try:
        seed = int(seed) % (1 << 64)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: seed must be an integer, got {seed!r}") from None
    tol = _innovation_tol(tol, what)
    if maxiter is None:
        maxiter = max(1, min(n, 1000))
    try:
        ok = int(maxiter) == maxiter and 1 <= maxiter <= 65536
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{what}: maxiter must be an integer in 1 .. 65536, got {maxiter!r}")
    maxiter = int(maxiter)
    m, is_torch = 0, False
    if d is not None:
        d, m, is_torch = _dense_operand(d, n, what, "D")
    on_device = is_torch or _result_device
    res = LogdetResult()

    def finish(z, info):
        """Split the batch (numpy, or a tensor on the device path) into d's columns and the probes', each of the kind
        the caller gets."""
        def part(cols, on_device):
            return _as_kind(cols.contiguous() if _is_torch(cols) else np.ascontiguousarray(cols), on_device)

        if d is not None:
            res.Z = part(z[:, :m].reshape(tuple(d.shape)), on_device)
            res.info_d = _info_columns(info, slice(0, m))
        if return_solutions:
            res.solutions = part(z[:, m:], _result_device)
        return _slq_result(res, _info_columns(info, slice(m, m + probes)), n)

    if n == 0:
        res.info = SolveInfo(probes, maxiter)
        res.samples = np.zeros(probes)
        res.logdet, res.stderr = 0.0, (0.0 if probes > 1 else np.nan)
        if d is not None:
            res.Z, res.info_d = _dense_zeros(tuple(d.shape), on_device), SolveInfo(m)
        if return_solutions:
            res.solutions = _dense_zeros((0, probes), _result_device)
        return res
    if matrix_h.nnz == 0 or matrix_q.nnz == 0:           # Psi = R: iterated on the host, as innovation_solve does
        if matrix_r is None:
            raise ValueError(f"{what}: H Q H^T has no entries and R is None: the matrix is singular")
        batch = _probe_signs(n, probes, seed)
        if d is not None:
            batch = np.concatenate([_as_kind(d, False).reshape(n, m), batch], axis=1)
        return finish(*_cg_on_host(_host_r_apply(matrix_r), np.ascontiguousarray(batch), tol, maxiter, record=True))
    ctx = default_context()
    solve = ctx.innovation_solve_coef_kron_into if kron else ctx.innovation_solve_coef_into

    def body(*leases):
        import torch
        h, q, r = _innovation_handles(leases, kron)
        dev = _torch_device(ctx)
        d_rhs = None if d is None else _to_device(ctx, d, is_torch, what, "D")
        k = m + probes
        b = torch.empty((n, k), dtype=torch.float64, device=dev)
        if m:
            b[:, :m] = d_rhs.reshape(n, m)
        ctx.probe_fill_into(b.data_ptr() + 8 * m, k, n, probes, seed)
        z = torch.empty((n, k), dtype=torch.float64, device=dev)
        info = solve(h, *q, r, b, k, k, z, k, tol, maxiter, exact=_exact)
        return z, info

    return finish(*with_leases(ctx, _innovation_leased(matrix_h, matrix_q, matrix_r, kron), body))
