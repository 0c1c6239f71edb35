"""Thin object layer over the v2 C ABI (include/smm_hip.h): context, HBM-resident CSR
operands, and the three products.  All arithmetic happens in libsmm_hip.so on the GPU; this
module only moves pointers and sizes (numpy for host buffers, torch tensors -- optional --
for device buffers and streams).
"""
import ctypes
import os
import threading

import numpy as np

from ._lib import (SMM_COV_EXPONENTIAL, SMM_COV_GAUSSIAN, SMM_COV_MATERN32, SMM_COV_MATERN52, SMM_COV_SCALE_BY_PATTERN, SMM_COV_SPHERICAL,
                   SMM_COV_WRT_ALL, SMM_COV_WRT_NONE, SMM_EXACT, SMM_FULL_MATRIX, SMM_INTERP_CLAMP, SMM_INTERP_LINEAR, SMM_INTERP_NEAREST, SMM_INTERP_REJECT, SMM_INTERP_ZERO,
                   SMM_MIRROR, SMM_SCALE_BY_MASK, SMM_SYMMETRIC, SMM_TAPER_BOXCAR, SMM_TAPER_GASPARI_COHN, SMM_TRANSPOSE, SMM_VG_ALL_ENTRIES,
                   SmmError, SmmLibrary, check)

__all__ = ["Context", "DeviceCSR", "default_context", "SmmError",
           "SMM_SYMMETRIC", "SMM_FULL_MATRIX", "SMM_EXACT", "SMM_MIRROR", "SMM_TRANSPOSE", "SMM_SCALE_BY_MASK",
           "SMM_TAPER_BOXCAR", "SMM_TAPER_GASPARI_COHN", "TAPER_KINDS",
           "SMM_INTERP_LINEAR", "SMM_INTERP_NEAREST", "SMM_INTERP_REJECT", "SMM_INTERP_CLAMP", "SMM_INTERP_ZERO", "INTERP_METHODS",
           "INTERP_OUTSIDE", "COV_MODELS"]

TAPER_KINDS = {"boxcar": SMM_TAPER_BOXCAR, "gaspari_cohn": SMM_TAPER_GASPARI_COHN}
COV_MODELS = {"spherical": SMM_COV_SPHERICAL, "exponential": SMM_COV_EXPONENTIAL, "gaussian": SMM_COV_GAUSSIAN,
              "matern32": SMM_COV_MATERN32, "matern52": SMM_COV_MATERN52}
INTERP_METHODS = {"linear": SMM_INTERP_LINEAR, "nearest": SMM_INTERP_NEAREST}
INTERP_OUTSIDE = {"error": SMM_INTERP_REJECT, "clamp": SMM_INTERP_CLAMP, "zero": SMM_INTERP_ZERO}


def _named(value, table, what):
    """The number of a name of `table`, or the number itself."""
    if isinstance(value, str):
        if value not in table:
            raise ValueError(f"unknown {what} {value!r}: expected one of {sorted(table)}")
        return table[value]
    return int(value)


def _taper_kind(kind):
    """SMM_TAPER_* for a name of TAPER_KINDS or the number itself."""
    return _named(kind, TAPER_KINDS, "taper")


def _flags(symmetric=False, exact=False, full=False, mirror=False):
    return ((SMM_SYMMETRIC if symmetric else 0) | (SMM_EXACT if exact else 0) | (SMM_FULL_MATRIX if full else 0) |
            (SMM_MIRROR if mirror else 0))


def _ptr(arr):
    return ctypes.c_void_p(arr.ctypes.data) if arr is not None and arr.size else ctypes.c_void_p(0)


class Context:
    """One GPU + one stream + pooled workspace (smm_ctx).  `stream`: None lets the library create
    (and own) a non-blocking stream; a raw hipStream_t (int) makes it launch there, e.g.
    torch.cuda.current_stream().cuda_stream -- whose value 0 means torch's default stream, i.e.
    the device's null stream (SMM_STREAM_DEFAULT), NOT "create one".  Calls from several host
    threads on one context are safe: the library serialises them on the context's lock."""

    def __init__(self, device=0, stream=None):
        self.lib = SmmLibrary().get_lib()
        h = ctypes.c_void_p()
        if stream is None:
            raw = 0                                   # NULL: the context creates its own stream
        elif int(stream) == 0:
            raw = ctypes.c_void_p(-1).value           # SMM_STREAM_DEFAULT: the null stream
        else:
            raw = int(stream)
        check(self.lib, self.lib.smm_ctx_create(int(device), ctypes.c_void_p(raw), ctypes.byref(h)))
        self.handle = h
        self.device = int(device)
        self.stream = None if stream is None else int(stream)     # None = private stream

    def close(self):
        if getattr(self, "handle", None):
            self.lib.smm_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        check(self.lib, self.lib.smm_ctx_synchronize(self.handle))

    def tune(self, lds_cols=0, waves=0):
        """Geometry of the SMM_EXACT walk (waves 1/2/4/8)."""
        check(self.lib, self.lib.smm_ctx_tune(self.handle, int(lds_cols), int(waves)))

    def tune_shared(self, lds_cols=0, waves=0):
        """Geometry of the default shared-tile walk (waves 4/8/16)."""
        check(self.lib, self.lib.smm_ctx_tune_shared(self.handle, int(lds_cols), int(waves)))

    def tune_hash(self, small_max=256, medium_max=2048):
        """Rows of C with at most small_max / medium_max nonzeros use the LDS-hash kernels
        (0, 0 = dense LDS tiles for every row)."""
        check(self.lib, self.lib.smm_ctx_tune_hash(self.handle, int(small_max), int(medium_max)))

    def tune_slab(self, mode=0, ws=0, rows_per_wave=0):
        """Row-block x column-slab kernels: mode 0 auto / 1 off / 2 force; ws = slab width (0 = L2-sized);
        rows_per_wave 2 or 4."""
        check(self.lib, self.lib.smm_ctx_tune_slab(self.handle, int(mode), int(ws), int(rows_per_wave)))

    def tune_narrow(self, enable=True):
        """uint16 column stream / lists in the symbolic phase for operands with < 65535 columns (default on)."""
        check(self.lib, self.lib.smm_ctx_tune_narrow(self.handle, 1 if enable else 0))

    def tune_symbolic(self, max_slab_cols=0):
        """Widest column slab of the symbolic walk (0 = default 63456); a wider B is walked slab by slab."""
        check(self.lib, self.lib.smm_ctx_tune_symbolic(self.handle, int(max_slab_cols)))

    def tune_dense_runs(self, mode=1):
        """Symbolic walk for operands with dense runs of columns: 0 never, 1 chosen per operand (default), 2 always."""
        check(self.lib, self.lib.smm_ctx_tune_dense_runs(self.handle, int(mode)))

    def tune_stage2(self, ring=False):
        """Triple product, stage 2: the ring kernel of round 4 (True) or the chunk kernel (False, default)."""
        check(self.lib, self.lib.smm_ctx_tune_stage2(self.handle, 1 if ring else 0))

    def tune_pack(self, mode=1):
        """B's packed payload for the CSR product's piece walk: 1 = 1.5-byte columns ("pack12") where smaller (default),
        0 = 16-bit columns always, 2 = pack12 wherever the four-entries-per-lane walk applies."""
        check(self.lib, self.lib.smm_ctx_tune_pack(self.handle, int(mode)))

    def tune_pack_stride(self, mode=1):
        """pack12 pieces at a fixed stride, addressed by row behind a 2-byte length table: 1 = where the strided payload is at
        most 1.5 times the compact one (default), 0 = never, 2 = wherever pack12 is chosen."""
        check(self.lib, self.lib.smm_ctx_tune_pack_stride(self.handle, int(mode)))

    def exact_selftest(self, inject_fault=False):
        """Run the SMM_EXACT guard now (every context runs it by itself before its first exact product):
        raises SmmError (code SMM_ERR_UNSUPPORTED) where the device does not add same-address lanes of one
        ds_add_f64 in ascending lane order.  inject_fault=True exercises that failure path."""
        check(self.lib, self.lib.smm_ctx_exact_selftest(self.handle, 1 if inject_fault else 0))

    def release_pool(self):
        """Return the pooled scratch of destroyed plans / finished calls to the device (smm_ctx_release_pool)."""
        check(self.lib, self.lib.smm_ctx_release_pool(self.handle))

    def pool_bytes(self):
        return int(self.lib.smm_ctx_pool_bytes(self.handle))

    def live_bytes(self):
        """Bytes of pooled scratch handed out: held by open plans and results only (smm_ctx_live_bytes)."""
        return int(self.lib.smm_ctx_live_bytes(self.handle))

    def inject_alloc_failure(self, nth, hard=False):
        """TEST HOOK: the nth device allocation from now fails (first attempt only, or both with hard=True)."""
        check(self.lib, self.lib.smm_ctx_inject_alloc_failure(self.handle, int(nth), 1 if hard else 0))

    def alloc_retries(self):
        return int(self.lib.smm_ctx_alloc_retries(self.handle))

    def set_check(self, enable=True):
        """Run the plan checker at the end of every symbolic phase (also env SMM_CHECK=1): inconsistent plan
        metadata raises SmmError (SMM_ERR_INTERNAL).  The kernels' own bounds clamps are always on."""
        check(self.lib, self.lib.smm_ctx_set_check(self.handle, 1 if enable else 0))

    def timing(self, enable=True):
        check(self.lib, self.lib.smm_ctx_timing(self.handle, 1 if enable else 0))

    def timing_reset(self):
        check(self.lib, self.lib.smm_ctx_timing_reset(self.handle))

    def kernel_time(self, name):
        """(total milliseconds, launches) of the named kernel since the last reset."""
        ms, n = ctypes.c_double(), ctypes.c_int64()
        check(self.lib, self.lib.smm_ctx_kernel_time(self.handle, name.encode(), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    # ------------------------------------------------------------------ operands
    def csr_from_scipy(self, m):
        """Upload a scipy CSR matrix with the reference's casts (matrix_ops.py:196-198)."""
        indptr = np.ascontiguousarray(m.indptr, dtype=np.int32)
        indices = np.ascontiguousarray(m.indices, dtype=np.int32)
        data = np.ascontiguousarray(m.data, dtype=np.float64)
        return self.csr_from_arrays(m.shape[0], m.shape[1], indptr, indices, data)

    def csr_from_arrays(self, rows, cols, indptr, indices, data):
        assert indptr.dtype == np.int32 and indices.dtype == np.int32 and data.dtype == np.float64
        nnz = int(indptr[-1]) if len(indptr) else 0
        h = ctypes.c_void_p()
        check(self.lib, self.lib.smm_csr_from_host(self.handle, rows, cols, nnz, _ptr(indptr), _ptr(indices),
                                                   _ptr(data), ctypes.byref(h)))
        return DeviceCSR(self, h, rows, cols, nnz)

    def csr_from_torch(self, rows, cols, indptr, indices, data):
        """Borrow int32/int32/float64 CUDA tensors already in HBM (kept alive by the handle).  The
        tensors must be complete before the library reads them: when the context does not launch on
        torch's current stream, that stream is synchronised here."""
        self._wait_for_torch(indices.device)
        nnz = int(indices.numel())
        h = ctypes.c_void_p()
        check(self.lib, self.lib.smm_csr_from_device(self.handle, rows, cols, nnz, ctypes.c_void_p(indptr.data_ptr()),
                                                     ctypes.c_void_p(indices.data_ptr()),
                                                     ctypes.c_void_p(data.data_ptr()), ctypes.byref(h)))
        out = DeviceCSR(self, h, rows, cols, nnz)
        out._keep = (indptr, indices, data)
        return out

    def row_products(self, a, b):
        out = np.zeros(a.rows, dtype=np.int64)
        check(self.lib, self.lib.smm_row_products(self.handle, a.handle, b.handle, _ptr(out)))
        return out

    # ------------------------------------------------------------------ CSR x CSR -> CSR
    def spgemm_plan(self, a, b, symmetric=False, row_offset=0, exact=False):
        flags = _flags(symmetric, exact)
        plan, nnz = ctypes.c_void_p(), ctypes.c_int64()
        check(self.lib, self.lib.smm_spgemm_symbolic(self.handle, a.handle, b.handle, flags, int(row_offset),
                                                     ctypes.byref(plan), ctypes.byref(nnz)))
        return Plan(self, plan, a, b, nnz.value)

    def spgemm_host(self, a, b, symmetric=False, row_offset=0, exact=False, index_dtype=None):
        """(indptr int64, indices int32 -- int64 when nnz >= 2^31 or index_dtype says so --, data float64)
        numpy arrays, reference (first-touch) order."""
        plan = self.spgemm_plan(a, b, symmetric, row_offset, exact)
        try:
            # nnz >= 2^31 (BASELINE configs[1]: 2.48e9): int64 column indices, like the row pointer -- scipy's
            # kernels take ONE index dtype per matrix; below that int32, as the reference returns
            return plan.numeric_host(index_dtype)
        finally:
            plan.close()

    def spgemm_torch(self, a, b, symmetric=False, row_offset=0, exact=False):
        """Same product with the result left in HBM as torch tensors (indptr int64); stream rule: _wait_for_torch."""
        import torch
        plan = self.spgemm_plan(a, b, symmetric, row_offset, exact)
        try:
            dev = torch.device("cuda", self.device)
            indptr = torch.empty(a.rows + 1, dtype=torch.int64, device=dev)
            indices = torch.empty(plan.nnz, dtype=torch.int32, device=dev)
            data = torch.empty(plan.nnz, dtype=torch.float64, device=dev)
            self._wait_for_torch(dev)                 # (the allocator may hand out a block torch's stream still uses)
            plan.numeric_into(indptr.data_ptr(), indices.data_ptr(), data.data_ptr())
            self._finish_for_torch(dev)
        finally:
            plan.close()
        return indptr, indices, data

    def spgemm_mirrored_torch(self, a, b, exact=False):
        """spgemm_host_mirrored with the full symmetric CSR left in HBM: (indptr int64, indices int32, data float64)
        torch tensors; stream rule: _wait_for_torch, before each of the two halves writes into torch's memory."""
        import torch
        if a.rows != b.cols:
            raise ValueError("For symmetric output, the resulting matrix must be square.")
        n = a.rows
        dev = torch.device("cuda", self.device)
        plan = self.spgemm_plan(a, b, symmetric=True, exact=exact)

        def empty():
            # the mirror of an upper triangle without entries is the empty n x n matrix; smm_csr_mirror_fill wants arrays
            # that exist (include/smm_hip.h), and a torch tensor of no elements has none
            return (torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                    torch.empty(0, dtype=torch.float64, device=dev))

        try:
            if plan.nnz == 0:
                return empty()
            up = torch.empty(n + 1, dtype=torch.int64, device=dev)
            ui = torch.empty(plan.nnz, dtype=torch.int32, device=dev)
            uv = torch.empty(plan.nnz, dtype=torch.float64, device=dev)
            fp = torch.empty(n + 1, dtype=torch.int64, device=dev)
            self._wait_for_torch(dev)
            plan.numeric_into(up.data_ptr(), ui.data_ptr(), uv.data_ptr())
        finally:
            plan.close()
        nnz = ctypes.c_int64()
        vp = ctypes.c_void_p
        check(self.lib, self.lib.smm_csr_mirror_symbolic(self.handle, n, vp(up.data_ptr()), vp(ui.data_ptr()), vp(fp.data_ptr()), ctypes.byref(nnz)))
        if nnz.value == 0:
            return empty()
        fi = torch.empty(nnz.value, dtype=torch.int32, device=dev)
        fv = torch.empty(nnz.value, dtype=torch.float64, device=dev)
        self._wait_for_torch(dev)
        check(self.lib, self.lib.smm_csr_mirror_fill(self.handle, n, vp(up.data_ptr()), vp(ui.data_ptr()), vp(uv.data_ptr()), vp(fp.data_ptr()),
                                                     vp(fi.data_ptr()), vp(fv.data_ptr())))
        self._finish_for_torch(dev)
        return fp, fi, fv

    def _dmalloc(self, nbytes):
        p = ctypes.c_void_p()
        check(self.lib, self.lib.smm_device_malloc(self.handle, int(nbytes), ctypes.byref(p)))
        return p

    def spgemm_host_mirrored(self, a, b, exact=False):
        """The symmetric product's upper triangle (symmetric=True), mirrored on the device to the full symmetric
        CSR (smm_csr_mirror_*).  Row i: mirrored entries (columns < i) in ascending column order, then the row's
        own entries in first-touch order; any row length (long segments are placed by rank on the device).
        (indptr int64, indices int32 -- int64 when nnz >= 2^31 --, data float64) numpy arrays."""
        if a.rows != b.cols:
            raise ValueError("For symmetric output, the resulting matrix must be square.")
        n = a.rows
        plan = self.spgemm_plan(a, b, symmetric=True, exact=exact)
        bufs = []
        try:
            up, ui, uv = (self._dmalloc(8 * (n + 1)), self._dmalloc(4 * max(plan.nnz, 1)), self._dmalloc(8 * max(plan.nnz, 1)))
            bufs += [up, ui, uv]
            plan.numeric_into(up.value, ui.value, uv.value)
            fp = self._dmalloc(8 * (n + 1)); bufs.append(fp)
            nnz = ctypes.c_int64()
            check(self.lib, self.lib.smm_csr_mirror_symbolic(self.handle, n, up, ui, fp, ctypes.byref(nnz)))
            fi, fv = self._dmalloc(4 * max(nnz.value, 1)), self._dmalloc(8 * max(nnz.value, 1))
            bufs += [fi, fv]
            check(self.lib, self.lib.smm_csr_mirror_fill(self.handle, n, up, ui, uv, fp, fi, fv))
            indptr = np.empty(n + 1, dtype=np.int64)
            indices = np.empty(nnz.value, dtype=np.int32)
            data = np.empty(nnz.value, dtype=np.float64)
            for dst, src in ((indptr, fp), (indices, fi), (data, fv)):
                check(self.lib, self.lib.smm_memcpy_d2h(self.handle, _ptr(dst), src, dst.nbytes))
            if nnz.value > np.iinfo(np.int32).max:            # scipy wants one index dtype per matrix (as spgemm_host)
                indices = indices.astype(np.int64)
            return indptr, indices, data
        finally:
            plan.close()
            for p in bufs:
                self.lib.smm_device_free(self.handle, p)

    # ------------------------------------------------------------------ CSR x CSR -> dense
    def dense_host(self, a, b, symmetric=False, row_offset=0, exact=False, mirror=False):
        flags = _flags(symmetric, exact, mirror=mirror)
        out = np.empty((a.rows, b.cols), dtype=np.float64)
        check(self.lib, self.lib.smm_spgemm_dense_host(self.handle, a.handle, b.handle, flags, int(row_offset),
                                                       _ptr(out)))
        return out

    def dense_into(self, a, b, d_ptr, symmetric=False, row_offset=0, exact=False, mirror=False):
        flags = _flags(symmetric, exact, mirror=mirror)
        check(self.lib, self.lib.smm_spgemm_dense(self.handle, a.handle, b.handle, flags, int(row_offset),
                                                  ctypes.c_void_p(d_ptr)))

    # ------------------------------------------------------------------ H Q H^T
    def triple_host(self, h, q, full=False, row_begin=0, row_end=None, exact=False, mirror=False):
        row_end = h.rows if row_end is None else row_end
        out = np.empty((row_end - row_begin, h.rows), dtype=np.float64)
        check(self.lib, self.lib.smm_triple_product_host(self.handle, h.handle, q.handle, _flags(False, exact, full, mirror),
                                                         int(row_begin), int(row_end), _ptr(out)))
        return out

    def triple_into(self, h, q, d_ptr, full=False, row_begin=0, row_end=None, exact=False, mirror=False):
        row_end = h.rows if row_end is None else row_end
        check(self.lib, self.lib.smm_triple_product(self.handle, h.handle, q.handle, _flags(False, exact, full, mirror),
                                                    int(row_begin), int(row_end), ctypes.c_void_p(d_ptr)))

    # ------------------------------------------------------------------ H Q H^T, sparse output
    def transpose(self, a):
        """A^T built on the device (smm_csr_transpose) as a new DeviceCSR: its arrays are those of scipy's a.tocsc()."""
        h = ctypes.c_void_p()
        check(self.lib, self.lib.smm_csr_transpose(self.handle, a.handle, ctypes.byref(h)))
        return DeviceCSR(self, h, a.cols, a.rows, a.nnz)

    def tune_triple_sparse(self, max_t_nnz=0):
        """Row-block budget of the sparse triple product: entries of T = H[b] * Q per block (0 = default 2^27)."""
        check(self.lib, self.lib.smm_ctx_tune_triple_sparse(self.handle, int(max_t_nnz)))

    def _triple_sparse(self, h, q, full, row_begin, row_end, exact, mask=None):
        row_end = h.rows if row_end is None else row_end
        r = ctypes.c_void_p()
        if isinstance(q, tuple):            # (D, E): Q = D (x) E through its factors, on a mask only
            if mask is None:
                raise ValueError("the sparse triple product with a factor-form Q needs a mask (its pattern would need Q itself)")
            check(self.lib, self.lib.smm_triple_product_sparse_masked_kron(self.handle, h.handle, q[0].handle, q[1].handle,
                                                                           mask.handle, _flags(False, exact, full), int(row_begin),
                                                                           int(row_end), ctypes.byref(r)))
        elif mask is None:
            check(self.lib, self.lib.smm_triple_product_sparse(self.handle, h.handle, q.handle, _flags(False, exact, full),
                                                               int(row_begin), int(row_end), ctypes.byref(r)))
        else:
            check(self.lib, self.lib.smm_triple_product_sparse_masked(self.handle, h.handle, q.handle, mask.handle,
                                                                      _flags(False, exact, full), int(row_begin), int(row_end),
                                                                      ctypes.byref(r)))
        return r, row_end - row_begin, int(self.lib.smm_result_nnz(r))

    def triple_sparse_host(self, h, q, full=False, row_begin=0, row_end=None, exact=False, index_dtype=None, mask=None):
        """Rows [row_begin, row_end) of S = H Q H^T as CSR (smm_triple_product_sparse): columns k >= i in ascending
        order (full=True: the whole symmetric matrix).  (indptr int64, indices int32 -- int64 when nnz >= 2^31 or
        index_dtype says so --, data float64) numpy arrays.  mask (a canonical n x n DeviceCSR): S on the positions of
        the mask with k >= i only (smm_triple_product_sparse_masked).  q may be a pair (D, E) of canonical square DeviceCSR
        factors, Q = D (x) E never formed (smm_triple_product_sparse_masked_kron): then a mask is required."""
        r, rows, nnz = self._triple_sparse(h, q, full, row_begin, row_end, exact, mask)
        try:
            wide = nnz > np.iinfo(np.int32).max if index_dtype is None else np.dtype(index_dtype) == np.int64
            indptr = np.empty(rows + 1, dtype=np.int64)
            indices = np.empty(nnz, dtype=np.int64 if wide else np.int32)
            data = np.empty(nnz, dtype=np.float64)
            check(self.lib, self.lib.smm_result_download(self.handle, r, _ptr(indptr), _ptr(indices), 8 if wide else 4, _ptr(data)))
            return indptr, indices, data
        finally:
            self.lib.smm_result_destroy(r)

    def triple_sparse_torch(self, h, q, full=False, row_begin=0, row_end=None, exact=False, mask=None):
        """triple_sparse_host with the result left in HBM: (indptr int64, indices int32, data float64) torch tensors;
        stream rule: _wait_for_torch."""
        import torch
        r, rows, nnz = self._triple_sparse(h, q, full, row_begin, row_end, exact, mask)
        try:
            dev = torch.device("cuda", self.device)
            indptr = torch.empty(rows + 1, dtype=torch.int64, device=dev)
            indices = torch.empty(nnz, dtype=torch.int32, device=dev)
            data = torch.empty(nnz, dtype=torch.float64, device=dev)
            self._wait_for_torch(dev)
            check(self.lib, self.lib.smm_result_copy_device(self.handle, r, ctypes.c_void_p(indptr.data_ptr()),
                                                            ctypes.c_void_p(indices.data_ptr()), ctypes.c_void_p(data.data_ptr())))
            self._finish_for_torch(dev)
            return indptr, indices, data
        finally:
            self.lib.smm_result_destroy(r)

    # ------------------------------------------------------------------ A B on a given pattern
    def tune_masked(self, mode=0):
        """Path of the masked SpGEMM: 0 per-row cost model (default), 1 dot path, 2 row path (A that is not canonical
        always takes the row path)."""
        check(self.lib, self.lib.smm_ctx_tune_masked(self.handle, int(mode)))

    def spgemm_masked_host(self, a, b, mask, exact=False):
        """Values of A B at the positions of mask (a canonical DeviceCSR, values ignored), in the mask's order: a
        float64 numpy array of nnz(mask) (smm_spgemm_masked_host).  Positions no product reaches hold +0.0."""
        out = np.empty(mask.nnz, dtype=np.float64)
        check(self.lib, self.lib.smm_spgemm_masked_host(self.handle, a.handle, b.handle, mask.handle, _flags(False, exact),
                                                        _ptr(out)))
        return out

    def spgemm_masked_into(self, a, b, mask, d_ptr, exact=False):
        """spgemm_masked_host into caller-owned HBM (nnz(mask) float64 at d_ptr)."""
        check(self.lib, self.lib.smm_spgemm_masked(self.handle, a.handle, b.handle, mask.handle, _flags(False, exact),
                                                   ctypes.c_void_p(d_ptr or 0)))

    def spgemm_masked_kron_host(self, a, d, e, mask, exact=False):
        """spgemm_masked_host with B = D (x) E given by its canonical factors and never formed: the values of A (D (x) E) at
        the positions of mask (a.rows x d.cols * e.cols), in the mask's order (smm_spgemm_masked_kron_host)."""
        out = np.empty(mask.nnz, dtype=np.float64)
        check(self.lib, self.lib.smm_spgemm_masked_kron_host(self.handle, a.handle, d.handle, e.handle, mask.handle,
                                                             _flags(False, exact), _ptr(out)))
        return out

    def spgemm_masked_kron_into(self, a, d, e, mask, d_ptr, exact=False):
        """spgemm_masked_kron_host into caller-owned HBM (nnz(mask) float64 at d_ptr); stream rule as spgemm_masked_into."""
        check(self.lib, self.lib.smm_spgemm_masked_kron(self.handle, a.handle, d.handle, e.handle, mask.handle,
                                                        _flags(False, exact), ctypes.c_void_p(d_ptr or 0)))

    # ------------------------------------------------------------------ sparse x dense
    def tune_spmm(self, mode=0, apply_budget_bytes=0):
        """Kernel classes of the sparse x dense product (0 rows binned by length, 1 / 2 / 3 every row in the tiny / group /
        long class) and the bytes of triple_apply's two intermediates per column block (0 = default, 1 GiB)."""
        check(self.lib, self.lib.smm_ctx_tune_spmm(self.handle, int(mode), int(apply_budget_bytes)))

    # The stream rule, for every torch tensor the library reads, writes or returns.  Shared stream (the context launches on
    # torch's current stream): nothing to do, stream order holds and the host does not wait.  Different streams: torch's
    # current stream is drained before the library reads torch's memory or writes into it (_wait_for_torch), and the
    # context is synchronised before a torch tensor goes back to the caller (_finish_for_torch).
    def _torch_stream_apart(self, device=None):
        """Torch's current stream on the device, or None when the context launches on that very stream."""
        import torch
        cur = torch.cuda.current_stream(torch.device("cuda", self.device) if device is None else device)
        return cur if self.stream is None or int(cur.cuda_stream) != self.stream else None

    def _wait_for_torch(self, device=None):
        cur = self._torch_stream_apart(device)
        if cur is not None:
            cur.synchronize()

    def _finish_for_torch(self, device=None):
        if self._torch_stream_apart(device) is not None:
            self.synchronize()

    def _sync_all(self, *tensors):
        """_wait_for_torch for every torch tensor among these; an int is a device address, whose ordering is the
        caller's."""
        for t in tensors:
            if hasattr(t, "data_ptr"):
                self._wait_for_torch(t.device)

    @staticmethod
    def _host_x(x):
        x = np.asarray(x, dtype=np.float64)
        if x.ndim not in (1, 2):
            raise ValueError(f"X must be 1-D or 2-D, got {x.ndim} dimensions")
        x = np.ascontiguousarray(x)
        return x, (1 if x.ndim == 1 else x.shape[1])

    def _host_blocks(self, entry, ops, x, in_rows, out_rows, flags, name, expect, tail=(), fill=np.empty):
        """Host block in, host block of the same kind out, through a _host entry of the library: x (1-D or 2-D, cast to
        C-contiguous float64) must have in_rows rows; a numpy array of out_rows rows and x's number of dimensions."""
        x, k = self._host_x(x)
        if x.shape[0] != in_rows:
            raise ValueError(f"{name} has {x.shape[0]} rows, {expect}")
        y = fill((out_rows,) + x.shape[1:], dtype=np.float64)
        check(self.lib, entry(self.handle, *_handles(ops), flags, k, _ptr(x), k, _ptr(y), k, *tail))
        return y

    def _device_blocks(self, entry, ops, flags, k, d_in, ld_in, d_out, ld_out, tail=()):
        """Device block in, device block out, through an entry of the library.  Ints (device addresses) or torch tensors:
        torch's current stream is synchronised before the library reads, and the context before this returns."""
        self._sync_all(d_in, d_out)
        check(self.lib, entry(self.handle, *_handles(ops), flags, int(k), ctypes.c_void_p(_dptr(d_in)), int(ld_in),
                              ctypes.c_void_p(_dptr(d_out)), int(ld_out), *tail))
        self.synchronize()

    def spmm_host(self, a, x, transpose=False, exact=False):
        """Y = op(A) X with X a numpy array (1-D or 2-D, cast to C-contiguous float64): a numpy array of the same number
        of dimensions (smm_spmm_host).  op(A) = A^T when transpose."""
        m, kx = (a.cols, a.rows) if transpose else (a.rows, a.cols)
        flags = _flags(exact=exact) | (SMM_TRANSPOSE if transpose else 0)
        return self._host_blocks(self.lib.smm_spmm_host, (a,), x, kx, m, flags, "X", f"op(A) has {kx} columns")

    def spmm_into(self, a, d_x, ldx, k, d_y, ldy, transpose=False, exact=False):
        """Y = op(A) X on device buffers: X (op(A).cols x k, leading dimension ldx) at d_x, Y (op(A).rows x k, leading
        dimension ldy) at d_y (smm_spmm).  Ints (device addresses) or torch tensors: torch's current stream is
        synchronised before the library reads, and the context before this returns."""
        flags = _flags(exact=exact) | (SMM_TRANSPOSE if transpose else 0)
        self._device_blocks(self.lib.smm_spmm, (a,), flags, k, d_x, ldx, d_y, ldy)

    def triple_apply_host(self, h, q, x, exact=False):
        """Y = H (Q (H^T X)) with numpy X (n x k or n): the same shape back (smm_triple_apply_host)."""
        return self._host_blocks(self.lib.smm_triple_apply_host, (h, q), x, h.rows, h.rows, _flags(exact=exact), "X", f"H has {h.rows}")

    def triple_apply_into(self, h, q, d_x, ldx, k, d_y, ldy, exact=False):
        """Y = H (Q (H^T X)) on device buffers (n x k, leading dimensions ldx / ldy; smm_triple_apply); stream rules as
        spmm_into."""
        self._device_blocks(self.lib.smm_triple_apply, (h, q), _flags(exact=exact), k, d_x, ldx, d_y, ldy)

    # ------------------------------------------------------------------ (X Y^T) on a pattern
    def tune_sddmm(self, mode=0):
        """Kernel class of the sampled dense product: 0 chosen from nnz(mask) (default), 1 neighbouring lane groups take
        neighbouring entries, 2 every lane group walks a run of consecutive entries.  Results never depend on it."""
        check(self.lib, self.lib.smm_ctx_tune_sddmm(self.handle, int(mode)))

    @staticmethod
    def _host_2d(x, rows, name):
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
        if x.ndim != 2:
            raise ValueError(f"{name} must be 2-D, got {x.ndim} dimensions")
        if x.shape[0] != rows:
            raise ValueError(f"{name} has {x.shape[0]} rows, expected {rows}")
        return x

    def sddmm_host(self, mask, x, y, scale=False, exact=False):
        """X[i,:] . Y[j,:] at every stored entry (i, j) of mask (a DeviceCSR, any legal CSR), times the entry's value with
        scale, in the mask's stored order: a float64 numpy array of nnz(mask) (smm_sddmm_host).  x: m x k, y: n x k numpy
        arrays (cast to C-contiguous float64); y=None means y = x."""
        x = self._host_2d(x, mask.rows, "X")
        y = x if y is None else self._host_2d(y, mask.cols, "Y")
        if y.shape != (mask.cols, x.shape[1]):
            raise ValueError(f"Y is {y.shape[0]} x {y.shape[1]}, expected {mask.cols} x {x.shape[1]}")
        k = x.shape[1]
        out = np.empty(mask.nnz, dtype=np.float64)
        flags = _flags(exact=exact) | (SMM_SCALE_BY_MASK if scale else 0)
        check(self.lib, self.lib.smm_sddmm_host(self.handle, mask.handle, flags, k, _ptr(x), k, _ptr(y), k, _ptr(out)))
        return out

    def sddmm_into(self, mask, d_x, ldx, d_y, ldy, k, d_c, scale=False, exact=False):
        """sddmm_host on device buffers: X (mask.rows x k, leading dimension ldx) at d_x, Y (mask.cols x k, leading
        dimension ldy) at d_y, nnz(mask) float64 written at d_c (smm_sddmm).  Ints (device addresses) or torch tensors;
        stream rules as spmm_into."""
        self._sync_all(d_x, d_y, d_c)
        flags = _flags(exact=exact) | (SMM_SCALE_BY_MASK if scale else 0)
        check(self.lib, self.lib.smm_sddmm(self.handle, mask.handle, flags, int(k), ctypes.c_void_p(_dptr(d_x)), int(ldx),
                                           ctypes.c_void_p(_dptr(d_y)), int(ldy), ctypes.c_void_p(_dptr(d_c))))
        self.synchronize()

    # ------------------------------------------------------------------ localisation taper from coordinates
    @staticmethod
    def _host_points(x, name):
        """(points, dim): a C-contiguous float64 n x dim numpy array; a 1-D array is n points on a line."""
        x = np.asarray(x, dtype=np.float64)
        if x.ndim == 1:
            x = x.reshape(-1, 1)
        if x.ndim != 2:
            raise ValueError(f"{name} must be 1-D or 2-D, got {x.ndim} dimensions")
        return np.ascontiguousarray(x), int(x.shape[1])

    def taper_host(self, a, b, cutoff, kind="gaspari_cohn"):
        """The taper matrix of the numpy points a (na x dim, or na on a line) against b (nb x dim; None means b = a, the
        square symmetric case): entry (i, j) iff |a_i - b_j| < cutoff, boxcar or Gaspari-Cohn weights, rows strictly
        ascending, as a new DeviceCSR (smm_taper_build_host)."""
        kind = _taper_kind(kind)
        a, dim = self._host_points(a, "a")
        if b is None:
            b = a
        else:
            b, dim_b = self._host_points(b, "b")
            if dim_b != dim:
                raise ValueError(f"a has {dim} coordinates per point, b has {dim_b}")
        h = ctypes.c_void_p()
        check(self.lib, self.lib.smm_taper_build_host(self.handle, dim, kind, float(cutoff), a.shape[0], _ptr(a), dim, b.shape[0],
                                                      _ptr(b), dim, ctypes.byref(h)))
        return DeviceCSR(self, h, a.shape[0], b.shape[0], int(self.lib.smm_csr_nnz(h)))

    def taper_into(self, d_a, lda, d_b, ldb, na, nb, dim, cutoff, kind="gaspari_cohn"):
        """taper_host on device buffers: a (na x dim, leading dimension lda) at d_a, b (nb x dim, leading dimension ldb) at
        d_b -- the same buffer for the square case (smm_taper_build).  Ints (device addresses) or torch tensors; stream
        rules as spmm_into.  Returns the DeviceCSR, which the library owns: nothing of the caller's is kept."""
        kind = _taper_kind(kind)
        self._sync_all(d_a, d_b)
        h = ctypes.c_void_p()
        check(self.lib, self.lib.smm_taper_build(self.handle, int(dim), kind, float(cutoff), int(na), ctypes.c_void_p(_dptr(d_a)), int(lda),
                                                 int(nb), ctypes.c_void_p(_dptr(d_b)), int(ldb), ctypes.byref(h)))
        return DeviceCSR(self, h, int(na), int(nb), int(self.lib.smm_csr_nnz(h)))

    # ------------------------------------------------------------------ parametric covariance on a pattern
    @staticmethod
    def _cov_args(model, length, dim, variance, wrt, scale):
        """(flags, model, dim, length, variance, wrt) as smm_cov_eval takes them.  length: a scalar (every coordinate) or dim
        numbers; wrt: None, "length" (the common length) or a coordinate's index.  The library checks the values."""
        length = np.ascontiguousarray(np.broadcast_to(np.asarray(length, dtype=np.float64), (dim,)))
        wrt = SMM_COV_WRT_NONE if wrt is None else (SMM_COV_WRT_ALL if isinstance(wrt, str) and wrt == "length" else int(wrt))
        return [SMM_COV_SCALE_BY_PATTERN if scale else 0, _named(model, COV_MODELS, "model"), int(dim), _ptr(length), float(variance), wrt], length

    def cov_host(self, pattern, a, b, model, length, variance=1.0, wrt=None, scale=False, value=True):
        """variance * c(h) at every stored entry (i, j) of pattern (a DeviceCSR, any legal CSR) from the numpy points a
        (rows x dim, or rows on a line) and b (cols x dim; None means b = a), h the distance in coordinates divided by
        `length`; with wrt also the derivative with respect to that length; times the entry's value with scale
        (smm_cov_eval_host).  Returns (val, dval): float64 numpy arrays of nnz(pattern) in the pattern's stored order, None
        for the one not asked for (value=False: the derivative alone)."""
        a, dim = self._host_points(a, "a")
        if b is None:
            b = a
        else:
            b, dim_b = self._host_points(b, "b")
            if dim_b != dim:
                raise ValueError(f"a has {dim} coordinates per point, b has {dim_b}")
        head, keep = self._cov_args(model, length, dim, variance, wrt, scale)
        # (an output that is asked for has an address, also for a pattern without entries: NULL means "not asked for")
        val = np.empty(max(pattern.nnz, 1), dtype=np.float64)[:pattern.nnz] if value else None
        dval = np.empty(max(pattern.nnz, 1), dtype=np.float64)[:pattern.nnz] if wrt is not None else None
        out = [ctypes.c_void_p(x.ctypes.data) if x is not None else ctypes.c_void_p(0) for x in (val, dval)]
        check(self.lib, self.lib.smm_cov_eval_host(self.handle, pattern.handle, *head, a.shape[0], _ptr(a), dim, b.shape[0], _ptr(b), dim, *out))
        del keep
        return val, dval

    def cov_into(self, pattern, d_a, lda, d_b, ldb, dim, model, length, variance, d_val, d_dval=None, wrt=None, scale=False):
        """cov_host on device buffers: a (pattern.rows x dim, leading dimension lda) at d_a, b (pattern.cols x dim, leading
        dimension ldb) at d_b -- the same buffer for the square case --, nnz(pattern) float64 written at d_val and / or
        d_dval, None for an output not wanted (smm_cov_eval).  Ints (device addresses) or torch tensors; stream rules as
        spmm_into."""
        head, keep = self._cov_args(model, length, dim, variance, wrt, scale)
        self._sync_all(d_a, d_b, d_val, d_dval)
        check(self.lib, self.lib.smm_cov_eval(self.handle, pattern.handle, *head, pattern.rows, ctypes.c_void_p(_dptr(d_a)), int(lda),
                                              pattern.cols, ctypes.c_void_p(_dptr(d_b)), int(ldb), ctypes.c_void_p(_dptr(d_val)),
                                              ctypes.c_void_p(_dptr(d_dval))))
        del keep
        self.synchronize()

    # ------------------------------------------------------------------ empirical variogram on a pattern
    @staticmethod
    def _variogram_bins(edges):
        """(edges float64[nb + 1], nb, count int64, sum_h, sum_sq): the host arrays of smm_variogram.  The outputs have an
        address whatever nb is: the library checks the number of bins and the edges' values."""
        edges = np.ascontiguousarray(np.asarray(edges, dtype=np.float64).reshape(-1))
        nb = int(edges.size) - 1
        size = max(nb, 1)
        return edges, nb, np.zeros(size, dtype=np.int64), np.zeros(size, dtype=np.float64), np.zeros(size, dtype=np.float64)

    def variogram_host(self, pattern, a, y, edges, upper=True):
        """Over the stored entries (i, j) of pattern (a square DeviceCSR, any legal CSR) -- those with j > i, or all of them
        with upper=False --, binned by the distance h of the numpy points a[i] and a[j] (n x dim, or n on a line) into
        [edges[b], edges[b+1]): the number of pairs, the sum of h and the sum over the columns of y (n x k, or n) of
        (y[i] - y[j])^2, summed in the fixed order of include/smm_hip.h (smm_variogram_host).  Returns (count int64, sum_h,
        sum_sq): numpy arrays of len(edges) - 1."""
        a, dim = self._host_points(a, "a")
        y, k = self._host_points(y, "y")
        if y.shape[0] != a.shape[0]:
            raise ValueError(f"a has {a.shape[0]} points, y has {y.shape[0]} rows")
        edges, nb, count, sum_h, sum_sq = self._variogram_bins(edges)
        check(self.lib, self.lib.smm_variogram_host(self.handle, pattern.handle, 0 if upper else SMM_VG_ALL_ENTRIES, dim, _ptr(a), dim, k,
                                                    _ptr(y), k, nb, _ptr(edges), _ptr(count), _ptr(sum_h), _ptr(sum_sq)))
        return count, sum_h, sum_sq                                # (nb >= 1 here: the library refused anything else)

    def variogram_device(self, pattern, d_a, lda, dim, d_y, ldy, k, edges, upper=True):
        """variogram_host on device buffers: a (pattern.rows x dim, leading dimension lda) at d_a and y (pattern.rows x k,
        leading dimension ldy) at d_y (smm_variogram); the edges and the three results stay host arrays.  Ints (device
        addresses) or torch tensors; torch's current stream is synchronised before the library reads, and the call returns
        synchronised."""
        edges, nb, count, sum_h, sum_sq = self._variogram_bins(edges)
        self._sync_all(d_a, d_y)
        check(self.lib, self.lib.smm_variogram(self.handle, pattern.handle, 0 if upper else SMM_VG_ALL_ENTRIES, int(dim),
                                               ctypes.c_void_p(_dptr(d_a)), int(lda), int(k), ctypes.c_void_p(_dptr(d_y)), int(ldy), nb,
                                               _ptr(edges), _ptr(count), _ptr(sum_h), _ptr(sum_sq)))
        return count, sum_h, sum_sq                                # (nb >= 1 here: the library refused anything else)

    # ------------------------------------------------------------------ observation operator from coordinates
    @staticmethod
    def _host_axes(axes, dim):
        """(axis_len int64[dim], nodes float64[sum]) of a sequence of 1-D arrays (one array: a line): the two host arrays of
        smm_interp_build.  Only the shapes are checked here; the library checks the values."""
        if isinstance(axes, np.ndarray) and axes.ndim == 1:
            axes = [axes]
        axes = [np.asarray(a, dtype=np.float64) for a in axes]
        if len(axes) != dim or any(a.ndim != 1 for a in axes):
            raise ValueError(f"the points have {dim} coordinates, axes holds {len(axes)} arrays (each must be 1-D)")
        return np.array([a.size for a in axes], dtype=np.int64), np.ascontiguousarray(np.concatenate(axes) if axes else np.zeros(0))

    def interp_host(self, points, axes, method="linear", outside="error"):
        """The matrix that interpolates a field on the rectilinear grid `axes` (a sequence of 1-D ascending arrays, axis 0
        slowest) to the numpy points (n x dim, or n on a line): 2^dim multilinear weights per row, or one 1.0 at the
        nearest node, rows strictly ascending, as a new DeviceCSR (smm_interp_build_host)."""
        method, outside = _named(method, INTERP_METHODS, "method"), _named(outside, INTERP_OUTSIDE, "policy")
        p, dim = self._host_points(points, "points")
        lens, nodes = self._host_axes(axes, dim)
        h = ctypes.c_void_p()
        check(self.lib, self.lib.smm_interp_build_host(self.handle, dim, _ptr(lens), _ptr(nodes), method, outside, p.shape[0], _ptr(p), dim,
                                                       ctypes.byref(h)))
        return DeviceCSR(self, h, p.shape[0], int(self.lib.smm_csr_cols(h)), int(self.lib.smm_csr_nnz(h)))

    def interp_into(self, d_pts, ldp, n, dim, axes, method="linear", outside="error"):
        """interp_host on a device buffer: the points (n x dim, leading dimension ldp) at d_pts, used where they are
        (smm_interp_build); the axes stay host arrays.  An int (device address) or a torch tensor; stream rules as
        spmm_into.  Returns the DeviceCSR, which the library owns: nothing of the caller's is kept."""
        method, outside = _named(method, INTERP_METHODS, "method"), _named(outside, INTERP_OUTSIDE, "policy")
        lens, nodes = self._host_axes(axes, int(dim))
        self._sync_all(d_pts)
        h = ctypes.c_void_p()
        check(self.lib, self.lib.smm_interp_build(self.handle, int(dim), _ptr(lens), _ptr(nodes), method, outside, int(n),
                                                  ctypes.c_void_p(_dptr(d_pts)), int(ldp), ctypes.byref(h)))
        return DeviceCSR(self, h, int(n), int(self.lib.smm_csr_cols(h)), int(self.lib.smm_csr_nnz(h)))

    # ------------------------------------------------------------------ Kronecker operand Q = D (x) E
    def kron_build(self, d, e):
        """D (x) E as a new DeviceCSR the library owns (smm_kron_build): row t * e.rows + j holds D.val[a] * E.val[b] at
        column D.idx[a] * e.cols + E.idx[b], a over row t of D and b over row j of E in stored order."""
        h = ctypes.c_void_p()
        check(self.lib, self.lib.smm_kron_build(self.handle, d.handle, e.handle, ctypes.byref(h)))
        return DeviceCSR(self, h, d.rows * e.rows, d.cols * e.cols, int(self.lib.smm_csr_nnz(h)))

    def kron_apply_host(self, d, e, x, exact=False):
        """Y = (D (x) E) X without forming it, X a numpy array (1-D or 2-D, cast to C-contiguous float64): a numpy array of
        the same number of dimensions (smm_kron_apply_host)."""
        m, kx = d.rows * e.rows, d.cols * e.cols
        return self._host_blocks(self.lib.smm_kron_apply_host, (d, e), x, kx, m, _flags(exact=exact), "X", f"D (x) E has {kx} columns")

    def kron_apply_into(self, d, e, d_x, ldx, k, d_y, ldy, exact=False):
        """Y = (D (x) E) X on device buffers (smm_kron_apply): X ((d.cols * e.cols) x k, leading dimension ldx) at d_x, Y
        ((d.rows * e.rows) x k, leading dimension ldy) at d_y; stream rules as spmm_into."""
        self._device_blocks(self.lib.smm_kron_apply, (d, e), _flags(exact=exact), k, d_x, ldx, d_y, ldy)

    def triple_apply_kron_host(self, h, d, e, x, exact=False):
        """Y = H ((D (x) E) (H^T X)) with numpy X (n x k or n): the same shape back (smm_triple_apply_kron_host)."""
        return self._host_blocks(self.lib.smm_triple_apply_kron_host, (h, d, e), x, h.rows, h.rows, _flags(exact=exact), "X",
                                 f"H has {h.rows}")

    def triple_apply_kron_into(self, h, d, e, d_x, ldx, k, d_y, ldy, exact=False):
        """triple_apply_kron_host on device buffers (smm_triple_apply_kron); stream rules as spmm_into."""
        self._device_blocks(self.lib.smm_triple_apply_kron, (h, d, e), _flags(exact=exact), k, d_x, ldx, d_y, ldy)

    # ------------------------------------------------------------------ CG on (H Q H^T + R) Z = D
    def _solve_host(self, entry, ops, r, d, tol, maxiter, exact):
        """A solve entry on the numpy right-hand sides d (n x k or n), ops = (H, Q) or (H, D, E): (Z, info)."""
        n = ops[0].rows
        info = SolveInfo(self._host_x(d)[1])
        z = self._host_blocks(entry, (*ops, r), d, n, n, _flags(exact=exact), "D", f"H has {n}",
                              info.tail(tol, n if maxiter is None else maxiter), np.zeros)
        return z, info

    def _solve(self, entry, ops, r, d_b, ldb, k, d_x, ldx, tol, maxiter, exact, history=None):
        """A solve entry on device buffers, ops = (H, Q) or (H, D, E); stream rules as spmm_into.  Returns info, with the
        coefficient histories (history rows each) where the entry records them."""
        info = SolveInfo(k, history)
        self._device_blocks(entry, (*ops, r), _flags(exact=exact), k, d_b, ldb, d_x, ldx, info.tail(tol, maxiter))
        return info

    def innovation_solve_host(self, h, q, r, d, tol=1e-8, maxiter=None, exact=False):
        """(Z, info) with (H Q H^T + R) Z = D by conjugate gradients, one CG per column of the numpy D (n x k or n), Z of
        the same shape (smm_innovation_solve_host).  r: a DeviceCSR (n x n) or None; maxiter None means n."""
        return self._solve_host(self.lib.smm_innovation_solve_host, (h, q), r, d, tol, maxiter, exact)

    def innovation_solve_into(self, h, q, r, d_b, ldb, k, d_x, ldx, tol=1e-8, maxiter=None, exact=False):
        """The same on device buffers: D (n x k, leading dimension ldb) at d_b, Z (leading dimension ldx) at d_x
        (smm_innovation_solve); stream rules as spmm_into.  Returns info."""
        return self._solve(self.lib.smm_innovation_solve, (h, q), r, d_b, ldb, k, d_x, ldx, tol, h.rows if maxiter is None else maxiter, exact)

    def innovation_solve_kron_host(self, h, d, e, r, rhs, tol=1e-8, maxiter=None, exact=False):
        """innovation_solve_host with Q = D (x) E applied through its factors (smm_innovation_solve_kron_host): (Z, info)."""
        return self._solve_host(self.lib.smm_innovation_solve_kron_host, (h, d, e), r, rhs, tol, maxiter, exact)

    def innovation_solve_kron_into(self, h, d, e, r, d_b, ldb, k, d_x, ldx, tol=1e-8, maxiter=None, exact=False):
        """The same on device buffers (smm_innovation_solve_kron); stream rules as spmm_into.  Returns info."""
        return self._solve(self.lib.smm_innovation_solve_kron, (h, d, e), r, d_b, ldb, k, d_x, ldx, tol,
                           h.rows if maxiter is None else maxiter, exact)

    # ------------------------------------------------------------------ log det(H Q H^T + R): probes, recorded coefficients
    def probe_fill_into(self, d_x, ldx, n, k, seed=0):
        """X[i, c] = +-1.0 by the hash of include/smm_hip.h (seed taken modulo 2^64) into the n x k block at d_x, leading
        dimension ldx (smm_probe_fill); padding is not written.  An int (device address) or a torch tensor; stream rules
        as spmm_into."""
        self._sync_all(d_x)
        check(self.lib, self.lib.smm_probe_fill(self.handle, int(n), int(k), int(seed) % (1 << 64), ctypes.c_void_p(_dptr(d_x)), int(ldx)))
        self.synchronize()

    def _solve_coef(self, entry, ops, r, d_b, ldb, k, d_x, ldx, tol, maxiter, exact):
        # (a maxiter the library refuses gets no history to size: it is refused there, before anything is written)
        return self._solve(entry, ops, r, d_b, ldb, k, d_x, ldx, tol, maxiter, exact, history=int(maxiter) if 1 <= int(maxiter) <= 65536 else 0)

    def innovation_solve_coef_into(self, h, q, r, d_b, ldb, k, d_x, ldx, tol=1e-8, maxiter=1000, exact=False):
        """innovation_solve_into that keeps every column's CG coefficients (smm_innovation_solve_coef): info.alpha and
        info.beta are maxiter x k, row it - 1 holding iteration it, +0.0 where a column computed none.  maxiter must be
        given as 1 .. 65536: it sizes the histories."""
        return self._solve_coef(self.lib.smm_innovation_solve_coef, (h, q), r, d_b, ldb, k, d_x, ldx, tol, maxiter, exact)

    def innovation_solve_coef_kron_into(self, h, d, e, r, d_b, ldb, k, d_x, ldx, tol=1e-8, maxiter=1000, exact=False):
        """The same with Q = D (x) E applied through its factors (smm_innovation_solve_coef_kron)."""
        return self._solve_coef(self.lib.smm_innovation_solve_coef_kron, (h, d, e), r, d_b, ldb, k, d_x, ldx, tol, maxiter, exact)


class SolveInfo:
    """Per-column outcome of innovation_solve: iterations (int32), status (int32: 0 converged, 1 iteration limit,
    2 breakdown), residual_sq (the recurrence's dot(r, r) at the end) and rhs_sq (dot(d, d)), numpy arrays of k entries.
    alpha and beta: None, or -- from the calls that record them -- the maxiter x k CG coefficients (row it - 1, column j)."""
    CONVERGED, ITERATION_LIMIT, BREAKDOWN = 0, 1, 2

    def __init__(self, k, history=None):
        self.iterations = np.zeros(k, dtype=np.int32)
        self.status = np.zeros(k, dtype=np.int32)
        self.residual_sq = np.zeros(k, dtype=np.float64)
        self.rhs_sq = np.zeros(k, dtype=np.float64)
        self.alpha = self.beta = None
        if history is not None:
            self.alpha, self.beta = np.zeros((history, k), dtype=np.float64), np.zeros((history, k), dtype=np.float64)

    def tail(self, tol, maxiter):
        """What a solve entry takes behind its blocks: tol, maxiter, the per-column outputs and, where kept, the histories."""
        out = (self.iterations, self.status, self.residual_sq, self.rhs_sq) + (() if self.alpha is None else (self.alpha, self.beta))
        return [float(tol), int(maxiter)] + [_ptr(a) for a in out]

    @property
    def converged(self):
        return bool(np.all(self.status == 0))

    def __repr__(self):
        return (f"SolveInfo(iterations={self.iterations.tolist()}, status={self.status.tolist()}, "
                f"residual_sq={self.residual_sq.tolist()}, rhs_sq={self.rhs_sq.tolist()})")


def _handles(ops):
    """The library's handles of these operands (None: an operand the call leaves out)."""
    return [o.handle if o is not None else None for o in ops]


def _dptr(p):
    """A device address: an int, or a torch tensor's data_ptr()."""
    if p is None:
        return 0
    return int(p.data_ptr()) if hasattr(p, "data_ptr") else int(p)


class DeviceCSR:
    def __init__(self, ctx, handle, rows, cols, nnz):
        self.ctx, self.handle, self.rows, self.cols, self.nnz = ctx, handle, int(rows), int(cols), int(nnz)
        self._keep = None

    def is_canonical(self):
        return bool(self.ctx.lib.smm_csr_is_canonical(self.ctx.handle, self.handle))

    def update_values(self, data):
        """New values on the same sparsity pattern (host array of nnz float64): the operand and every cached
        copy are rewritten in place, plans made on it stay valid (smm_csr_update_values)."""
        data = np.ascontiguousarray(data, dtype=np.float64)
        if data.size != self.nnz:
            raise ValueError(f"update_values: {data.size} values for an operand with {self.nnz} nonzeros")
        check(self.ctx.lib, self.ctx.lib.smm_csr_update_values(self.ctx.handle, self.handle, _ptr(data)))

    def values_changed(self, d_ptr=None):
        """The values in HBM were rewritten by the caller (borrowed operands: csr_from_torch), or are at device
        pointer d_ptr (copied over the operand's own array): refresh the cached copies.  A borrowed operand's tensors were
        rewritten on torch's current stream: the stream rule (Context._wait_for_torch) holds for them; a d_ptr's ordering
        is the caller's."""
        if self._keep is not None:
            self.ctx._wait_for_torch(self._keep[2].device)
        check(self.ctx.lib, self.ctx.lib.smm_csr_update_values_device(self.ctx.handle, self.handle,
                                                                      ctypes.c_void_p(d_ptr or 0)))

    def to_host(self):
        """The operand's own arrays copied back: (indptr int32, indices int32, data float64) numpy arrays."""
        indptr = np.empty(self.rows + 1, dtype=np.int32)
        indices = np.empty(self.nnz, dtype=np.int32)
        data = np.empty(self.nnz, dtype=np.float64)
        check(self.ctx.lib, self.ctx.lib.smm_csr_download(self.ctx.handle, self.handle, _ptr(indptr), _ptr(indices), _ptr(data)))
        return indptr, indices, data

    def pattern_torch(self):
        """The operand's row pointer and columns copied into new int32 CUDA tensors (device to device,
        smm_csr_copy_device): (indptr, indices)."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        indptr = torch.empty(self.rows + 1, dtype=torch.int32, device=dev)
        indices = torch.empty(self.nnz, dtype=torch.int32, device=dev)
        self.ctx._wait_for_torch(dev)                                # (smm_csr_copy_device synchronises the context itself)
        check(self.ctx.lib, self.ctx.lib.smm_csr_copy_device(self.ctx.handle, self.handle, ctypes.c_void_p(indptr.data_ptr()),
                                                             ctypes.c_void_p(indices.data_ptr()), None))
        return indptr, indices

    def values_into(self, d_data):
        """The operand's values copied into a float64 CUDA tensor (or device address) of nnz entries, device to device
        (smm_csr_copy_device).  A tensor follows the stream rule (Context._wait_for_torch); an address's ordering is the
        caller's."""
        self.ctx._sync_all(d_data)
        check(self.ctx.lib, self.ctx.lib.smm_csr_copy_device(self.ctx.handle, self.handle, None, None, ctypes.c_void_p(_dptr(d_data))))
        if hasattr(d_data, "data_ptr"):
            self.ctx._finish_for_torch(d_data.device)

    def device_bytes(self):
        return int(self.ctx.lib.smm_csr_device_bytes(self.handle)) if self.handle else 0

    def close(self):
        if getattr(self, "handle", None) and getattr(self.ctx, "handle", None):
            self.ctx.lib.smm_csr_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Plan:
    """Symbolic phase of one product (smm_plan): nnz and row pointer are known, the numeric
    phase fills caller-owned buffers."""

    def __init__(self, ctx, handle, a, b, nnz):
        self.ctx, self.handle, self.a, self.b, self.nnz = ctx, handle, a, b, int(nnz)

    def indptr_host(self):
        out = np.empty(self.a.rows + 1, dtype=np.int64)
        check(self.ctx.lib, self.ctx.lib.smm_plan_indptr_host(self.ctx.handle, self.handle, _ptr(out)))
        return out

    def device_bytes(self):
        return int(self.ctx.lib.smm_plan_device_bytes(self.handle)) if self.handle else 0

    def check(self):
        """Verify the plan's metadata on the device (smm_plan_check); raises SmmError (SMM_ERR_INTERNAL)."""
        check(self.ctx.lib, self.ctx.lib.smm_plan_check(self.ctx.handle, self.handle))

    def inject_fault(self, kind):
        """TEST HOOK: damage one piece of the plan's metadata (smm_plan_inject_fault)."""
        check(self.ctx.lib, self.ctx.lib.smm_plan_inject_fault(self.ctx.handle, self.handle, int(kind)))

    def numeric_host(self, index_dtype=None):
        """Run the numeric phase of this plan (again, after update_values on its operands if wanted) and return
        (indptr int64, indices, data) as numpy arrays."""
        ctx = self.ctx
        wide = self.nnz > np.iinfo(np.int32).max if index_dtype is None else np.dtype(index_dtype) == np.int64
        indptr = np.empty(self.a.rows + 1, dtype=np.int64)
        indices = np.empty(self.nnz, dtype=np.int64 if wide else np.int32)
        data = np.empty(self.nnz, dtype=np.float64)
        fn = ctx.lib.smm_spgemm_numeric_host_i64 if wide else ctx.lib.smm_spgemm_numeric_host
        check(ctx.lib, fn(ctx.handle, self.handle, _ptr(indptr), _ptr(indices), _ptr(data)))
        return indptr, indices, data

    def numeric_into(self, d_indptr, d_indices, d_data):
        check(self.ctx.lib, self.ctx.lib.smm_spgemm_numeric(self.ctx.handle, self.handle, ctypes.c_void_p(d_indptr),
                                                            ctypes.c_void_p(d_indices), ctypes.c_void_p(d_data)))

    def close(self):
        if getattr(self, "handle", None) and getattr(self.ctx, "handle", None):
            self.ctx.lib.smm_plan_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default = None
_default_lock = threading.Lock()


def default_context():
    """Process-wide context on the device of this rank (LOCAL_RANK, else SMM_DEVICE, else 0)."""
    global _default
    with _default_lock:
        if _default is None:
            dev = int(os.environ.get("SMM_DEVICE", os.environ.get("LOCAL_RANK", "0")))
            _default = Context(dev)
        return _default
