"""ctypes loader of lib/libsmm_hip.so -- the only native code this package uses.

Mirrors MatrixOpsLibrary of the reference (sparse_matrix_mult/matrix_ops.py:51-184): a
process-wide singleton that loads the shared library once and declares the prototypes.
Unlike the reference it is silent at import (SURVEY F9 / section 8b "Side effects") and it
refuses to run without the HIP library: there is no CPU fallback in this package.
"""
import ctypes
import importlib.util
import os
import re
import subprocess
import sys
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# SMM_LIB_PATH: load another build of the same library (diagnostic builds, e.g. -DSMM_STAMPS)
LIB_PATH = os.environ.get("SMM_LIB_PATH") or os.path.join(_HERE, "lib", "libsmm_hip.so")

SMM_SYMMETRIC = 1
SMM_FULL_MATRIX = 2
SMM_EXACT = 4
SMM_MIRROR = 8
SMM_TRANSPOSE = 16
SMM_SCALE_BY_MASK = 32
SMM_TAPER_BOXCAR = 0
SMM_TAPER_GASPARI_COHN = 1
SMM_COV_SPHERICAL = 0
SMM_COV_EXPONENTIAL = 1
SMM_COV_GAUSSIAN = 2
SMM_COV_MATERN32 = 3
SMM_COV_MATERN52 = 4
SMM_COV_WRT_NONE = -1
SMM_COV_WRT_ALL = 3
SMM_COV_SCALE_BY_PATTERN = 32
SMM_INTERP_LINEAR = 0
SMM_INTERP_NEAREST = 1
SMM_INTERP_REJECT = 0
SMM_INTERP_CLAMP = 1
SMM_INTERP_ZERO = 2


def _header_constants(prefix):
    """name -> value of the `NAME = integer` enumerators of include/smm_hip.h whose name starts with prefix: constants of a
    contract that the header alone states (the tree of smm_variogram), read and never restated here."""
    with open(os.path.join(os.path.dirname(_HERE), "include", "smm_hip.h")) as f:
        return {name: int(value) for name, value in re.findall(r"\b(%s\w+) = (-?\d+)\b" % prefix, f.read())}


_VG = _header_constants("SMM_VG_")
SMM_VG_RUN, SMM_VG_SLOTS, SMM_VG_MAX_BINS = _VG["SMM_VG_RUN"], _VG["SMM_VG_SLOTS"], _VG["SMM_VG_MAX_BINS"]
SMM_VG_ALL_ENTRIES = _VG["SMM_VG_ALL_ENTRIES"]
SMM_ERR_INVALID = -2
SMM_ERR_ALLOC = -3
SMM_ERR_OVERFLOW = -5
SMM_ERR_UNSUPPORTED = -6
SMM_ERR_INTERNAL = -7

_c_i64 = ctypes.c_int64
_vp = ctypes.c_void_p
_pp = ctypes.POINTER(ctypes.c_void_p)
# the argument tails of the entries that take one row-major block in and give one out, behind the context and the operands
_BLOCKS = [ctypes.c_int, _c_i64, _vp, _c_i64, _vp, _c_i64]                  # flags, k, in, ld_in, out, ld_out
_SOLVE = _BLOCKS + [ctypes.c_double, _c_i64, _vp, _vp, _vp, _vp]            # tol, maxiter, the four per-column outputs
# smm_cov_eval[_host] behind the context and the pattern: flags, model, dim, length, variance, wrt, na, a, lda, nb, b, ldb, val, dval
_COV = [ctypes.c_int] * 3 + [_vp, ctypes.c_double, ctypes.c_int, _c_i64, _vp, _c_i64, _c_i64, _vp, _c_i64, _vp, _vp]
# smm_variogram[_host] behind the context and the pattern: flags, dim, a, lda, k, y, ldy, nb, edges, count, sum_h, sum_sq
_VARIOGRAM = [ctypes.c_int] * 2 + [_vp, _c_i64, _c_i64, _vp, _c_i64, ctypes.c_int, _vp, _vp, _vp, _vp]

# name -> (restype, argtypes); every v2 symbol declared in include/smm_hip.h
V2_PROTOTYPES = {
    "smm_device_count": (ctypes.c_int, []),
    "smm_last_error": (ctypes.c_char_p, []),
    "smm_ctx_create": (ctypes.c_int, [ctypes.c_int, _vp, _pp]),
    "smm_ctx_destroy": (None, [_vp]),
    "smm_ctx_synchronize": (ctypes.c_int, [_vp]),
    "smm_ctx_timing": (ctypes.c_int, [_vp, ctypes.c_int]),
    "smm_ctx_timing_reset": (ctypes.c_int, [_vp]),
    "smm_ctx_kernel_time": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double),
                                           ctypes.POINTER(_c_i64)]),
    "smm_ctx_tune": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "smm_ctx_tune_shared": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "smm_ctx_tune_hash": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "smm_ctx_tune_slab": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "smm_ctx_tune_narrow": (ctypes.c_int, [_vp, ctypes.c_int]),
    "smm_ctx_exact_selftest": (ctypes.c_int, [_vp, ctypes.c_int]),
    "smm_ctx_tune_symbolic": (ctypes.c_int, [_vp, ctypes.c_int]),
    "smm_ctx_tune_dense_runs": (ctypes.c_int, [_vp, ctypes.c_int]),
    "smm_ctx_tune_stage2": (ctypes.c_int, [_vp, ctypes.c_int]),
    "smm_ctx_tune_pack": (ctypes.c_int, [_vp, ctypes.c_int]),
    "smm_ctx_tune_pack_stride": (ctypes.c_int, [_vp, ctypes.c_int]),
    "smm_ctx_set_check": (ctypes.c_int, [_vp, ctypes.c_int]),
    "smm_ctx_release_pool": (ctypes.c_int, [_vp]),
    "smm_ctx_pool_bytes": (_c_i64, [_vp]),
    "smm_ctx_live_bytes": (_c_i64, [_vp]),
    "smm_ctx_inject_alloc_failure": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "smm_ctx_alloc_retries": (_c_i64, [_vp]),
    "smm_plan_check": (ctypes.c_int, [_vp, _vp]),
    "smm_plan_inject_fault": (ctypes.c_int, [_vp, _vp, ctypes.c_int]),
    "smm_csr_from_host": (ctypes.c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp, _pp]),
    "smm_csr_from_device": (ctypes.c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp, _pp]),
    "smm_csr_destroy": (None, [_vp]),
    "smm_csr_rows": (_c_i64, [_vp]),
    "smm_csr_cols": (_c_i64, [_vp]),
    "smm_csr_nnz": (_c_i64, [_vp]),
    "smm_csr_is_canonical": (ctypes.c_int, [_vp, _vp]),
    "smm_csr_update_values": (ctypes.c_int, [_vp, _vp, _vp]),
    "smm_csr_update_values_device": (ctypes.c_int, [_vp, _vp, _vp]),
    "smm_csr_device_bytes": (_c_i64, [_vp]),
    "smm_host_hash64": (ctypes.c_uint64, [_vp, _c_i64]),
    "smm_row_products": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "smm_spgemm_symbolic": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _c_i64, _pp, ctypes.POINTER(_c_i64)]),
    "smm_spgemm_numeric": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "smm_spgemm_numeric_host": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "smm_spgemm_numeric_host_i64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "smm_plan_indptr_host": (ctypes.c_int, [_vp, _vp, _vp]),
    "smm_plan_nnz": (_c_i64, [_vp]),
    "smm_plan_device_bytes": (_c_i64, [_vp]),
    "smm_plan_destroy": (None, [_vp]),
    "smm_csr_mirror_symbolic": (ctypes.c_int, [_vp, _c_i64, _vp, _vp, _vp, ctypes.POINTER(_c_i64)]),
    "smm_csr_mirror_fill": (ctypes.c_int, [_vp, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "smm_spgemm_dense": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _c_i64, _vp]),
    "smm_spgemm_dense_host": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _c_i64, _vp]),
    "smm_triple_product": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _c_i64, _c_i64, _vp]),
    "smm_triple_product_host": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _c_i64, _c_i64, _vp]),
    "smm_csr_transpose": (ctypes.c_int, [_vp, _vp, _pp]),
    "smm_csr_download": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "smm_csr_copy_device": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "smm_triple_product_sparse": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _c_i64, _c_i64, _pp]),
    "smm_result_nnz": (_c_i64, [_vp]),
    "smm_result_rows": (_c_i64, [_vp]),
    "smm_result_download": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int, _vp]),
    "smm_result_copy_device": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "smm_result_destroy": (None, [_vp]),
    "smm_ctx_tune_triple_sparse": (ctypes.c_int, [_vp, _c_i64]),
    "smm_triple_product_sparse_masked": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int, _c_i64, _c_i64, _pp]),
    "smm_spgemm_masked": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int, _vp]),
    "smm_spgemm_masked_host": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int, _vp]),
    "smm_ctx_tune_masked": (ctypes.c_int, [_vp, ctypes.c_int]),
    "smm_spmm": (ctypes.c_int, [_vp] * 2 + _BLOCKS),
    "smm_spmm_host": (ctypes.c_int, [_vp] * 2 + _BLOCKS),
    "smm_triple_apply": (ctypes.c_int, [_vp] * 3 + _BLOCKS),
    "smm_triple_apply_host": (ctypes.c_int, [_vp] * 3 + _BLOCKS),
    "smm_ctx_tune_spmm": (ctypes.c_int, [_vp, ctypes.c_int, _c_i64]),
    "smm_sddmm": (ctypes.c_int, [_vp] * 2 + _BLOCKS + [_vp]),
    "smm_sddmm_host": (ctypes.c_int, [_vp] * 2 + _BLOCKS + [_vp]),
    "smm_ctx_tune_sddmm": (ctypes.c_int, [_vp, ctypes.c_int]),
    "smm_taper_build": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, _c_i64, _vp, _c_i64, _c_i64, _vp, _c_i64, _pp]),
    "smm_taper_build_host": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, _c_i64, _vp, _c_i64, _c_i64, _vp, _c_i64,
                                            _pp]),
    "smm_cov_eval": (ctypes.c_int, [_vp, _vp] + _COV),
    "smm_cov_eval_host": (ctypes.c_int, [_vp, _vp] + _COV),
    "smm_variogram": (ctypes.c_int, [_vp, _vp] + _VARIOGRAM),
    "smm_variogram_host": (ctypes.c_int, [_vp, _vp] + _VARIOGRAM),
    "smm_interp_build": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, ctypes.c_int, ctypes.c_int, _c_i64, _vp, _c_i64, _pp]),
    "smm_interp_build_host": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, ctypes.c_int, ctypes.c_int, _c_i64, _vp, _c_i64, _pp]),
    "smm_innovation_solve": (ctypes.c_int, [_vp] * 4 + _SOLVE),
    "smm_innovation_solve_host": (ctypes.c_int, [_vp] * 4 + _SOLVE),
    "smm_kron_build": (ctypes.c_int, [_vp, _vp, _vp, _pp]),
    "smm_kron_apply": (ctypes.c_int, [_vp] * 3 + _BLOCKS),
    "smm_kron_apply_host": (ctypes.c_int, [_vp] * 3 + _BLOCKS),
    "smm_triple_apply_kron": (ctypes.c_int, [_vp] * 4 + _BLOCKS),
    "smm_triple_apply_kron_host": (ctypes.c_int, [_vp] * 4 + _BLOCKS),
    "smm_innovation_solve_kron": (ctypes.c_int, [_vp] * 5 + _SOLVE),
    "smm_innovation_solve_kron_host": (ctypes.c_int, [_vp] * 5 + _SOLVE),
    "smm_triple_product_sparse_masked_kron": (ctypes.c_int, [_vp] * 5 + [ctypes.c_int, _c_i64, _c_i64, _pp]),
    "smm_spgemm_masked_kron": (ctypes.c_int, [_vp] * 5 + [ctypes.c_int, _vp]),
    "smm_spgemm_masked_kron_host": (ctypes.c_int, [_vp] * 5 + [ctypes.c_int, _vp]),
    "smm_probe_fill": (ctypes.c_int, [_vp, _c_i64, _c_i64, ctypes.c_uint64, _vp, _c_i64]),
    "smm_innovation_solve_coef": (ctypes.c_int, [_vp] * 4 + _SOLVE + [_vp, _vp]),
    "smm_innovation_solve_coef_kron": (ctypes.c_int, [_vp] * 5 + _SOLVE + [_vp, _vp]),
    "smm_device_malloc": (ctypes.c_int, [_vp, _c_i64, _pp]),
    "smm_device_free": (ctypes.c_int, [_vp, _vp]),
    "smm_memcpy_d2h": (ctypes.c_int, [_vp, _vp, _vp, _c_i64]),
    "smm_memcpy_h2d": (ctypes.c_int, [_vp, _vp, _vp, _c_i64]),
}

# the legacy symbols the reference's own matrix_ops.py binds (matrix_ops.py:147-171) plus the
# rest of include/functions.h:43-84
LEGACY_SYMBOLS = [
    "create_sparsemat", "create_darray", "destroy_sparsemat", "destroy_darray", "destroy_iarray",
    "modifyalloc", "limits", "sparse_nosym", "sparse_sym", "sparsework_nosym", "sparsework_sym",
    "dense_nosym", "dense_sym", "triple_product",
]


class SmmError(RuntimeError):
    """A call into libsmm_hip.so failed; .code is the negative smm_status."""

    def __init__(self, code, message):
        super().__init__(f"libsmm_hip error {code}: {message}")
        self.code = code


def build(force=False):
    """Compile lib/libsmm_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    args = ["make", "-s", "-C", os.path.join(_HERE, "csrc")]
    if force:
        args.append("-B")
    subprocess.run(args, check=True)


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so (same
    SONAME as /opt/rocm's, which libsmm_hip.so links).  When torch is imported FIRST the dynamic
    linker hands that copy to this library too and device pointers are interchangeable
    (csr_from_torch, spgemm_torch, bench.py).  In the other order the process would hold two
    runtimes and the second one finds no device -- so, when torch is installed but not yet
    imported, its copy is loaded here first (no `import torch`: only the shared object).
    SMM_HIP_RUNTIME=system keeps /opt/rocm's runtime (a process that will never import torch)."""
    if "torch" in sys.modules or os.environ.get("SMM_HIP_RUNTIME", "") == "system":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.submodule_search_locations:
        return
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(path):
        try:
            ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


class SmmLibrary:
    """Singleton holding the loaded library (reference MatrixOpsLibrary, matrix_ops.py:51-72)."""
    _instance = None
    _lock = threading.Lock()

    def __new__(cls):
        with cls._lock:
            if cls._instance is None:
                inst = super().__new__(cls)
                inst._lib = None
                cls._instance = inst
        return cls._instance

    def get_lib(self):
        if self._lib is None:
            if not os.path.exists(LIB_PATH):
                raise OSError(
                    f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                    "or `make -C sparse_matrix_mult_amd/csrc`. This package has no CPU fallback.")
            _share_hip_runtime_with_torch()
            lib = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in V2_PROTOTYPES.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            self._lib = lib
        return self._lib


def check(lib, rc):
    if rc != 0:
        msg = lib.smm_last_error()
        raise SmmError(rc, msg.decode("utf-8", "replace") if msg else "unknown error")
