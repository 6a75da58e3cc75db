"""ctypes binding of libleansearch.so (include/leansearch.h) — the only way Python reaches the
HIP kernels. There is no fallback: if the shared library is missing, or no MI355X is visible,
every compute call raises.

The reference reaches its dense index through the faiss SWIG module
(reference src/lean_explore/search/engine.py:156,240); this module is the counterpart of that
import for the HIP library.
"""

from __future__ import annotations

import ctypes
import os
from pathlib import Path

LS_OK = 0
LS_ERR_INVALID_ARG = -1
LS_ERR_NO_DEVICE = -2
LS_ERR_HIP = -3
LS_ERR_K_TOO_LARGE = -4
LS_ERR_OVERFLOW = -5

LS_DTYPE_F32 = 0
LS_DTYPE_F16 = 1
LS_DTYPE_SQ8 = 2
LS_DTYPE_BF16 = 3
LS_FLAG_NORMALIZE = 1
LS_FLAG_ASYNC = 2
LS_FLAG_PIPELINE = 4
LS_FLAG_INORDER = 8
LS_MAX_K = 2048
LS_METRIC_INNER_PRODUCT = 0
LS_METRIC_L2 = 1

_PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("LEANSEARCH_LIB", _PKG_DIR / "libleansearch.so"))

# every symbol include/leansearch.h declares: (restype, argtypes)
_vp = ctypes.c_void_p
_i32 = ctypes.c_int32
_i64 = ctypes.c_int64
_u32 = ctypes.c_uint32
_f32p = ctypes.POINTER(ctypes.c_float)
_i64p = ctypes.POINTER(ctypes.c_int64)
SYMBOLS: dict[str, tuple] = {
    "ls_create": (ctypes.c_int, [ctypes.POINTER(_vp), _vp, _i64, _i32, _i32, _i32]),
    "ls_create_from_device": (ctypes.c_int, [ctypes.POINTER(_vp), _vp, _i64, _i32, _i32, _i32]),
    "ls_create_sharded": (ctypes.c_int, [ctypes.POINTER(_vp), _vp, _i64, _i32, _i32, _vp, _i32]),
    "ls_create_replicated": (ctypes.c_int, [ctypes.POINTER(_vp), _vp, _i64, _i32, _i32, _vp, _i32]),
    "ls_create_sharded_from_device": (ctypes.c_int, [ctypes.POINTER(_vp), _vp, _vp, _i32, _i32, _vp,
                                                     _i32]),
    "ls_shard_count": (_i32, [_vp]),
    "ls_shard_info": (ctypes.c_int, [_vp, _i32, ctypes.POINTER(_i32), _i64p, _i64p]),
    "ls_shard_exchange_info": (_i32, [_vp, ctypes.c_char_p, _i32]),
    "ls_add": (ctypes.c_int, [_vp, _vp, _i64]),
    "ls_reconstruct": (ctypes.c_int, [_vp, _i64, _i64, _vp]),
    "ls_destroy": (None, [_vp]),
    "ls_ntotal": (_i64, [_vp]),
    "ls_dim": (_i32, [_vp]),
    "ls_dtype": (_i32, [_vp]),
    "ls_device": (_i32, [_vp]),
    "ls_set_base": (ctypes.c_int, [_vp, _i64]),
    "ls_set_f16_small_batch": (ctypes.c_int, [_vp, _i32]),
    "ls_search": (ctypes.c_int, [_vp, _vp, _i64, _i32, _u32, _vp, _vp]),
    "ls_search_device": (ctypes.c_int, [_vp, _vp, _i64, _i32, _u32, _vp, _vp, _vp]),
    "ls_subset_create": (ctypes.c_int, [_vp, _vp, _i64, ctypes.POINTER(_i32), _i64p]),
    "ls_subset_destroy": (ctypes.c_int, [_vp, _i32]),
    "ls_search_subset": (ctypes.c_int, [_vp, _i32, _vp, _i64, _i32, _u32, _vp, _vp]),
    "ls_check": (ctypes.c_int, [_vp, _vp]),
    "ls_export_flags": (ctypes.c_int, [_vp, _vp, _i64, _vp]),
    "ls_normalize_l2": (ctypes.c_int, [_vp, _i64, _i32, _i32]),
    "ls_merge_topk": (ctypes.c_int, [_vp, _vp, _i32, _i64, _i32, _vp, _vp, _i32, _vp]),
    "ls_merge_topk_strided": (ctypes.c_int, [_vp, _vp, _i64, _i32, _i64, _i32, _vp, _vp, _i32, _vp]),
    "ls_set_profiling": (ctypes.c_int, [_vp, _i32]),
    "ls_last_kernel_ms": (ctypes.c_int, [_vp, _f32p, _f32p]),
    "ls_debug_option": (ctypes.c_int, [_vp, _i32, _i32]),
    "ls_debug_counter": (_i64, [_vp, _i32]),
    "ls_debug_read_scores": (ctypes.c_int, [_vp, _vp, _i64]),
    "ls_bm25_create": (ctypes.c_int, [ctypes.POINTER(_vp), _vp, _vp, _vp, _vp, _i64, _i64, _i32]),
    "ls_bm25_search": (ctypes.c_int, [_vp, _vp, _i32, _i32, _vp, _vp]),
    "ls_bm25_ntotal": (_i64, [_vp]),
    "ls_bm25_debug_counter": (_i64, [_vp, _i32]),
    "ls_bm25_destroy": (None, [_vp]),
    "ls_last_error": (ctypes.c_char_p, []),
    "ls_version": (ctypes.c_char_p, []),
    "ls_device_count": (_i32, []),
}

# every symbol include/leansearch_ivf.h declares (the IVF-flat search, bound by load() as well)
_i32p = ctypes.POINTER(_i32)
IVF_SYMBOLS: dict[str, tuple] = {
    "ls_ivf_create": (ctypes.c_int, [ctypes.POINTER(_vp), _vp, _i64, _i32, _i32, _vp, _i32, _vp, _i32]),
    "ls_ivf_search": (ctypes.c_int, [_vp, _vp, _i64, _i32, _i32, _u32, _vp, _vp]),
    "ls_ivf_ntotal": (_i64, [_vp]),
    "ls_ivf_dim": (_i32, [_vp]),
    "ls_ivf_nlist": (_i32, [_vp]),
    "ls_ivf_list_sizes": (ctypes.c_int, [_vp, _vp]),
    "ls_ivf_assignment": (ctypes.c_int, [_vp, _vp]),
    "ls_ivf_destroy": (None, [_vp]),
    "ls_ivf_set_profiling": (ctypes.c_int, [_vp, _i32]),
    "ls_ivf_last_kernel_ms": (ctypes.c_int, [_vp, _f32p, _f32p, _i32p]),
}

# every symbol include/leansearch_ivf_subset.h declares (IVF-flat search over a row subset)
IVF_SUBSET_SYMBOLS: dict[str, tuple] = {
    "ls_ivf_subset_create": (ctypes.c_int, [_vp, _vp, _i64, _i32p, _i64p]),
    "ls_ivf_subset_destroy": (ctypes.c_int, [_vp, _i32]),
    "ls_ivf_subset_list_sizes": (ctypes.c_int, [_vp, _i32, _vp]),
    "ls_ivf_search_subset": (ctypes.c_int, [_vp, _i32, _vp, _i64, _i32, _i32, _u32, _vp, _vp]),
}

# every symbol include/leansearch_sq8.h declares (the 8-bit storage dtype)
SQ8_SYMBOLS: dict[str, tuple] = {
    "ls_create_sq8": (ctypes.c_int, [ctypes.POINTER(_vp), _vp, _i64, _i32, _vp, _i32]),
    "ls_sq8_step": (ctypes.c_int, [_vp, _vp]),
    "ls_sq8_codes": (ctypes.c_int, [_vp, _i64, _i64, _vp]),
    "ls_sq8_geom": (ctypes.c_int, [_i32, _i32p, _i32p, _i32p]),
}

# every symbol include/leansearch_sq8_batch.h declares (the opt-in small-batch pass of an sq8 index)
SQ8_BATCH_SYMBOLS: dict[str, tuple] = {
    "ls_set_sq8_small_batch": (ctypes.c_int, [_vp, _i32]),
}

# every symbol include/leansearch_subset_batch.h declares (the opt-in pass that serves 2..16 queries of a subset search)
SUBSET_BATCH_SYMBOLS: dict[str, tuple] = {
    "ls_set_subset_small_batch": (ctypes.c_int, [_vp, _i32]),
}

# every symbol include/leansearch_ivf_batch.h declares (the opt-in pass that serves 2..16 queries of an IVF search)
IVF_BATCH_SYMBOLS: dict[str, tuple] = {
    "ls_ivf_set_small_batch": (ctypes.c_int, [_vp, _i32]),
    "ls_ivf_last_passes": (ctypes.c_int, [_vp, _i32p, _i64p]),
}

# every symbol include/leansearch_bm25_subset.h declares (BM25 retrieval over a subset of the documents)
BM25_SUBSET_SYMBOLS: dict[str, tuple] = {
    "ls_bm25_subset_create": (ctypes.c_int, [_vp, _vp, _i64, _i32p, _i64p]),
    "ls_bm25_subset_destroy": (ctypes.c_int, [_vp, _i32]),
    "ls_bm25_search_subset": (ctypes.c_int, [_vp, _i32, _vp, _i32, _i32, _vp, _vp]),
}

# every symbol include/leansearch_ivf_build.h declares (IVF build on the GPU: k-means steps, list assignment, read-back)
IVF_BUILD_SYMBOLS: dict[str, tuple] = {
    "ls_ivf_trainer_create": (ctypes.c_int, [ctypes.POINTER(_vp), _vp, _i64, _i32, _i32, _i32]),
    "ls_ivf_trainer_assign": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "ls_ivf_trainer_means": (ctypes.c_int, [_vp, _vp]),
    "ls_ivf_trainer_last_kernel_ms": (ctypes.c_int, [_vp, _f32p, _f32p]),
    "ls_ivf_trainer_destroy": (None, [_vp]),
    "ls_ivf_assign": (ctypes.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _i32]),
    "ls_ivf_reconstruct": (ctypes.c_int, [_vp, _i64, _i64, _vp]),
}

# every symbol include/leansearch_ivf_add.h declares (rows added to a built IVF handle, lists merged on the GPU)
IVF_ADD_SYMBOLS: dict[str, tuple] = {
    "ls_ivf_add": (ctypes.c_int, [_vp, _vp, _i64, _vp]),
    "ls_ivf_add_last_kernel_ms": (ctypes.c_int, [_vp, _f32p, _i64p]),
}

# every symbol include/leansearch_ivf_remove.h declares (rows removed from a built IVF handle, lists compacted on the GPU)
IVF_REMOVE_SYMBOLS: dict[str, tuple] = {
    "ls_ivf_remove": (ctypes.c_int, [_vp, _vp, _i64, _i64p]),
    "ls_ivf_remove_last_kernel_ms": (ctypes.c_int, [_vp, _f32p, _i64p]),
}

# every symbol include/leansearch_remove.h declares (rows removed from a built flat handle, compacted in place in HBM)
REMOVE_SYMBOLS: dict[str, tuple] = {
    "ls_remove": (ctypes.c_int, [_vp, _vp, _i64, _i64p]),
    "ls_subset_rows": (ctypes.c_int, [_vp, _i32, _i64p]),
    "ls_remove_set_slab_rows": (ctypes.c_int, [_vp, _i64]),
    "ls_remove_last": (ctypes.c_int, [_vp, _i64p, _i64p, _f32p, _i64p]),
}

# every symbol include/leansearch_range.h declares (range search: all rows scoring above a radius, flat and IVF handles)
RANGE_SYMBOLS: dict[str, tuple] = {
    "ls_range_search": (ctypes.c_int, [_vp, _vp, _i64, ctypes.c_float, _u32, ctypes.POINTER(_vp)]),
    "ls_range_search_subset": (ctypes.c_int, [_vp, _i32, _vp, _i64, ctypes.c_float, _u32, ctypes.POINTER(_vp)]),
    "ls_ivf_range_search": (ctypes.c_int, [_vp, _vp, _i64, ctypes.c_float, _i32, _u32, ctypes.POINTER(_vp)]),
    "ls_ivf_range_search_subset": (ctypes.c_int, [_vp, _i32, _vp, _i64, ctypes.c_float, _i32, _u32,
                                                  ctypes.POINTER(_vp)]),
    "ls_range_nq": (_i64, [_vp]),
    "ls_range_lims": (_vp, [_vp]),
    "ls_range_scores": (_vp, [_vp]),
    "ls_range_rows": (_vp, [_vp]),
    "ls_range_kernel_ms": (ctypes.c_float, [_vp]),
    "ls_range_free": (None, [_vp]),
}

# every symbol include/leansearch_l2.h declares (the L2 metric: squared-distance search on the flat index)
L2_SYMBOLS: dict[str, tuple] = {
    "ls_create_l2": (ctypes.c_int, [ctypes.POINTER(_vp), _vp, _i64, _i32, _i32, _i32]),
    "ls_create_l2_from_device": (ctypes.c_int, [ctypes.POINTER(_vp), _vp, _i64, _i32, _i32, _i32]),
    "ls_metric": (_i32, [_vp]),
}

# every symbol include/leansearch_l2_batch.h declares (opt-in: 2..8 queries of an L2 index share one corpus pass)
L2_BATCH_SYMBOLS: dict[str, tuple] = {
    "ls_set_l2_small_batch": (ctypes.c_int, [_vp, _i32]),
    "ls_l2_small_batch": (_i32, [_vp]),
}

# every symbol include/leansearch_ivf_l2.h declares (the L2 metric on the IVF index: create, metric, assignment, trainer)
IVF_L2_SYMBOLS: dict[str, tuple] = {
    "ls_ivf_create_l2": (ctypes.c_int, [ctypes.POINTER(_vp), _vp, _i64, _i32, _i32, _vp, _i32, _vp, _i32]),
    "ls_ivf_metric": (_i32, [_vp]),
    "ls_ivf_assign_l2": (ctypes.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _i32]),
    "ls_ivf_trainer_create_l2": (ctypes.c_int, [ctypes.POINTER(_vp), _vp, _i64, _i32, _i32, _i32]),
}

# every symbol include/leansearch_bf16.h declares (the bfloat16 storage dtype)
BF16_SYMBOLS: dict[str, tuple] = {
    "ls_bf16_rows": (ctypes.c_int, [_vp, _i64, _i64, _vp]),
    "ls_bf16_inexact": (ctypes.c_int, [_vp, _i64p]),
    "ls_ivf_bf16_inexact": (ctypes.c_int, [_vp, _i64p]),
}

_lib: ctypes.CDLL | None = None


class LeanSearchError(RuntimeError):
    """A libleansearch call failed (carries the library's thread-local message)."""

    def __init__(self, code: int, message: str):
        super().__init__(f"libleansearch error {code}: {message}")
        self.code = code


def _preload_hip_runtime() -> None:
    """One HIP runtime per process. PyTorch wheels bundle their own libamdhip64.so.7 (same
    SONAME as /opt/rocm's); whichever is mapped first serves both, and torch cannot initialise
    on top of the system copy. So when torch is installed, map ITS runtime before ours resolves
    its NEEDED entry. Without torch, libleansearch binds to /opt/rocm as linked."""
    import importlib.util

    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = Path(list(spec.submodule_search_locations)[0]) / "lib" / "libamdhip64.so"
    if cand.exists():
        ctypes.CDLL(str(cand), mode=ctypes.RTLD_GLOBAL)


def load() -> ctypes.CDLL:
    """Load libleansearch.so and bind every declared symbol. Raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc, gfx950). There is no CPU fallback for the dense search path.")
    _preload_hip_runtime()
    lib = ctypes.CDLL(str(LIB_PATH))
    for name, (restype, argtypes) in (list(SYMBOLS.items()) + list(IVF_SYMBOLS.items()) + list(SQ8_SYMBOLS.items()) + list(SQ8_BATCH_SYMBOLS.items())
                                       + list(BM25_SUBSET_SYMBOLS.items()) + list(IVF_SUBSET_SYMBOLS.items())
                                       + list(SUBSET_BATCH_SYMBOLS.items()) + list(IVF_BUILD_SYMBOLS.items())
                                       + list(IVF_BATCH_SYMBOLS.items()) + list(IVF_ADD_SYMBOLS.items())
                                       + list(IVF_REMOVE_SYMBOLS.items()) + list(REMOVE_SYMBOLS.items())
                                       + list(RANGE_SYMBOLS.items()) + list(L2_SYMBOLS.items())
                                       + list(IVF_L2_SYMBOLS.items()) + list(L2_BATCH_SYMBOLS.items())
                                       + list(BF16_SYMBOLS.items())):
        fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


_fast = None
_fast_tried = False


def fast_search():
    """(module, address of ls_search) of the CPython binding csrc/lsfast.c, or None: the same symbol
    of the same library as the ctypes binding, minus ~1.5 us of argument conversion per call."""
    global _fast, _fast_tried
    if not _fast_tried:
        _fast_tried = True
        try:
            from . import _lsfast
            _fast = (_lsfast, ctypes.cast(load().ls_search, ctypes.c_void_p).value)
        except ImportError:
            _fast = None
    return _fast


_c_char_from_buffer = ctypes.c_char.from_buffer
_addressof = ctypes.addressof


def addr(a) -> int | None:
    """Base address of a C-contiguous numpy array for a pointer argument (None if it is empty).
    ``ndarray.ctypes.data`` builds a helper object per access (1.4 us; three of them were most of
    the interpreter's share of a 64 us ``ls_search``); the buffer protocol gives the same address
    in 0.4 us. Read-only arrays do not export a writable buffer and take the slow way."""
    if not a.size:
        return None
    try:
        return _addressof(_c_char_from_buffer(a))
    except (TypeError, ValueError):
        return a.ctypes.data


def check(rc: int) -> None:
    if rc == LS_OK:
        return
    msg = load().ls_last_error().decode("utf-8", "replace")
    if rc == LS_ERR_INVALID_ARG:
        raise ValueError(f"libleansearch: {msg}")
    raise LeanSearchError(rc, msg)


def device_count() -> int:
    return int(load().ls_device_count())


def version() -> str:
    return load().ls_version().decode()
