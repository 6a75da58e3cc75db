"""``ls_ivf_remove`` without a GPU: the C ABI of include/leansearch_ivf_remove.h is exported and bound, arguments are
refused before any device is touched, the host placement plan (csrc/ls_ivf_remove_plan.h) equals a from-scratch counting
sort of the survivors under sanitizers, ``IVFFlatIndex.remove_ids`` edits the buffered rows of an unbuilt index.
(The kernels' resources: tests/test_rows_cpu.py.)"""

import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from lean_explore_amd import faiss_compat, native
from lean_explore_amd.ivf import IVFFlatIndex
from tests.test_ivf_cpu import declared

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "lean-explore_amd" / "csrc"
HEADER = ROOT / "include" / "leansearch_ivf_remove.h"
INVALID = native.LS_ERR_INVALID_ARG


def test_header_symbols_exported_bound_and_disjoint():
    names = declared(HEADER)
    assert names == ["ls_ivf_remove", "ls_ivf_remove_last_kernel_ms"]
    assert sorted(native.IVF_REMOVE_SYMBOLS) == names
    for other in (native.SYMBOLS, native.IVF_SYMBOLS, native.IVF_SUBSET_SYMBOLS, native.IVF_BUILD_SYMBOLS,
                  native.IVF_BATCH_SYMBOLS, native.IVF_ADD_SYMBOLS, native.SQ8_SYMBOLS, native.SQ8_BATCH_SYMBOLS,
                  native.SUBSET_BATCH_SYMBOLS, native.BM25_SUBSET_SYMBOLS):
        assert not set(native.IVF_REMOVE_SYMBOLS) & set(other)
    raw = ctypes.CDLL(str(native.LIB_PATH))
    lib = native.load()
    for n in names:
        assert hasattr(raw, n), f"{n} declared in leansearch_ivf_remove.h but not exported"
        assert getattr(lib, n).argtypes == native.IVF_REMOVE_SYMBOLS[n][1], n  # load() bound it


def test_bad_arguments_are_refused_with_a_message_and_without_a_device():
    lib = native.load()
    bm = np.array([0xff, 0x01], np.uint8)
    removed = ctypes.c_int64(-7)
    assert lib.ls_ivf_remove(None, bm.ctypes.data, 2, ctypes.byref(removed)) == INVALID
    assert b"ls_ivf_remove" in lib.ls_last_error() and b"handle null" in lib.ls_last_error()
    assert lib.ls_ivf_remove(None, None, 0, None) == INVALID  # (even a removal of nothing needs a handle)
    # every argument is checked before the handle is touched: a handle that is never dereferenced stands in for one
    fake = ctypes.c_void_p(1)
    assert lib.ls_ivf_remove(fake, bm.ctypes.data, -1, ctypes.byref(removed)) == INVALID
    assert b"ls_ivf_remove" in lib.ls_last_error() and b"nbytes=-1" in lib.ls_last_error()
    assert lib.ls_ivf_remove(fake, None, 2, ctypes.byref(removed)) == INVALID
    assert b"ls_ivf_remove" in lib.ls_last_error() and b"bitmap null" in lib.ls_last_error()
    assert removed.value == -7
    assert lib.ls_ivf_remove_last_kernel_ms(None, None, None) == INVALID
    assert b"ls_ivf_remove_last_kernel_ms" in lib.ls_last_error()


# ---- remove_ids before the build: host work on the buffered rows -----------------------------------------------------
D, NLIST, N = 8, 4, 37


def _rows():
    rng = np.random.default_rng(5)
    return rng.standard_normal((N, D), dtype=np.float32), rng.integers(0, NLIST, N).astype(np.int32)


def _trained(named, parts=(10, 0, 27)):
    """A host-only index with the N rows buffered in three adds (one of them empty)."""
    x, a = _rows()
    ix = IVFFlatIndex(D, NLIST)
    ix.set_centroids(np.eye(NLIST, D, dtype=np.float32))
    r0 = 0
    for m in parts:
        ix.add(x[r0:r0 + m], assign=a[r0:r0 + m] if named else None)
        r0 += m
    assert ix.ntotal == N
    return ix, x, a


def _selections():
    mask = np.zeros(N, bool)
    mask[[0, 5, 6, 20, N - 1]] = True
    bits = np.zeros(N, bool)
    bits[[1, 9, 33]] = True
    return [
        ("mask", mask, np.flatnonzero(mask)),
        ("ids", np.array([3, 11, 12], np.int64), np.array([3, 11, 12])),
        ("duplicated and out-of-range ids", np.array([7, 7, 30, -1, N, N + 100, 7], np.int64), np.array([7, 30])),
        ("range", faiss_compat.IDSelectorRange(8, 15), np.arange(8, 15)),
        ("range past the end", faiss_compat.IDSelectorRange(30, 1000), np.arange(30, N)),
        ("batch", faiss_compat.IDSelectorBatch([2, 4, 4, 36, 99]), np.array([2, 4, 36])),
        ("bitmap", faiss_compat.IDSelectorBitmap(np.packbits(bits, bitorder="little")), np.flatnonzero(bits)),
        ("nothing", np.zeros(N, bool), np.zeros(0, np.int64)),
        ("no ids", np.zeros(0, np.int64), np.zeros(0, np.int64)),
        ("everything", np.ones(N, bool), np.arange(N)),
    ]


@pytest.mark.parametrize("named", [True, False])
@pytest.mark.parametrize("case", range(len(_selections())))
def test_remove_ids_before_the_build_edits_the_buffers(named, case):
    name, sel, gone = _selections()[case]
    ix, x, a = _trained(named)
    assert ix.remove_ids(sel) == len(gone), name
    assert ix.ntotal == N - len(gone)
    assert ix._handle is None, "no handle is created"
    assert np.array_equal(ix.reconstruct_n(), np.delete(x, gone, axis=0)), name
    if ix.ntotal:
        assert np.array_equal(ix.reconstruct_n(1, 1), np.delete(x, gone, axis=0)[1:2])
    if named and ix.ntotal:
        lists = np.concatenate(ix._assign)
        assert np.array_equal(lists, np.delete(a, gone)), "named lists stay aligned with the rows"
        assert sum(p.shape[0] for p in ix._pending) == lists.shape[0] == ix.ntotal
    elif not named:
        assert ix._assign is None
    # the "either every add names its lists or none does" rule is untouched
    if ix.ntotal:
        with pytest.raises(ValueError, match="either every add"):
            ix.add(x[:2], assign=None if named else a[:2])
    ix.add(x[:2], assign=a[:2] if named else None)
    assert ix.ntotal == N - len(gone) + 2 and ix._handle is None
    assert np.array_equal(ix.reconstruct_n(), np.concatenate([np.delete(x, gone, axis=0), x[:2]]))


def test_two_removals_in_a_row_before_the_build_renumber_densely():
    ix, x, a = _trained(True)
    assert ix.remove_ids(np.array([0, 10])) == 2
    assert ix.remove_ids(np.array([0, 9])) == 2  # (old rows 1 and 11)
    gone = [0, 1, 10, 11]
    assert ix.ntotal == N - 4 and ix._handle is None
    assert np.array_equal(ix.reconstruct_n(), np.delete(x, gone, axis=0))
    assert np.array_equal(np.concatenate(ix._assign), np.delete(a, gone))


def test_remove_ids_refuses_an_untrained_index_and_a_wrong_mask_shape():
    with pytest.raises(ValueError, match="not trained"):
        IVFFlatIndex(D, NLIST).remove_ids(np.zeros(0, bool))
    ix, x, a = _trained(True)
    for bad in (np.zeros(N + 1, bool), np.zeros(N - 1, bool), np.zeros((N, 1), bool)):
        with pytest.raises(ValueError, match="bool mask"):
            ix.remove_ids(bad)
    with pytest.raises(ValueError, match="row selection"):
        ix.remove_ids(np.array([0.5, 1.0]))
    assert ix.ntotal == N and ix._handle is None
    assert np.array_equal(ix.reconstruct_n(), x)


def test_remove_ids_on_a_built_index_makes_one_library_call(monkeypatch):
    """The built path with the library stubbed out: one ``ls_ivf_remove`` with the selection's bitmap, ntotal follows
    the count the library reports."""
    calls = []

    class Lib:
        def ls_ivf_remove(self, h, bitmap, nbytes, out_removed):
            calls.append((h, bytes((ctypes.c_uint8 * nbytes).from_address(bitmap)), nbytes))
            out_removed._obj.value = 3
            return 0

        def ls_ivf_destroy(self, h):
            return None

    monkeypatch.setattr(native, "load", lambda: Lib())
    ix, x, a = _trained(True)
    ix._pending, ix._assign, ix._names_lists = [], None, True  # what _ensure_built leaves behind ...
    ix._handle = ctypes.c_void_p(1)                              # ... with the handle
    try:
        assert ix.remove_ids(np.array([0, 9, 36])) == 3
        assert ix.ntotal == N - 3
        want = np.zeros(N, bool)
        want[[0, 9, 36]] = True
        assert calls == [(ix._handle, np.packbits(want, bitorder="little").tobytes(), (N + 7) // 8)]
    finally:
        ix._handle = None


def test_the_faiss_surface_documents_the_renumbering():
    doc = faiss_compat.IndexIVFFlat.__doc__
    assert "remove_ids" in doc and "IndexFlat.remove_ids" in doc and "RENUMBERED" in doc
    ix = faiss_compat.IndexIVFFlat(None, D, NLIST, ivf=True)
    assert isinstance(ix, IVFFlatIndex) and callable(ix.remove_ids)


# ---- the host plan -------------------------------------------------------------------------------------------------
def test_host_plan_under_sanitizers(tmp_path):
    """csrc/ls_ivf_remove_plan.h in a plain host program with its own main (tests/ivf_remove_plan_check.cpp), built
    with AddressSanitizer and UndefinedBehaviorSanitizer: 10 named edge cases, 400 random (index, bitmap) pairs against
    a from-scratch counting sort of the surviving assignment, the row kernel's deal of (row, chunk) pairs and the subset
    kernels' (list, step, lane) deal against a sequential compaction."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host check of ls_ivf_remove_plan.h"
    exe = tmp_path / "ivf_remove_plan_check"
    p = subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", str(CSRC),
                        str(ROOT / "tests" / "ivf_remove_plan_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.strip() == f"OK {10 + 400 + 12 * 6 * 2 + 5 * 3} cases"
