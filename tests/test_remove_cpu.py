"""``ls_remove`` without a GPU: the C ABI of include/leansearch_remove.h is exported and bound, arguments are refused
before any device is touched, the host plan (csrc/ls_remove_plan.h) holds to a sequential model under sanitizers - the
in-place slab schedule never reads a row after a write to it -, ``FlatIPIndex.remove_ids`` edits the buffered rows of
an unbuilt index. (The kernels' resources: tests/test_rows_cpu.py.)"""

import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from lean_explore_amd import faiss_compat, native
from lean_explore_amd.index import FlatIPIndex
from tests.test_ivf_cpu import declared

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "lean-explore_amd" / "csrc"
HEADER = ROOT / "include" / "leansearch_remove.h"
INVALID = native.LS_ERR_INVALID_ARG


def test_header_symbols_exported_bound_and_disjoint():
    names = declared(HEADER)
    assert names == ["ls_remove", "ls_remove_last", "ls_remove_set_slab_rows", "ls_subset_rows"]
    assert sorted(native.REMOVE_SYMBOLS) == names
    others = [getattr(native, t) for t in dir(native) if t.endswith("SYMBOLS") and t != "REMOVE_SYMBOLS"]
    assert len(others) >= 11  # SYMBOLS and every *_SYMBOLS table
    for other in others:
        assert not set(native.REMOVE_SYMBOLS) & set(other)
    raw = ctypes.CDLL(str(native.LIB_PATH))
    lib = native.load()
    for n in names:
        assert hasattr(raw, n), f"{n} declared in leansearch_remove.h but not exported"
        assert getattr(lib, n).argtypes == native.REMOVE_SYMBOLS[n][1], n  # load() bound it
    # leansearch.h stays as it is
    assert "ls_remove" not in (ROOT / "include" / "leansearch.h").read_text()


def test_bad_arguments_are_refused_with_a_message_and_without_a_device():
    lib = native.load()
    bm = np.array([0xff, 0x01], np.uint8)
    removed = ctypes.c_int64(-7)
    assert lib.ls_remove(None, bm.ctypes.data, 2, ctypes.byref(removed)) == INVALID
    assert b"ls_remove:" in lib.ls_last_error() and b"handle null" in lib.ls_last_error()
    assert lib.ls_remove(None, None, 0, None) == INVALID  # (even a removal of nothing needs a handle)
    # every argument is checked before the handle is touched: a handle that is never dereferenced stands in for one
    fake = ctypes.c_void_p(1)
    assert lib.ls_remove(fake, bm.ctypes.data, -1, ctypes.byref(removed)) == INVALID
    assert b"ls_remove:" in lib.ls_last_error() and b"nbytes=-1" in lib.ls_last_error()
    assert lib.ls_remove(fake, None, 2, ctypes.byref(removed)) == INVALID
    assert b"ls_remove:" in lib.ls_last_error() and b"bitmap null" in lib.ls_last_error()
    assert removed.value == -7
    rows = ctypes.c_int64(-7)
    assert lib.ls_subset_rows(None, 1, ctypes.byref(rows)) == INVALID
    assert b"ls_subset_rows" in lib.ls_last_error() and b"handle null" in lib.ls_last_error()
    assert lib.ls_subset_rows(fake, 1, None) == INVALID
    assert b"ls_subset_rows" in lib.ls_last_error() and b"out_rows null" in lib.ls_last_error()
    assert lib.ls_remove_set_slab_rows(None, 0) == INVALID
    assert b"ls_remove_set_slab_rows" in lib.ls_last_error() and b"handle null" in lib.ls_last_error()
    assert lib.ls_remove_set_slab_rows(fake, -1) == INVALID
    assert b"ls_remove_set_slab_rows" in lib.ls_last_error() and b"rows < 0" in lib.ls_last_error()
    assert lib.ls_remove_last(None, None, None, None, None) == INVALID
    assert b"ls_remove_last" in lib.ls_last_error() and b"handle null" in lib.ls_last_error()
    assert rows.value == -7


# ---- remove_ids before the build: host work on the buffered rows -----------------------------------------------------
D, N = 8, 37


def _buffered(parts=(10, 0, 27), dtype="f32"):
    """A host-only index with the N rows buffered in three adds (one of them empty)."""
    x = np.random.default_rng(5).standard_normal((N, D), dtype=np.float32)
    ix = FlatIPIndex(D, dtype=dtype)
    r0 = 0
    for m in parts:
        ix.add(x[r0:r0 + m])
        r0 += m
    assert ix.ntotal == N and ix._handle is None
    return ix, x


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
        ("everything", np.ones(N, bool), np.arange(N)),
    ]


@pytest.mark.parametrize("dtype", ["f32", "sq8"])
@pytest.mark.parametrize("case", range(len(_selections())))
def test_remove_ids_before_the_build_edits_the_buffers(case, dtype):
    name, sel, gone = _selections()[case]
    ix, x = _buffered(dtype=dtype)
    assert ix.remove_ids(sel) == len(gone), name
    assert ix.ntotal == N - len(gone)
    assert ix._handle is None, "no handle is created"
    assert np.array_equal(ix.host_corpus(), np.delete(x, gone, axis=0)), name
    ix.add(x[:2])  # an add afterwards appends
    assert ix.ntotal == N - len(gone) + 2 and ix._handle is None
    assert np.array_equal(ix.host_corpus(), np.concatenate([np.delete(x, gone, axis=0), x[:2]]))


def test_two_removals_in_a_row_before_the_build_renumber_densely():
    ix, x = _buffered()
    assert ix.remove_ids(np.array([0, 10])) == 2
    assert ix.remove_ids(np.array([0, 9])) == 2  # (old rows 1 and 11)
    assert ix.ntotal == N - 4 and ix._handle is None
    assert np.array_equal(ix.host_corpus(), np.delete(x, [0, 1, 10, 11], axis=0))


def test_remove_ids_refuses_a_wrong_mask_shape_and_a_float_array():
    ix, x = _buffered()
    for bad in (np.zeros(N + 1, bool), np.zeros(N - 1, bool), np.zeros((N, 1), bool)):
        with pytest.raises(ValueError, match="bool mask"):
            ix.remove_ids(bad)
    with pytest.raises(ValueError, match="row selection"):
        ix.remove_ids(np.array([0.5, 1.0]))
    assert ix.ntotal == N and ix._handle is None
    assert np.array_equal(ix.host_corpus(), x)


def test_remove_ids_on_a_built_index_makes_one_library_call(monkeypatch):
    """The built path with the library stubbed out: one ``ls_remove`` with exactly the packed bitmap, ntotal follows
    the count the library reports."""
    calls = []

    class Lib:
        def ls_remove(self, h, bitmap, nbytes, out_removed):
            calls.append((h, bytes((ctypes.c_uint8 * nbytes).from_address(bitmap)), nbytes))
            out_removed._obj.value = 2  # (not the 3 rows selected: ntotal must follow the library)
            return 0

        def ls_destroy(self, h):
            return None

    monkeypatch.setattr(native, "load", lambda: Lib())
    ix, x = _buffered()
    ix._pending = []                   # what _ensure_built leaves behind ...
    ix._handle = ctypes.c_void_p(1)    # ... with the handle
    try:
        assert ix.remove_ids(np.array([0, 9, 36])) == 2
        assert ix.ntotal == N - 2
        want = np.zeros(N, bool)
        want[[0, 9, 36]] = True
        assert calls == [(ix._handle, np.packbits(want, bitorder="little").tobytes(), (N + 7) // 8)]
    finally:
        ix._handle = None


def test_the_faiss_surface_inherits_remove_ids_and_documents_the_renumbering():
    for cls, args in ((faiss_compat.IndexFlatIP, (D,)), (faiss_compat.IndexIVFFlat, (None, D, 4)),
                      (faiss_compat.IndexScalarQuantizer, (D,))):
        assert "remove_ids" in cls.__doc__ and "IndexFlat.remove_ids" in cls.__doc__, cls
        ix = cls(*args)
        assert isinstance(ix, FlatIPIndex) and cls.remove_ids is FlatIPIndex.remove_ids
        x = np.random.default_rng(1).standard_normal((N, D), dtype=np.float32)
        ix.add(x)
        assert ix.remove_ids(faiss_compat.IDSelectorRange(3, 6)) == 3 and ix.ntotal == N - 3 and ix._handle is None
        assert np.array_equal(ix.host_corpus(), np.delete(x, [3, 4, 5], axis=0))


def test_write_index_after_a_removal_before_the_build_writes_the_survivors(tmp_path):
    ix, x = _buffered()
    ix.remove_ids(np.array([1, 2, 30]))
    faiss_compat.write_index(ix, tmp_path / "flat.index")
    assert ix._handle is None
    with open(tmp_path / "flat.index", "rb") as f:
        f.read(4)
        d, xb = faiss_compat._read_flat_payload(f)
    assert d == D and np.array_equal(xb, np.delete(x, [1, 2, 30], axis=0))


# ---- the host plan -------------------------------------------------------------------------------------------------
def test_host_plan_under_sanitizers(tmp_path):
    """csrc/ls_remove_plan.h in a plain host program with its own main (tests/remove_plan_check.cpp), built with
    AddressSanitizer and UndefinedBehaviorSanitizer: 14 named edge cases, shard slices at the bit offsets 0..7 and 400
    random (n, bitmap, slab rows, shard split) pairs against a sequential model that fails on a read after a write."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host check of ls_remove_plan.h"
    exe = tmp_path / "remove_plan_check"
    p = subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", str(CSRC),
                        str(ROOT / "tests" / "remove_plan_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.strip() == f"OK {14 + 8 + 400} cases"
