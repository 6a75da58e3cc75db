"""Range search without a GPU: the C ABI of include/leansearch_range.h is exported and bound, arguments are refused
before any device is touched (and nothing computes without one), the Python surface marshals one library call and
copies the result out, the host plan (csrc/ls_range_plan.h) holds to a sequential threshold scan under sanitizers, and
the three kernels of csrc/ls_range.hip use no scratch and spill nothing."""

import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from lean_explore_amd import faiss_compat, native
from lean_explore_amd.index import FlatIPIndex, RowSubset
from lean_explore_amd.ivf import IVFFlatIndex, IVFSubset
from tests.test_ivf_cpu import declared
from tests.test_ivf_subset_cpu import resource_usage

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "lean-explore_amd" / "csrc"
HEADER = ROOT / "include" / "leansearch_range.h"
INVALID, NO_DEVICE = native.LS_ERR_INVALID_ARG, native.LS_ERR_NO_DEVICE
D = 8


def test_header_symbols_exported_bound_and_disjoint():
    names = declared(HEADER)
    assert names == ["ls_ivf_range_search", "ls_ivf_range_search_subset", "ls_range_free", "ls_range_kernel_ms",
                     "ls_range_lims", "ls_range_nq", "ls_range_rows", "ls_range_scores", "ls_range_search",
                     "ls_range_search_subset"]
    assert sorted(native.RANGE_SYMBOLS) == names
    others = [getattr(native, t) for t in dir(native) if t.endswith("SYMBOLS") and t != "RANGE_SYMBOLS"]
    assert len(others) >= 12  # SYMBOLS and every other *_SYMBOLS table
    for other in others:
        assert not set(native.RANGE_SYMBOLS) & set(other)
    raw = ctypes.CDLL(str(native.LIB_PATH))
    lib = native.load()
    for n in names:
        assert hasattr(raw, n), f"{n} declared in leansearch_range.h but not exported"
        assert getattr(lib, n).argtypes == native.RANGE_SYMBOLS[n][1], n  # load() bound it
    # leansearch.h and leansearch_ivf.h stay as they are
    for h in ("leansearch.h", "leansearch_ivf.h"):
        assert "ls_range" not in (ROOT / "include" / h).read_text() and "range_search" not in (ROOT / "include" / h).read_text()
    assert "ls_range.hip" in (CSRC / "Makefile").read_text()


def test_bad_arguments_are_refused_with_a_message_and_without_a_device():
    lib = native.load()
    q = np.ones((2, D), np.float32)
    qp = q.ctypes.data
    fake = ctypes.c_void_p(1)  # every argument is checked before the handle is touched: never dereferenced below
    sentinel = 0x5a5a

    def out():
        return ctypes.c_void_p(sentinel)

    calls = {
        "ls_range_search": lambda h, qq, nq, fl, o: lib.ls_range_search(h, qq, nq, 0.5, fl, o),
        "ls_range_search_subset": lambda h, qq, nq, fl, o: lib.ls_range_search_subset(h, 1, qq, nq, 0.5, fl, o),
        "ls_ivf_range_search": lambda h, qq, nq, fl, o: lib.ls_ivf_range_search(h, qq, nq, 0.5, 4, fl, o),
        "ls_ivf_range_search_subset": lambda h, qq, nq, fl, o: lib.ls_ivf_range_search_subset(h, 1, qq, nq, 0.5, 4, fl, o),
    }
    for name, call in calls.items():
        o = out()
        assert call(None, qp, 2, 0, ctypes.byref(o)) == INVALID, name  # no handle
        assert name.encode() + b":" in lib.ls_last_error()
        assert o.value is None, "*out is NULL after an error"
        assert call(fake, qp, 2, 0, None) == INVALID, name  # a null out
        o = out()
        assert call(fake, qp, -1, 0, ctypes.byref(o)) == INVALID and o.value is None, name
        assert b"nq=-1" in lib.ls_last_error()
        o = out()
        assert call(fake, None, 2, 0, ctypes.byref(o)) == INVALID and o.value is None, name  # queries missing
        for flags in (native.LS_FLAG_ASYNC, native.LS_FLAG_PIPELINE, native.LS_FLAG_INORDER,
                      native.LS_FLAG_NORMALIZE | native.LS_FLAG_ASYNC, 0x100):
            o = out()
            assert call(fake, qp, 2, flags, ctypes.byref(o)) == INVALID and o.value is None, (name, flags)
            assert b"only LS_FLAG_NORMALIZE" in lib.ls_last_error()
    for nprobe in (0, -3):
        o = out()
        assert lib.ls_ivf_range_search(fake, qp, 2, 0.5, nprobe, 0, ctypes.byref(o)) == INVALID and o.value is None
        assert b"nprobe" in lib.ls_last_error()
        assert lib.ls_ivf_range_search_subset(fake, 1, qp, 2, 0.5, nprobe, 0, ctypes.byref(o)) == INVALID
    # the accessors of a null result
    assert lib.ls_range_nq(None) == 0 and lib.ls_range_lims(None) is None and lib.ls_range_scores(None) is None
    assert lib.ls_range_rows(None) is None and lib.ls_range_kernel_ms(None) == 0.0
    lib.ls_range_free(None)  # (a no-op)


def test_nothing_computes_without_a_device(gpu_available):
    if gpu_available:
        pytest.skip("a GPU is visible; the refusal path is for CPU-only hosts")
    lib = native.load()
    q = np.ones((2, D), np.float32)
    # a zeroed block stands in for a single-device handle: only its group pointer (null) and its device number are read
    # before the device check, which comes after every argument check
    blank = ctypes.create_string_buffer(1 << 16)
    o = ctypes.c_void_p(0x5a5a)
    assert lib.ls_range_search(ctypes.addressof(blank), q.ctypes.data, 2, 0.5, 0, ctypes.byref(o)) == NO_DEVICE
    assert b"no CPU path" in lib.ls_last_error() and o.value is None
    assert lib.ls_range_search(ctypes.addressof(blank), q.ctypes.data, 2, 0.5, native.LS_FLAG_ASYNC,
                               ctypes.byref(o)) == INVALID  # (the flag check comes first)
    for ix in (FlatIPIndex(D), faiss_compat.IndexScalarQuantizer(D), _trained_ivf()):
        ix.add(np.ones((4, D), np.float32))
        with pytest.raises(native.LeanSearchError) as e:
            ix.range_search(q, 0.5)
        assert e.value.code == NO_DEVICE


def _trained_ivf():
    ivf = IVFFlatIndex(D, 2)
    ivf.set_centroids(np.eye(2, D, dtype=np.float32))
    return ivf


# ---- the Python surface with the library stubbed out ---------------------------------------------------------------------
class _Result:
    """What the stub hands back as an ``ls_range_result``: arrays kept alive by the stub, addresses as the library's."""

    def __init__(self, lims, scores, rows):
        self.lims = np.asarray(lims, np.int64)
        self.scores = np.asarray(scores, np.float32)
        self.rows = np.asarray(rows, np.int64)


class _Lib:
    def __init__(self, result):
        self.result, self.calls, self.freed = result, [], 0

    def _give(self, out):
        out._obj.value = 77
        return 0

    def ls_range_search(self, h, q, nq, radius, flags, out):
        self.calls.append(("flat", h, (ctypes.c_float * (nq * D)).from_address(q)[:], nq, radius, flags))
        return self._give(out)

    def ls_range_search_subset(self, h, sid, q, nq, radius, flags, out):
        self.calls.append(("subset", h, sid, nq, radius, flags))
        return self._give(out)

    def ls_ivf_range_search(self, h, q, nq, radius, nprobe, flags, out):
        self.calls.append(("ivf", h, nq, radius, nprobe, flags))
        return self._give(out)

    def ls_ivf_range_search_subset(self, h, sid, q, nq, radius, nprobe, flags, out):
        self.calls.append(("ivf_subset", h, sid, nq, radius, nprobe, flags))
        return self._give(out)

    def ls_range_nq(self, r):
        assert r.value == 77
        return self.result.lims.size - 1

    def ls_range_lims(self, r):
        return self.result.lims.ctypes.data

    def ls_range_scores(self, r):
        return self.result.scores.ctypes.data if self.result.scores.size else None

    def ls_range_rows(self, r):
        return self.result.rows.ctypes.data if self.result.rows.size else None

    def ls_range_free(self, r):
        assert r.value == 77
        self.freed += 1

    def ls_destroy(self, h):
        return None

    def ls_ivf_destroy(self, h):
        return None

    def ls_subset_destroy(self, h, sid):
        return 0

    def ls_ivf_subset_destroy(self, h, sid):
        return 0


def _check_copy(got, res):
    lims, Dv, Iv = got
    assert lims.dtype == np.uint64 and Dv.dtype == np.float32 and Iv.dtype == np.int64
    assert np.array_equal(lims, res.lims.astype(np.uint64)) and np.array_equal(Dv, res.scores)
    assert np.array_equal(Iv, res.rows)
    res.scores[...] = -1.0  # the arrays are copies: the library's memory may go
    res.rows[...] = -1
    res.lims[...] = 0
    assert lims[-1] == Dv.size == Iv.size and (Iv >= 0).all()


def test_flat_range_search_makes_one_library_call_and_copies_the_result(monkeypatch):
    res = _Result([0, 2, 2, 3], [0.9, 0.8, 0.7], [3, 5, 1])
    lib = _Lib(res)
    monkeypatch.setattr(native, "load", lambda: lib)
    ix = faiss_compat.IndexFlatIP(D)
    ix._handle = ctypes.c_void_p(1)
    try:
        q = np.arange(3 * D, dtype=np.float64).reshape(3, D)  # (converted to float32, row-major)
        got = ix.range_search(q, 0.5, normalize=True)
        assert lib.calls == [("flat", ix._handle, list(map(float, range(3 * D))), 3, 0.5, native.LS_FLAG_NORMALIZE)]
        assert lib.freed == 1
        _check_copy(got, res)
        # a RowSubset of this index: nothing is uploaded, the subset stays
        lib.result = _Result([0, 1], [0.25], [4])
        sub = RowSubset(ix, 9, 5)
        got = ix.range_search(q[:1], -np.inf, params=faiss_compat.SearchParameters(sel=sub))
        assert lib.calls[-1] == ("subset", ix._handle, 9, 1, -np.inf, 0) and lib.freed == 2 and sub.valid
        _check_copy(got, lib.result)
        # no hits: empty arrays of the right types, the result freed all the same
        lib.result = _Result([0, 0, 0], [], [])
        lims, Dv, Iv = ix.range_search(q[:2], np.inf)
        assert lims.tolist() == [0, 0, 0] and Dv.shape == (0,) and Iv.shape == (0,) and Iv.dtype == np.int64
        assert lib.freed == 3
        # nq = 0 and a wrong shape never reach the library
        n_calls = len(lib.calls)
        lims, Dv, Iv = ix.range_search(np.zeros((0, D), np.float32), 0.5)
        assert lims.tolist() == [0] and lims.dtype == np.uint64 and Dv.size == 0 and Iv.size == 0
        for bad in (np.zeros(D, np.float32), np.zeros((2, D + 1), np.float32)):
            with pytest.raises(ValueError, match="range_search expects"):
                ix.range_search(bad, 0.5)
        other = RowSubset(FlatIPIndex(D), 1, 1)
        with pytest.raises(ValueError, match="another index"):
            ix.range_search(q, 0.5, params=other)
        assert len(lib.calls) == n_calls and lib.freed == 3
        sub._id = other._id = None
    finally:
        ix._handle = None


def test_a_failed_call_raises_and_frees_nothing(monkeypatch):
    class Failing(_Lib):
        def ls_range_search(self, h, q, nq, radius, flags, out):
            return INVALID

        def ls_last_error(self):
            return b"ls_range_search: a sharded handle"

    lib = Failing(_Result([0], [], []))
    monkeypatch.setattr(native, "load", lambda: lib)
    ix = FlatIPIndex(D)
    ix._handle = ctypes.c_void_p(1)
    try:
        with pytest.raises(ValueError, match="sharded"):
            ix.range_search(np.zeros((1, D), np.float32), 0.5)
        assert lib.freed == 0
    finally:
        ix._handle = None


def test_ivf_range_search_handles_nprobe_and_subsets_as_search_does(monkeypatch):
    res = _Result([0, 1, 3], [0.5, 0.75, 0.25], [7, 0, 2])
    lib = _Lib(res)
    monkeypatch.setattr(native, "load", lambda: lib)
    ivf = faiss_compat.IndexIVFFlat(None, D, 4, ivf=True)
    assert isinstance(ivf, IVFFlatIndex)
    ivf.set_centroids(np.eye(4, D, dtype=np.float32))
    ivf._handle = ctypes.c_void_p(2)
    try:
        q = np.zeros((2, D), np.float32)
        ivf.nprobe = 3
        _check_copy(ivf.range_search(q, 0.125), res)
        assert lib.calls == [("ivf", ivf._handle, 2, 0.125, 3, 0)] and lib.freed == 1
        lib.result = _Result([0, 0, 1], [1.5], [6])
        sub = IVFSubset(ivf, 5, 10)
        ivf.range_search(q, 0.0, normalize=True, params=faiss_compat.SearchParametersIVF(nprobe=2, sel=sub))
        assert lib.calls[-1] == ("ivf_subset", ivf._handle, 5, 2, 0.0, 2, native.LS_FLAG_NORMALIZE)
        ivf.range_search(q, 0.0, params=sub)  # the subset itself as params: the attribute's nprobe
        assert lib.calls[-1] == ("ivf_subset", ivf._handle, 5, 2, 0.0, 3, 0) and lib.freed == 3
        n_calls = len(lib.calls)
        with pytest.raises(ValueError, match="IVFSubset"):
            ivf.range_search(q, 0.0, params=faiss_compat.SearchParameters(sel=np.ones(4, bool)))
        other = IVFFlatIndex(D, 4)
        other._handle = ctypes.c_void_p(3)
        foreign = IVFSubset(other, 1, 1)
        with pytest.raises(ValueError, match="another index"):
            ivf.range_search(q, 0.0, params=foreign)
        with pytest.raises(ValueError, match="nprobe"):
            ivf.range_search(q, 0.0, params=faiss_compat.SearchParametersIVF(nprobe=0))
        with pytest.raises(ValueError):
            ivf.range_search(np.zeros((2, D - 1), np.float32), 0.0)
        lims, Dv, Iv = ivf.range_search(np.zeros((0, D), np.float32), 0.0)
        assert lims.tolist() == [0] and Dv.size == 0 and Iv.size == 0
        assert len(lib.calls) == n_calls
        sub._id = foreign._id = None
        other._handle = None
    finally:
        ivf._handle = None


def test_the_faiss_surface_inherits_range_search():
    for cls in (faiss_compat.IndexFlatIP, faiss_compat.IndexIVFFlat, faiss_compat.IndexScalarQuantizer):
        assert cls.range_search is FlatIPIndex.range_search
    assert "lims" in FlatIPIndex.range_search.__doc__ and "lims" in IVFFlatIndex.range_search.__doc__


# ---- the host plan ---------------------------------------------------------------------------------------------------------
def test_host_plan_under_sanitizers(tmp_path):
    """csrc/ls_range_plan.h in a plain host program with its own main (tests/range_plan_check.cpp), built with
    AddressSanitizer and UndefinedBehaviorSanitizer: n over {0, 1, 63, 64, 65, slab - 1, slab, slab + 1, 3 slab + 17}
    x G over {1, 3, 8} x 22 hit masks (none, all, slab edges, every other row, one slab full, NaN / -FLT_MAX / +inf
    rows, random densities; radii equal to and just below a present score, -inf, +inf, NaN) through a model of count ->
    offsets -> emit against a sequential threshold scan, and the split of 0..40 queries into groups."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host check of ls_range_plan.h"
    exe = tmp_path / "range_plan_check"
    p = subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", str(CSRC),
                        str(ROOT / "tests" / "range_plan_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.strip() == f"OK {9 * 3 * 22 + 41} cases"


# ---- the kernels' resources ------------------------------------------------------------------------------------------------
def test_range_kernels_resources(tmp_path):
    """ls_range_count_kernel, ls_range_offsets_kernel and ls_range_emit_kernel for gfx950: no scratch, no spilled VGPR
    (DESIGN.md section 4.10 has the table)."""
    usage = resource_usage("ls_range.hip", tmp_path)
    kernels = {n: u for n, u in usage.items() if "ls_range_" in n and "_kernel" in n}
    assert len(kernels) == 3, sorted(usage)
    for want in ("ls_range_count_kernel", "ls_range_offsets_kernel", "ls_range_emit_kernel"):
        assert any(want in n for n in kernels), (want, sorted(kernels))
    for n, u in sorted(kernels.items()):
        print(n, u)
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0, (n, u)
        assert u["VGPRs"] + u["AGPRs"] <= 128, (n, u)
