"""``ls_ivf_add`` without a GPU: the C ABI of include/leansearch_ivf_add.h is exported and bound, arguments are refused
before any device is touched, the host placement plan (csrc/ls_ivf_add_plan.h) equals a from-scratch counting sort
under sanitizers, ``IVFFlatIndex.add`` keeps its rules across the build. (The kernels' resources: tests/test_rows_cpu.py.)"""

import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from lean_explore_amd import native
from lean_explore_amd.ivf import IVFFlatIndex
from tests.test_ivf_cpu import declared

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "lean-explore_amd" / "csrc"
HEADER = ROOT / "include" / "leansearch_ivf_add.h"
INVALID = native.LS_ERR_INVALID_ARG


def test_header_symbols_exported_bound_and_disjoint():
    names = declared(HEADER)
    assert names == ["ls_ivf_add", "ls_ivf_add_last_kernel_ms"]
    assert sorted(native.IVF_ADD_SYMBOLS) == names
    for other in (native.SYMBOLS, native.IVF_SYMBOLS, native.IVF_SUBSET_SYMBOLS, native.IVF_BUILD_SYMBOLS,
                  native.IVF_BATCH_SYMBOLS, native.SQ8_SYMBOLS):
        assert not set(native.IVF_ADD_SYMBOLS) & set(other)
    raw = ctypes.CDLL(str(native.LIB_PATH))
    lib = native.load()
    for n in names:
        assert hasattr(raw, n), f"{n} declared in leansearch_ivf_add.h but not exported"
        assert getattr(lib, n).argtypes == native.IVF_ADD_SYMBOLS[n][1], n  # load() bound it


def test_a_null_handle_is_refused_with_a_message():
    lib = native.load()
    x = np.ones((2, 8), np.float32)
    a = np.zeros(2, np.int32)
    assert lib.ls_ivf_add(None, x.ctypes.data, 2, a.ctypes.data) == INVALID
    assert b"ls_ivf_add" in lib.ls_last_error() and b"null" in lib.ls_last_error()
    assert lib.ls_ivf_add(None, x.ctypes.data, 2, None) == INVALID
    assert lib.ls_ivf_add(None, None, 0, None) == INVALID  # (even an add of nothing needs a handle)
    assert lib.ls_ivf_add_last_kernel_ms(None, None, None) == INVALID
    assert b"ls_ivf_add_last_kernel_ms" in lib.ls_last_error()


def _trained(d=8, nlist=4, **kw):
    ix = IVFFlatIndex(d, nlist, **kw)
    ix.set_centroids(np.eye(nlist, d, dtype=np.float32))
    return ix


def test_a_wrong_shape_add_on_a_trained_index_raises():
    ix = _trained()
    for bad in (np.zeros((3, 7), np.float32), np.zeros(8, np.float32), np.zeros((2, 3, 8), np.float32)):
        with pytest.raises(ValueError, match="add expects"):
            ix.add(bad)
    with pytest.raises(ValueError, match="assign must name"):
        ix.add(np.zeros((3, 8), np.float32), assign=np.array([0, 1], np.int32))  # one list short
    with pytest.raises(ValueError, match="assign must name"):
        ix.add(np.zeros((2, 8), np.float32), assign=np.array([0, 4], np.int32))  # nlist is no list
    assert ix.ntotal == 0 and ix._handle is None
    with pytest.raises(ValueError, match="not trained"):
        IVFFlatIndex(8, 4).add(np.zeros((1, 8), np.float32))


def test_named_and_unnamed_lists_do_not_mix_before_or_after_the_build():
    x = np.ones((3, 8), np.float32)
    a = np.array([0, 1, 2], np.int32)
    # before the build: the buffered adds decide
    ix = _trained()
    ix.add(x, assign=a)
    with pytest.raises(ValueError, match="either every add"):
        ix.add(x)
    ix = _trained()
    ix.add(x)
    with pytest.raises(ValueError, match="either every add"):
        ix.add(x, assign=a)
    assert ix.ntotal == 3
    # after the build the buffers are gone: a flag that survives _ensure_built decides. (No device here: a handle that is
    # never dereferenced stands in for the built one - both refusals come before any library call.)
    for named in (True, False):
        ix = _trained()
        ix.add(x, assign=a if named else None)
        ix._names_lists, ix._pending, ix._assign = named, [], None  # what _ensure_built leaves behind ...
        ix._handle = ctypes.c_void_p(1)                              # ... with the handle
        try:
            with pytest.raises(ValueError, match="either every add"):
                ix.add(x, assign=None if named else a)
            with pytest.raises(ValueError, match="add expects"):
                ix.add(np.zeros((3, 7), np.float32), assign=a if named else None)
            if named:
                with pytest.raises(ValueError, match="assign must name"):
                    ix.add(x, assign=np.array([0, 1, 4], np.int32))
            ix.add(np.zeros((0, 8), np.float32), assign=np.zeros(0, np.int32) if named else None)  # nothing: no call
            assert ix.ntotal == 3
        finally:
            ix._handle = None


def test_ensure_built_records_whether_the_adds_named_their_lists(monkeypatch):
    """_ensure_built with the library's create stubbed out: the flag follows the buffered adds."""
    class Lib:
        def ls_ivf_create(self, out, *a):
            return 0

        def ls_ivf_destroy(self, h):
            return None

    monkeypatch.setattr(native, "load", lambda: Lib())
    x = np.ones((3, 8), np.float32)
    for named in (True, False):
        ix = _trained()
        ix.add(x, assign=np.array([0, 1, 2], np.int32) if named else None)
        ix._ensure_built()
        assert ix._names_lists is named and ix._assign is None and not ix._pending
        with pytest.raises(ValueError, match="either every add"):
            ix.add(x, assign=None if named else np.array([0, 1, 2], np.int32))
        ix._handle = None


def test_host_plan_under_sanitizers(tmp_path):
    """csrc/ls_ivf_add_plan.h in a plain host program with its own main (tests/ivf_add_plan_check.cpp), built with
    AddressSanitizer and UndefinedBehaviorSanitizer: the named edge cases, 400 random (old index, add) pairs against
    a from-scratch counting sort of the concatenated assignment, and the row mover's deal of (row, chunk) pairs (csrc/ls_rows_plan.h)."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host check of ls_ivf_add_plan.h"
    exe = tmp_path / "ivf_add_plan_check"
    p = subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", str(CSRC),
                        str(ROOT / "tests" / "ivf_add_plan_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.strip() == f"OK {11 + 400 + 12 * 6 * 2} cases"
