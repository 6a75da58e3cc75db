"""Several L2 queries per corpus pass (include/leansearch_l2_batch.h) without a GPU: the header and the
binding, the refusals that come before any device check, the Python keyword, and the query groups of the scan-call plan
(tests/l2_batch_plan_check.cpp, a stand-alone host program over the plan headers)."""

import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from lean_explore_amd import faiss_compat, native
from lean_explore_amd.index import FlatIPIndex, FlatL2Index

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "lean-explore_amd" / "csrc"
HEADER = ROOT / "include" / "leansearch_l2_batch.h"


def test_header_declares_exactly_the_option_and_it_is_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ls_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(native.L2_BATCH_SYMBOLS) == ["ls_l2_small_batch", "ls_set_l2_small_batch"]
    assert not set(native.L2_BATCH_SYMBOLS) & (set(native.SYMBOLS) | set(native.L2_SYMBOLS) | set(native.IVF_L2_SYMBOLS))
    raw = ctypes.CDLL(str(native.LIB_PATH))
    lib = native.load()  # load() bound them
    for n in names:
        assert hasattr(raw, n), f"{n} is not exported"
        assert getattr(lib, n).argtypes == native.L2_BATCH_SYMBOLS[n][1]
        assert getattr(lib, n).restype == native.L2_BATCH_SYMBOLS[n][0]
    assert lib.ls_set_l2_small_batch.argtypes == [ctypes.c_void_p, ctypes.c_int32]
    assert lib.ls_l2_small_batch.argtypes == [ctypes.c_void_p] and lib.ls_l2_small_batch.restype == ctypes.c_int32


def test_null_handle_is_an_argument_error():
    raw = ctypes.CDLL(str(native.LIB_PATH))
    raw.ls_set_l2_small_batch.restype = ctypes.c_int
    raw.ls_set_l2_small_batch.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    raw.ls_l2_small_batch.restype = ctypes.c_int32
    raw.ls_l2_small_batch.argtypes = [ctypes.c_void_p]
    raw.ls_last_error.restype = ctypes.c_char_p
    for enable in (0, 1):
        assert raw.ls_set_l2_small_batch(None, enable) == native.LS_ERR_INVALID_ARG
        assert b"ls_set_l2_small_batch" in raw.ls_last_error() and b"null" in raw.ls_last_error()
    assert raw.ls_l2_small_batch(None) == 0
    assert native.load().ls_debug_counter(None, 38) == -1


def test_the_keyword_needs_an_l2_index_of_f32_or_f16_rows_on_one_device():
    with pytest.raises(ValueError, match="l2_small_batch"):
        FlatIPIndex(64, metric="ip", l2_small_batch=True)
    with pytest.raises(ValueError, match="l2_small_batch"):
        FlatIPIndex(64, l2_small_batch=True)  # (the default metric is the inner product)
    with pytest.raises(ValueError, match="l2_small_batch"):
        FlatIPIndex(64, dtype="sq8", l2_small_batch=True)
    with pytest.raises(ValueError):
        FlatIPIndex(64, metric="l2", dtype="sq8", l2_small_batch=True)
    with pytest.raises(ValueError):
        FlatIPIndex(64, metric="l2", devices=[0, 1], l2_small_batch=True)
    with pytest.raises(ValueError):
        FlatL2Index(64, devices=[0, 1], l2_small_batch=True)
    with pytest.raises(ValueError, match="l2_small_batch"):
        FlatIPIndex(64, devices=[0, 1], l2_small_batch=True)
    with pytest.raises(ValueError, match="l2_small_batch"):
        faiss_compat.IndexFlat(64, faiss_compat.METRIC_INNER_PRODUCT, l2_small_batch=True)
    ip = FlatIPIndex(64)
    with pytest.raises(ValueError, match="l2_small_batch"):
        ip.set_l2_small_batch(True)
    with pytest.raises(ValueError, match="l2_small_batch"):
        ip.l2_small_batch = True
    ip.set_l2_small_batch(False)  # switching it off is always allowed
    assert ip.l2_small_batch is False and ip._handle is None


def test_keyword_property_and_setter_before_any_device_is_touched(tmp_path):
    for dtype in ("f32", "f16"):
        for ix in (FlatL2Index(64, dtype=dtype, l2_small_batch=True),
                   FlatIPIndex(64, dtype=dtype, metric="l2", l2_small_batch=True),
                   faiss_compat.IndexFlatL2(64, dtype=dtype, l2_small_batch=True),
                   faiss_compat.IndexFlat(64, faiss_compat.METRIC_L2, dtype=dtype, l2_small_batch=True)):
            assert ix.l2_small_batch is True and ix.metric == "l2" and ix._handle is None
            ix.l2_small_batch = False
            assert ix.l2_small_batch is False and ix._handle is None
            ix.set_l2_small_batch(True)
            assert ix.l2_small_batch is True and ix._handle is None
    assert FlatL2Index(64).l2_small_batch is False and faiss_compat.IndexFlatL2(64).l2_small_batch is False
    assert faiss_compat.IndexFlat(64).l2_small_batch is False
    # read_index: the keyword of an IxF2 file, refused for every other container
    import numpy as np

    x = np.arange(5 * 8, dtype=np.float32).reshape(5, 8)
    l2 = faiss_compat.IndexFlatL2(8)
    l2.add(x)
    p = tmp_path / "l2.index"
    faiss_compat.write_index(l2, p)  # (nothing was searched: the rows are still on the host)
    back = faiss_compat.read_index(p, l2_small_batch=True)
    assert isinstance(back, faiss_compat.IndexFlatL2) and back.l2_small_batch is True and back.ntotal == 5
    assert back._handle is None and faiss_compat.read_index(p).l2_small_batch is False
    ip = faiss_compat.IndexFlatIP(8)
    ip.add(x)
    p2 = tmp_path / "ip.index"
    faiss_compat.write_index(ip, p2)
    with pytest.raises(ValueError, match="l2_small_batch"):
        faiss_compat.read_index(p2, l2_small_batch=True)


def test_query_groups_of_the_scan_call_plan_under_sanitizers(tmp_path):
    """tests/l2_batch_plan_check.cpp: with the new field on an L2 handle's launches carry 8 / 4 / 1 queries (left =
    1..17, kind LS_K_SCAN), with it off one each, and for every input that is not such a handle the call plan, the
    launch shapes and the launch plans are the same whether the field is set or not."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host check of ls_scan_call_plan.h"
    exe = tmp_path / "l2_batch_plan_check"
    p = subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", str(CSRC), str(ROOT / "tests" / "l2_batch_plan_check.cpp"),
                        "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    last = p.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) >= 100_000, p.stdout[-500:]
