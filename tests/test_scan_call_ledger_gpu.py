"""Every way a call reaches the scan path (csrc/ls_api.hip, scan_search_on_stream), through the public C ABI alone:
the results against a numpy top-k in the project's total order (score descending, row ascending), and the launches the
call queued - the exact rise of debug counters 10, 11, 23, 34, 35 and 37 - against tests/scan_call_ledger_parent.txt,
recorded by this same file at the commit that file names. These are launch counts: equality, no margin. (Counters 20,
25 and 27 depend on timing - a riding selection may give up waiting - and are not compared.)

4096 rows x d = 64 is the smallest index the small-batch passes serve; the corpus and the queries are small integers, so
every summation order gives the same bits, on fp32 and on fp16 rows."""

import ctypes
from pathlib import Path

import numpy as np
import pytest

from lean_explore_amd import native
from tests import helpers as H

pytestmark = pytest.mark.gpu

N, D, K = 4096, 64, 10
COUNTERS = (10, 11, 23, 34, 35, 37)
LEDGER = Path(__file__).resolve().parent / "scan_call_ledger_parent.txt"
DTYPES = {"f32": (native.LS_DTYPE_F32, False), "f16": (native.LS_DTYPE_F16, False),
          "f16sb": (native.LS_DTYPE_F16, True)}  # (f16sb: with ls_set_f16_small_batch)
CASES = ([("search", nq) for nq in (1, 3)] + [("device", nq) for nq in (1, 3, 17)] +
         [("async", nq) for nq in (1, 3)] + [("pipeline", nq) for nq in (1, 3)] +
         [("inorder", nq) for nq in (1, 3)] + [("lanes", nq) for nq in (1, 3)] +
         [("subset", 3), ("subset_small_batch", 3)])

_ref = {}


def inputs():
    """The corpus, 34 queries and their top-K lists, computed once and never changed."""
    if not _ref:
        c, q = H.int_corpus(211, N, D), H.int_corpus(212, 34, D)
        s = q @ c.T  # (small integers: exact in fp32 in any order, and every entry is an fp16 number)
        order = np.argsort(-s, axis=1, kind="stable")[:, :K]  # equal scores: the lower row first
        _ref.update(c=c, q=q, D=np.take_along_axis(s, order, axis=1), I=order.astype(np.int64))
        for a in _ref.values():
            a.setflags(write=False)
    return _ref


def ledger():
    rows = {}
    for line in LEDGER.read_text().splitlines():
        if line and not line.startswith("#"):
            name, *vals = line.split()
            rows[name] = tuple(int(v) for v in vals)
    return rows


def check(rc):
    if rc:
        native.check(rc)


@pytest.mark.parametrize("entry, nq", CASES, ids=[f"{e}-{n}" for e, n in CASES])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_results_and_launch_ledger(dtype, entry, nq):
    import torch

    lib, R = native.load(), inputs()
    code, small_batch = DTYPES[dtype]
    h = ctypes.c_void_p()
    check(lib.ls_create(ctypes.byref(h), R["c"].ctypes.data, N, D, code, 0))
    try:
        if small_batch:
            check(lib.ls_set_f16_small_batch(h, 1))
        sid = None
        if entry.startswith("subset"):
            bm = np.full(N // 8, 0xFF, np.uint8)  # every row: the smallest subset a pass serves
            i32, i64 = ctypes.c_int32(), ctypes.c_int64()
            check(lib.ls_subset_create(h, bm.ctypes.data, bm.size, ctypes.byref(i32), ctypes.byref(i64)))
            assert i64.value == N
            sid = i32.value
        setter_rc = 0
        if entry == "subset_small_batch":  # (fp32 rows only: on fp16 rows the setter refuses and the call is the plain one)
            setter_rc = lib.ls_set_subset_small_batch(h, 1)
            assert (setter_rc == 0) == (dtype == "f32")
        if entry == "lanes":
            check(lib.ls_debug_option(h, 24, 2))
        stream = torch.cuda.current_stream().cuda_stream
        before = [lib.ls_debug_counter(h, c) for c in COUNTERS]
        got = []  # (first query, scores, rows) per call
        if entry == "search" or sid is not None:
            q = np.ascontiguousarray(R["q"][:nq])
            Dh, Ih = np.empty((nq, K), np.float32), np.empty((nq, K), np.int64)
            if sid is None:
                check(lib.ls_search(h, q.ctypes.data, nq, K, 0, Dh.ctypes.data, Ih.ctypes.data))
            else:
                check(lib.ls_search_subset(h, sid, q.ctypes.data, nq, K, 0, Dh.ctypes.data, Ih.ctypes.data))
            got.append((0, Dh, Ih))
        else:
            flags = {"device": 0, "async": native.LS_FLAG_ASYNC, "pipeline": native.LS_FLAG_PIPELINE,
                     "lanes": native.LS_FLAG_PIPELINE, "inorder": native.LS_FLAG_PIPELINE | native.LS_FLAG_INORDER}[entry]
            tq = torch.from_numpy(R["q"].copy()).cuda()
            outs = []
            for call in range(2 if flags & native.LS_FLAG_PIPELINE else 1):
                q0 = call * nq
                Dd = torch.empty((nq, K), dtype=torch.float32, device="cuda")
                Id = torch.empty((nq, K), dtype=torch.int64, device="cuda")
                check(lib.ls_search_device(h, tq[q0:q0 + nq].data_ptr(), nq, K, flags, Dd.data_ptr(), Id.data_ptr(), stream))
                outs.append((q0, Dd, Id))
            if flags & native.LS_FLAG_PIPELINE:
                check(lib.ls_check(h, stream))
            torch.cuda.synchronize()
            got = [(q0, Dd.cpu().numpy(), Id.cpu().numpy()) for q0, Dd, Id in outs]
        rise = tuple(int(lib.ls_debug_counter(h, c) - b) for c, b in zip(COUNTERS, before))
        name = f"{dtype}/{entry}-{nq}"
        print("LEDGER", name, *rise)
        for q0, Dg, Ig in got:
            assert np.array_equal(Ig, R["I"][q0:q0 + nq]), f"{name}: rows differ from the numpy top-k"
            assert np.array_equal(Dg, R["D"][q0:q0 + nq]), f"{name}: scores differ from the numpy top-k"
        want = ledger().get(name)
        assert want is not None, f"{name}: no row in {LEDGER.name}"
        assert rise == want, f"{name}: counters {COUNTERS} rose by {rise}, the recorded call by {want}"
    finally:
        lib.ls_destroy(h)
