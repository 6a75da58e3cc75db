"""The small-batch setters of the C ABI on the smallest handles that build (64 rows, d = 16; IVF: nlist 4), against
tests/switch_ledger_c_parent.txt, recorded by this same file (run as a script, it prints the ledger) with the library of
the commit that file names. Every row is the return code, ls_l2_small_batch() afterwards and, where the code is not 0,
ls_last_error(): equality is exact. tests/switch_plan_check.cpp holds csrc/ls_switch_plan.h to the same rows on the CPU.

The second test flips a switch while two pipelined calls are unchecked (4096 x 64 integer-valued rows, as in
tests/test_scan_call_ledger_gpu.py): both calls must equal the numpy top-k, and the rise of the launch counters 11, 23, 34
and 36 over the flip and over the whole sequence must be the recorded one."""

import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from lean_explore_amd import native  # noqa: E402
from tests import helpers as H  # noqa: E402

pytestmark = pytest.mark.gpu

LEDGER = Path(__file__).resolve().parent / "switch_ledger_c_parent.txt"
FLAT_SETTERS = ("f16", "sq8", "subset", "l2")
# (kind, dtype, metric, placement)
FLAT_HANDLES = [("flat", "f32", "ip", "single"), ("flat", "f16", "ip", "single"), ("flat", "sq8", "ip", "single"),
                ("flat", "f32", "l2", "single"), ("flat", "f16", "l2", "single"),
                ("flat", "f32", "ip", "sharded"), ("flat", "f16", "ip", "sharded"),
                ("flat", "f32", "ip", "replicated"), ("flat", "f16", "ip", "replicated")]
IVF_HANDLES = [("ivf", "f32", "ip", "na"), ("ivf", "f16", "ip", "na"), ("ivf", "sq8", "ip", "na"),
               ("ivf", "f32", "l2", "na"), ("ivf", "f16", "l2", "na")]
FLIP_COUNTERS = (11, 23, 34, 36)
N, D, K = 4096, 64, 10


def _row(lib, h, setter, enable, flat_h):
    fn = lib.ls_ivf_set_small_batch if setter == "ivf" else getattr(lib, f"ls_set_{setter}_small_batch")
    rc = int(fn(h, enable))
    err = lib.ls_last_error().decode("utf-8", "replace") if rc else "-"
    return f"{rc}\t{int(lib.ls_l2_small_batch(flat_h))}\t{err}"


def setter_rows():
    from lean_explore_amd.index import FlatIPIndex
    from lean_explore_amd.ivf import IVFFlatIndex

    lib = native.load()
    rows = H.int_corpus(311, 64, 16)
    for kind, dtype, metric, place in FLAT_HANDLES:
        kw = {"single": {}, "sharded": {"devices": [0, 0]}, "replicated": {"devices": [0, 0], "replicate": True}}[place]
        ix = FlatIPIndex.from_array(rows, dtype=dtype, metric=metric, **kw)
        try:
            for setter in FLAT_SETTERS:
                for enable in (0, 1):
                    yield f"{kind} {dtype} {metric} {place} {setter} {enable}", _row(lib, ix._handle, setter, enable, ix._handle)
        finally:
            ix.close()
    for kind, dtype, metric, place in IVF_HANDLES:
        ivf = IVFFlatIndex(16, 4, dtype=dtype, metric=metric)
        ivf.set_centroids(rows[:4])
        ivf.add(rows)
        try:
            h = ivf._ensure_built()
            for enable in (0, 1):
                yield f"{kind} {dtype} {metric} {place} ivf {enable}", _row(lib, h, "ivf", enable, None)
        finally:
            ivf.close()
    for setter in FLAT_SETTERS + ("ivf",):
        for enable in (0, 1):
            yield f"null - - - {setter} {enable}", _row(lib, None, setter, enable, None)


def flip_rows():
    """f16 on an fp16 handle, sq8 on an sq8 handle, each off -> on and on -> off: (name, answer, the calls' results)."""
    import torch

    lib = native.load()
    c, q = H.int_corpus(211, N, D), H.int_corpus(212, 6, D)
    stream = torch.cuda.current_stream().cuda_stream
    for dtype, first in (("f16", 0), ("f16", 1), ("sq8", 0), ("sq8", 1)):
        setter = getattr(lib, f"ls_set_{dtype}_small_batch")
        h = ctypes.c_void_p()
        if dtype == "f16":
            native.check(lib.ls_create(ctypes.byref(h), c.ctypes.data, N, D, native.LS_DTYPE_F16, 0))
        else:
            step = np.ones(D, np.float32)  # (integer rows in -3..3: the codes are the rows)
            native.check(lib.ls_create_sq8(ctypes.byref(h), c.ctypes.data, N, D, step.ctypes.data, 0))
        try:
            native.check(setter(h, first))
            tq = torch.from_numpy(q.copy()).cuda()
            count = lambda: [int(lib.ls_debug_counter(h, w)) for w in FLIP_COUNTERS]  # noqa: E731
            start, outs = count(), []
            for call in range(2):
                Dd = torch.empty((3, K), dtype=torch.float32, device="cuda")
                Id = torch.empty((3, K), dtype=torch.int64, device="cuda")
                native.check(lib.ls_search_device(h, tq[3 * call:3 * call + 3].data_ptr(), 3, K, native.LS_FLAG_PIPELINE,
                                                  Dd.data_ptr(), Id.data_ptr(), stream))
                outs.append((Dd, Id))
            queued = count()
            native.check(setter(h, 1 - first))
            flipped = count()
            native.check(lib.ls_check(h, stream))
            torch.cuda.synchronize()
            end = count()
            rise = lambda a, b: " ".join(str(y - x) for x, y in zip(a, b))  # noqa: E731
            yield (f"flip {dtype} {first}->{1 - first}", f"queue {rise(start, queued)} | flip {rise(queued, flipped)} | all {rise(start, end)}",
                   [(Dd.cpu().numpy(), Id.cpu().numpy()) for Dd, Id in outs], (c, q))
        finally:
            lib.ls_destroy(h)


def ledger():
    out = {}
    for line in LEDGER.read_text().splitlines():
        if line and not line.startswith("#"):
            name, _, answer = line.partition("\t")
            out[name] = answer
    return out


def test_every_setter_answers_every_handle_as_the_parent_library_did():
    want, n = ledger(), 0
    for name, answer in setter_rows():
        print("LEDGER", name, answer)
        assert name in want, f"{name}: no row in {LEDGER.name}"
        assert answer == want[name], f"{name}: {answer!r}, the ledger says {want[name]!r}"
        n += 1
    assert n == 9 * 8 + 5 * 2 + 10


def test_a_switch_flipped_while_pipelined_calls_are_unchecked():
    want, n = ledger(), 0
    for name, answer, got, (c, q) in flip_rows():
        print("LEDGER", name, answer)
        s = q @ c.T  # (small integers: exact in any order, on fp16 rows and sq8 codes too)
        order = np.argsort(-s, axis=1, kind="stable")[:, :K]  # equal scores: the lower row first
        for call, (Dg, Ig) in enumerate(got):
            sl = slice(3 * call, 3 * call + 3)
            assert np.array_equal(Ig, order[sl]), f"{name}: call {call}: rows differ from the numpy top-k"
            assert np.array_equal(Dg, np.take_along_axis(s, order, axis=1)[sl]), f"{name}: call {call}: scores differ"
        assert name in want, f"{name}: no row in {LEDGER.name}"
        assert answer == want[name], f"{name}: counters {FLIP_COUNTERS} rose by {answer}, the recorded sequence by {want[name]}"
        n += 1
    assert n == 4


if __name__ == "__main__":
    for name, answer in setter_rows():
        print(f"{name}\t{answer}")
    for name, answer, _, _ in flip_rows():
        print(f"{name}\t{answer}")
