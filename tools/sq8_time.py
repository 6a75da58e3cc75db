"""sq8 index against the fp32 and fp16 indexes of the same rows: the single-query scan launch, one process, interleaved.

Per shape and dtype it prints
  - kernel time per scan launch from the library's hipEvents (ls_set_profiling / ls_last_kernel_ms) over bursts of
    pipelined single-query device calls: mean over REPEATS bursts and [min .. max] of the bursts;
  - the stream time per step of the same bursts (torch events around CALLS pipelined calls + check);
  - the synchronous host call (ls_search, one query): p50 of CALLS calls per burst;
  - each launch against the scan's model, stored bytes / 7.09 TB/s + 3.1 us, and the sq8 / fp16 and sq8 / fp32 ratios.
The condition DESIGN.md 4.9 quotes: at C2M (1 M x 384) the sq8 launch is no slower than the fp16 launch of the same run.

    python tools/sq8_time.py            (SQ8_SHAPES=0,1,2 SQ8_REPEATS=5 SQ8_CALLS=100; writes profiles/ab/sq8_scan.txt)
"""
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from lean_explore_amd import native
from lean_explore_amd.index import FlatIPIndex
from tests import helpers as H

SHAPES = (("C2", 200_000, 384, 50), ("C2'", 200_000, 1024, 1000), ("C2M", 1_000_000, 384, 50))
if os.environ.get("SQ8_SHAPES"):
    SHAPES = tuple(SHAPES[int(i)] for i in os.environ["SQ8_SHAPES"].split(","))
REPEATS = int(os.environ.get("SQ8_REPEATS", "5"))
CALLS = int(os.environ.get("SQ8_CALLS", "100"))
DTYPES = ("f32", "f16", "sq8")
ELEM = {"f32": 4, "f16": 2, "sq8": 1}
OUT = ROOT / "profiles" / "ab" / "sq8_scan.txt"
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def model_us(nbytes):
    return nbytes / 7.09e12 * 1e6 + 3.1


def burst(ix, q_dev, q_host, k):
    """(kernel us per launch, stream us per step, host p50 us) of CALLS single-query calls each"""
    ix.set_profiling(True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        ix.search_device(q_dev, k, pipeline=True)
    ix.check()
    e1.record()
    e1.synchronize()
    ms, _ = ix.last_kernel_ms()
    ix.set_profiling(False)
    host = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        ix.search(q_host, k)
        host.append((time.perf_counter() - t0) * 1e6)
    return ms * 1e3, e0.elapsed_time(e1) * 1e3 / CALLS, float(np.median(host))


def stats(v):
    return f"{np.mean(v):7.1f} [{np.min(v):6.1f} .. {np.max(v):6.1f}]"


say(f"device: {torch.cuda.get_device_name(0)}; {native.version()}; {REPEATS} bursts of {CALLS} calls per dtype, interleaved")
for name, n, d, k in SHAPES:
    c = H.gauss(1234, n, d)
    idx = {dt: FlatIPIndex.from_array(c, dtype=dt) for dt in DTYPES}
    del c
    qh = H.gauss(5678, 1, d)
    qd = torch.from_numpy(qh).cuda()
    chunks = {dt: -(-d * ELEM[dt] // 16) for dt in DTYPES}
    nbytes = {}
    for dt in DTYPES:  # stored row: chunks padded to the geometry (sq8: ls_sq8_geom; f32 / f16: multiples of 16 chunks)
        if dt == "sq8":
            import ctypes

            cc = ctypes.c_int32()
            native.check(native.load().ls_sq8_geom(d, ctypes.byref(cc), None, None))
            nbytes[dt] = n * cc.value * 16
        else:
            nbytes[dt] = n * (-(-chunks[dt] // 16) * 16) * 16
    say(f"{name}: N={n} d={d} k={k}; stored MB " + ", ".join(f"{dt} {nbytes[dt] / 1e6:.1f}" for dt in DTYPES))
    res = {dt: [] for dt in DTYPES}
    for dt in DTYPES:  # warm-up
        for _ in range(30):
            idx[dt].search_device(qd, k, pipeline=True)
        idx[dt].check()
        idx[dt].search(qh, k)
    for _ in range(REPEATS):
        for dt in DTYPES:
            res[dt].append(burst(idx[dt], qd, qh, k))
    kern = {}
    for dt in DTYPES:
        kv = np.array([r[0] for r in res[dt]])
        kern[dt] = kv
        say(f"  {dt}: kernel us/launch {stats(kv)}  model {model_us(nbytes[dt]):6.1f} (x{np.mean(kv) / model_us(nbytes[dt]):.2f})"
            f"  {nbytes[dt] / (np.mean(kv) * 1e-6) / 1e12:.2f} TB/s  pipelined us/step {stats([r[1] for r in res[dt]])}"
            f"  host call p50 us {stats([r[2] for r in res[dt]])}")
    say(f"  sq8 / f16 kernel {np.mean(kern['sq8']) / np.mean(kern['f16']):.3f} (worst sq8 burst {np.max(kern['sq8']):.1f} vs best "
        f"f16 burst {np.min(kern['f16']):.1f});  sq8 / f32 kernel {np.mean(kern['sq8']) / np.mean(kern['f32']):.3f};  "
        f"model sq8 / f16 {model_us(nbytes['sq8']) / model_us(nbytes['f16']):.2f}")
    if name == "C2M":
        ok = np.mean(kern["sq8"]) <= np.mean(kern["f16"])
        say(f"  CONDITION (C2M: sq8 launch no slower than the fp16 launch of the same run): {'holds' if ok else 'FAILS'}")
    for ix in idx.values():
        ix.close()
OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text("\n".join(lines) + "\n")
print(f"wrote {OUT}")
