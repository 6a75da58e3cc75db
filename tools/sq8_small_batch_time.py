"""sq8 index, small batches: one ls_mq8 pass per 16 queries (ls_set_sq8_small_batch on) against the default service
of the same queries (one scan launch per query), same process, same index, option off and on interleaved.

Per (shape, nq) and mode it prints
  - kernel time per launch from the library's hipEvents (ls_set_profiling / ls_last_kernel_ms) times the scan-path
    launches one call needs = GPU time per call: mean over REPEATS bursts and [min .. max] of the bursts (the repeat
    spread). Off: nq launches. On: one per 16 queries, and a lone rest (nq = 1, 17, 33) on the scan kernel;
  - the stream time per call of the same bursts (torch events around CALLS pipelined calls + check): a cross-check
    that includes the selection launches and the gaps;
  - the p50 of the synchronous host call (FlatIPIndex.search, the reference's call) over HOST_CALLS calls.
For N = 200 k, d = 384 it also reports (no gate) the 16-query pass against the model
max(15.6 us of matrix time, bytes / 7.09 TB/s + 3.1 us).
The record goes to profiles/ab/sq8_small_batch.txt as well.

    python tools/sq8_small_batch_time.py        (SQ8SB_SHAPES=0,1 SQ8SB_NQS=1,2,4,8,16,32 SQ8SB_REPEATS=5)
"""
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from lean_explore_amd.index import FlatIPIndex
from tests import helpers as H

SHAPES = ((200_000, 384, 50), (200_000, 1024, 1000))  # C2, C2' (the reference's call shape)
if os.environ.get("SQ8SB_SHAPES"):
    SHAPES = tuple(SHAPES[int(i)] for i in os.environ["SQ8SB_SHAPES"].split(","))
NQS = tuple(int(x) for x in os.environ.get("SQ8SB_NQS", "1,2,4,8,16,32").split(","))
REPEATS = int(os.environ.get("SQ8SB_REPEATS", "5"))
CALLS = int(os.environ.get("SQ8SB_CALLS", "50"))
HOST_CALLS = int(os.environ.get("SQ8SB_HOST_CALLS", "100"))
OUT = ROOT / "profiles" / "ab" / "sq8_small_batch.txt"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def burst(ix, q, k):
    """CALLS pipelined calls: (kernel us per launch, launches per call, stream us per call)"""
    l0 = ix.debug_counter(11)
    ix.set_profiling(True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        ix.search_device(q, k, pipeline=True)
    ix.check()
    e1.record()
    e1.synchronize()
    ms, _ = ix.last_kernel_ms()
    ix.set_profiling(False)
    return ms * 1e3, (ix.debug_counter(11) - l0) / CALLS, e0.elapsed_time(e1) * 1e3 / CALLS


def host_p50(ix, qh, k):
    t = []
    for _ in range(HOST_CALLS):
        t0 = time.perf_counter()
        ix.search(qh, k)
        t.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(t))


def stats(v):
    return f"{np.mean(v):7.1f} [{np.min(v):6.1f} .. {np.max(v):6.1f}]"


say(f"device: {torch.cuda.get_device_name(0)}; {REPEATS} bursts of {CALLS} pipelined calls per mode, interleaved off / on; "
    f"host p50 over {HOST_CALLS} calls")
for (n, d, k) in SHAPES:
    c = H.gauss(1234, n, d)
    ix = FlatIPIndex.from_array(c, dtype="sq8")
    del c
    mb = n * ((d + 15) // 16 * 16) / 1e6
    hbm_us = mb * 1e6 / 7.09e12 * 1e6 + 3.1
    say(f"N={n} d={d} sq8 k={k}: codes {mb:.1f} MB, scan model bytes / 7.09 TB/s + 3.1 us = {hbm_us:.1f} us per pass")
    for nq in NQS:
        qh = H.gauss(5678, nq, d)
        q = torch.from_numpy(qh).cuda()
        scan_launches = {0: nq, 1: -(-nq // 16)}
        res, host = {0: [], 1: []}, {}
        for mode in (0, 1):  # warm-up, both modes
            ix.set_sq8_small_batch(bool(mode))
            for _ in range(20):
                ix.search_device(q, k, pipeline=True)
            ix.check()
        for _ in range(REPEATS):
            for mode in (0, 1):
                ix.set_sq8_small_batch(bool(mode))
                res[mode].append(burst(ix, q, k))
        for mode in (0, 1):
            ix.set_sq8_small_batch(bool(mode))
            host[mode] = host_p50(ix, qh, k)
        gpu = {}
        for mode in (0, 1):
            gpu[mode] = np.array([r[0] for r in res[mode]]) * scan_launches[mode]
            launches = float(np.mean([r[1] for r in res[mode]]))
            stream = np.array([r[2] for r in res[mode]])
            say(f"  nq={nq:2d} {'on ' if mode else 'off'}: kernel us/call {stats(gpu[mode])} ({scan_launches[mode]} scan-path "
                f"launch(es); {launches:.2f} launches/call)  stream us/call {stats(stream)}  host call p50 {host[mode]:7.1f} us")
        s_off, s_on = np.array([r[2] for r in res[0]]), np.array([r[2] for r in res[1]])
        say(f"  nq={nq:2d} on/off: kernel {np.mean(gpu[1]) / np.mean(gpu[0]):.2f} (worst burst on {np.max(gpu[1]):.1f} vs best "
            f"burst off {np.min(gpu[0]):.1f}), stream {np.mean(s_on) / np.mean(s_off):.2f} (worst on {np.max(s_on):.1f} vs best "
            f"off {np.min(s_off):.1f}), host p50 {host[1] / host[0]:.2f}")
        if nq == 16 and d == 384:
            model = max(15.6, hbm_us)
            say(f"  nq=16 on: {np.mean(gpu[1]):.1f} us = {np.mean(gpu[1]) / model:.2f} x max(15.6 us matrix, {hbm_us:.1f} us scan model)")
    ix.close()
OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text("\n".join(lines) + "\n")
