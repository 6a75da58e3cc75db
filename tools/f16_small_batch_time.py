"""fp16 index, small batches: one ls_mq16 pass (ls_set_f16_small_batch on) against the default service of the same
queries (VALU scan groups of 8 / 4 / 1; 32 queries: the batched path), same process, same index, interleaved.

Per (shape, nq) and mode it prints
  - kernel time per launch from the library's hipEvents (ls_set_profiling / ls_last_kernel_ms), times the launches
    one call needs = GPU time per call, mean over REPEATS bursts and [min .. max] of the bursts (the repeat spread);
  - the stream time per call of the same bursts (torch events around CALLS pipelined calls + check): a cross-check
    that includes the selection launches and gaps;
  - corpus bytes / kernel time against 8 TB/s (HBM3E peak) for the one-pass mode.
153.6 MB (N = 200 k, d = 384) fits the 256 MB Infinity Cache - back-to-back passes over it are served from there,
which is why the fraction can pass 1 - 409.6 MB (d = 1024) and 768 MB (N = 1 M, d = 384) do not.

    python tools/f16_small_batch_time.py            (F16SB_SHAPES=0,1,2 F16SB_NQS=1,2,4,8,16,32 F16SB_REPEATS=7)
    F16SB_BASELINE_ONLY=1 LEANSEARCH_LIB=<a build without the option> python tools/f16_small_batch_time.py
        the default service alone, also through a library built before the option existed: its numbers should
        agree with this build's "off" lines to within the repeat spread.
"""
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

from lean_explore_amd import native
from lean_explore_amd.index import FlatIPIndex
from tests import helpers as H

SHAPES = ((200_000, 384, 50, (1, 2, 4, 8, 16, 32)), (200_000, 1024, 1000, (1, 2, 4, 8, 16, 32)),
          (1_000_000, 384, 50, (16,)))
if os.environ.get("F16SB_SHAPES"):
    SHAPES = tuple(SHAPES[int(i)] for i in os.environ["F16SB_SHAPES"].split(","))
NQS = tuple(int(x) for x in os.environ["F16SB_NQS"].split(",")) if os.environ.get("F16SB_NQS") else None
REPEATS = int(os.environ.get("F16SB_REPEATS", "7"))
CALLS = int(os.environ.get("F16SB_CALLS", "100"))
PEAK = 8.0e12
BASELINE_ONLY = os.environ.get("F16SB_BASELINE_ONLY", "0") == "1"
MODES = (0,) if BASELINE_ONLY else (0, 1)
if BASELINE_ONLY:
    native.SYMBOLS.pop("ls_set_f16_small_batch", None)  # (an older build does not export it; never called here)


def set_mode(ix, mode):
    if not BASELINE_ONLY:
        ix.set_f16_small_batch(bool(mode))


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


def stats(v):
    return f"{np.mean(v):7.1f} [{np.min(v):6.1f} .. {np.max(v):6.1f}]"


print(f"device: {torch.cuda.get_device_name(0)}; library {native.LIB_PATH.name if BASELINE_ONLY else 'of this tree'}; "
      f"{REPEATS} bursts of {CALLS} pipelined calls per mode, " + ("option off only" if BASELINE_ONLY else "interleaved off / on"),
      flush=True)
for (n, d, k, nqs) in SHAPES:
    c = H.gauss(1234, n, d)
    ix = FlatIPIndex.from_array(c, dtype="f16")
    del c
    mb = n * ((d * 2 + 255) // 256 * 256) / 1e6
    print(f"N={n} d={d} fp16 k={k}: corpus {mb:.1f} MB ({'fits' if mb <= 256 else 'does not fit'} the 256 MB Infinity "
          f"Cache), {mb * 1e6 / PEAK * 1e6:.1f} us at 8 TB/s", flush=True)
    on_time = {}
    for nq in (NQS or nqs):
        q = torch.from_numpy(H.gauss(5678, nq, d)).cuda()
        groups = {0: 1 if nq <= 4 else -(-nq // 8), 1: 1}  # scan launches per call (off: groups of 8 / 4 / 1)
        res = {0: [], 1: []}
        for mode in MODES:  # warm-up, both modes
            set_mode(ix, mode)
            for _ in range(30):
                ix.search_device(q, k, pipeline=True)
            ix.check()
        for _ in range(REPEATS):
            for mode in MODES:
                set_mode(ix, mode)
                res[mode].append(burst(ix, q, k))
        for mode in MODES:
            per_launch = np.array([r[0] for r in res[mode]])
            launches = float(np.mean([r[1] for r in res[mode]]))
            stream = np.array([r[2] for r in res[mode]])
            batched = mode == 0 and nq > 16  # (the speculative batched path: its launches are not scan launches)
            gpu = per_launch * (1 if batched else groups[mode])
            line = (f"  nq={nq:2d} {'on ' if mode else 'off'}: kernel us/{'launch' if batched else 'call'} {stats(gpu)}"
                    f" ({'batched path: mean over its launches, compare the stream time' if batched else str(groups[mode]) + ' scan launch(es)'};"
                    f" {launches:.2f} launches/call)  stream us/call {stats(stream)}")
            if mode:
                on_time[nq] = float(np.mean(gpu))
                line += f"  {mb * 1e6 / (np.mean(gpu) * 1e-6) / PEAK:.2f} of 8 TB/s"
            print(line, flush=True)
        if BASELINE_ONLY:
            continue
        off = np.array([r[0] for r in res[0]]) * groups[0]
        on = np.array([r[0] for r in res[1]]) * groups[1]
        s_off, s_on = np.array([r[2] for r in res[0]]), np.array([r[2] for r in res[1]])
        kern = (f"kernel {np.mean(on) / np.mean(off):.2f} (worst burst on {np.max(on):.1f} vs best burst off {np.min(off):.1f}), "
                if nq <= 16 else "")
        print(f"  nq={nq:2d} on/off: {kern}stream {np.mean(s_on) / np.mean(s_off):.2f} (worst on {np.max(s_on):.1f} vs best off "
              f"{np.min(s_off):.1f})", flush=True)
    if 16 in on_time and 2 in on_time:
        print(f"  time(nq=16) / time(nq=2), option on: {on_time[16] / on_time[2]:.2f}", flush=True)
    ix.close()
