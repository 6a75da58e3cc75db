"""Subset search, small batches: one pass per group of 2..16 queries (ls_set_subset_small_batch on) against the default
service of the same call (one row-list scan launch + one finalize launch per query), same process, same index, option
off and on interleaved in bursts.

Per (shape, subset, nq) and mode it prints
  - the call's kernel time: the library's own event pairs (ls_set_profiling / ls_last_kernel_ms: one pair around every
    scan + finalize, or pass + finalize), summed per call; mean over REPEATS bursts of CALLS calls and [min .. max] of
    the bursts (the burst spread);
  - the p50 of the synchronous host call (FlatIPIndex.search with a selector) over HOST_CALLS calls, profiling off.
Shapes: C2 (200 k x 384, k = 50) and C2' (200 k x 1024, k = 1000). Subsets: all rows, a random 50 / 10 / 1 %, one
contiguous 10 % block. nq: 1 / 2 / 4 / 8 / 16 / 32.

Gates (printed as PASS / FAIL; the exit code is 1 if one fails):
  - random 10 % subset, 16 queries, both shapes: the WORST burst with the option on is below the BEST burst with it off;
  - nq = 1 (the same launches either way): the modes' means differ by no more than the bursts' own min-to-max spread.
Reported, not gated: the all-rows 16-query pass against a plain 16-query ls_mq call that writes its score vectors
(LS_FLAG_ASYNC alone: the library's event pair holds its pass only, so the pass + finalize of one call is also taken
between two stream events - what a subset call's pair holds), and the 1 % subset.
The record goes to profiles/ab/subset_small_batch.txt as well.

    python tools/subset_small_batch_time.py     (SSB_SHAPES=0,1 SSB_NQS=1,2,4,8,16,32 SSB_REPEATS=5 SSB_CALLS=20)
"""
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from lean_explore_amd import faiss_compat as fc
from lean_explore_amd.index import FlatIPIndex
from tests import helpers as H

SHAPES = ((200_000, 384, 50), (200_000, 1024, 1000))  # C2, C2' (the reference's call shape)
if os.environ.get("SSB_SHAPES"):
    SHAPES = tuple(SHAPES[int(i)] for i in os.environ["SSB_SHAPES"].split(","))
NQS = tuple(int(x) for x in os.environ.get("SSB_NQS", "1,2,4,8,16,32").split(","))
REPEATS = int(os.environ.get("SSB_REPEATS", "5"))
CALLS = int(os.environ.get("SSB_CALLS", "20"))
HOST_CALLS = int(os.environ.get("SSB_HOST_CALLS", "60"))
OUT = ROOT / "profiles" / "ab" / "subset_small_batch.txt"
lines, failed = [], []


def say(s):
    print(s, flush=True)
    lines.append(s)


def pairs(nq, mode, served):
    """event pairs one call records: one per query, or - option on and the plan serves the subset - one per group of
    2..16 queries plus one for a lone rest"""
    if not (mode and served):
        return nq
    return nq // 16 + (1 if nq % 16 else 0)


def burst(ix, q, k, sub, npairs):
    """CALLS synchronous calls: mean kernel us per call (sum of the call's event pairs)"""
    par = fc.SearchParameters(sel=sub)
    ix.set_profiling(True)
    tot = 0.0
    for _ in range(CALLS):
        ix.search(q, k, params=par)
        ms, _ = ix.last_kernel_ms()  # (mean over the call's pairs; reading it starts the next call's record)
        tot += ms * 1e3 * npairs
    ix.set_profiling(False)
    return tot / CALLS


def host_p50(ix, q, k, sub):
    par = fc.SearchParameters(sel=sub)
    t = []
    for _ in range(HOST_CALLS):
        t0 = time.perf_counter()
        ix.search(q, k, params=par)
        t.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(t))


def plain_burst(ix, q, k):
    """CALLS plain 16-query ls_mq calls that keep their score vectors: kernel us of the pass"""
    ix.set_profiling(True)
    for _ in range(CALLS):
        ix.search_device(q, k, asynchronous=True)
    torch.cuda.synchronize()
    ms, _ = ix.last_kernel_ms()
    ix.set_profiling(False)
    return ms * 1e3


def plain_total(ix, q, k):
    """the same calls, one at a time between two stream events: the pass AND the finalize launch behind it, us per call
    - what a subset call's event pair holds"""
    tot = 0.0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(CALLS):
        torch.cuda.synchronize()
        e0.record()
        ix.search_device(q, k, asynchronous=True)
        e1.record()
        e1.synchronize()
        tot += e0.elapsed_time(e1) * 1e3
    return tot / CALLS


def stats(v):
    return f"{np.mean(v):8.1f} [{np.min(v):7.1f} .. {np.max(v):7.1f}]"


def gate(name, ok, detail):
    say(f"  GATE {name}: {'PASS' if ok else 'FAIL'} ({detail})")
    if not ok:
        failed.append(name)


say(f"device: {torch.cuda.get_device_name(0)}; {REPEATS} bursts of {CALLS} synchronous calls per mode, interleaved off / on; "
    f"host p50 over {HOST_CALLS} calls")
for (n, d, k) in SHAPES:
    c = H.gauss(1234, n, d)
    ix = FlatIPIndex.from_array(c)
    del c
    rng = np.random.default_rng(99)
    subsets = [("all rows", np.ones(n, bool))]
    for frac in (0.5, 0.1, 0.01):
        subsets.append((f"random {frac:g}", rng.random(n) < frac))
    block = np.zeros(n, bool)
    block[n // 3: n // 3 + n // 10] = True
    subsets.append(("block 0.1", block))
    say(f"N={n} d={d} f32 k={k}: scan model per selected row set = bytes / 7.09 TB/s + 3.1 us")
    for name, mask in subsets:
        sub = ix.subset(mask)
        m = sub.rows
        model = m * d * 4 / 7.09e12 * 1e6 + 3.1
        say(f" subset {name}: m={m} ({m * d * 4 / 1e6:.1f} MB, scan model {model:.1f} us per pass over it)")
        for nq in NQS:
            q = H.gauss(5678, nq, d)
            ix.set_subset_small_batch(True)
            p0 = ix.debug_counter(37)
            ix.search(q, k, params=fc.SearchParameters(sel=sub))
            served = ix.debug_counter(37) > p0 or nq == 1  # (nq = 1 never takes a pass: one pair either way)
            res, host = {0: [], 1: []}, {}
            for mode in (0, 1):  # warm-up, both modes
                ix.set_subset_small_batch(bool(mode))
                for _ in range(5):
                    ix.search(q, k, params=fc.SearchParameters(sel=sub))
            for _ in range(REPEATS):
                for mode in (0, 1):
                    ix.set_subset_small_batch(bool(mode))
                    res[mode].append(burst(ix, q, k, sub, pairs(nq, mode, served)))
            for mode in (0, 1):
                ix.set_subset_small_batch(bool(mode))
                host[mode] = host_p50(ix, q, k, sub)
            g = {mode: np.array(res[mode]) for mode in (0, 1)}
            for mode in (0, 1):
                say(f"  nq={nq:2d} {'on ' if mode else 'off'}: kernel us/call {stats(g[mode])} ({pairs(nq, mode, served)} "
                    f"event pair(s))  host call p50 {host[mode]:8.1f} us")
            say(f"  nq={nq:2d} on/off: kernel {np.mean(g[1]) / np.mean(g[0]):.3f} (worst burst on {np.max(g[1]):.1f} vs best "
                f"burst off {np.min(g[0]):.1f}), host p50 {host[1] / host[0]:.3f}"
                + ("" if served else "  [the plan declines this (subset, k): the same launches either way]"))
            if name == "random 0.1" and nq == 16:
                gate(f"d={d} random 10 % nq=16 worst-on < best-off", np.max(g[1]) < np.min(g[0]),
                     f"{np.max(g[1]):.1f} vs {np.min(g[0]):.1f} us")
            if nq == 1:
                spread = max(np.max(g[0]) - np.min(g[0]), np.max(g[1]) - np.min(g[1]))
                gate(f"d={d} {name} nq=1 on == off within the burst spread", abs(np.mean(g[1]) - np.mean(g[0])) <= spread,
                     f"|{np.mean(g[1]):.1f} - {np.mean(g[0]):.1f}| vs spread {spread:.1f} us")
            if name == "all rows" and nq == 16:
                qd = torch.from_numpy(q).cuda()
                for _ in range(5):
                    ix.search_device(qd, k, asynchronous=True)
                torch.cuda.synchronize()
                pl = np.array([plain_burst(ix, qd, k) for _ in range(REPEATS)])
                pt = np.array([plain_total(ix, qd, k) for _ in range(REPEATS)])
                pspread = (np.max(pt) - np.min(pt)) / np.mean(pt)
                say(f"  nq=16 all rows: subset pass + finalize {np.mean(g[1]):.1f} us; plain ls_mq call with score vectors: pass "
                    f"alone {stats(pl)} us, pass + finalize {stats(pt)} us: ratio to the latter {np.mean(g[1]) / np.mean(pt):.3f} "
                    f"(plain burst spread {100 * pspread:.1f} %)")
        sub.close()
    ix.close()
OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text("\n".join(lines) + "\n")
if failed:
    say(f"FAILED gates: {failed}")
    sys.exit(1)
