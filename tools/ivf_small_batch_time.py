"""IVF search, small batches: one pass per group of 2..16 queries over the union of their probed lists
(ls_ivf_set_small_batch on) against the default service of the same call (one chain per query: centroid search, probed-
list scan, selection), same process, same handle, option off and on interleaved in bursts of synchronous calls.

Results are compared for equality (scores and indices, every query) before anything is timed. Per (shape, nprobe, nq)
it prints
  - the host time of the synchronous call (IVFFlatIndex.search), us per call: mean over REPEATS bursts of CALLS calls
    and [min .. max] of the bursts (the burst spread), and the p50 over all calls, off -> on;
  - what the on call launched: passes, queries left to chains, queries served again, union rows (ls_ivf_last_passes);
  - the byte model of the passes - union rows x row bytes / 7.09 TB/s - beside the measured fine stage of the on call
    (the library's event pairs: union step + pass + selection launch, summed over the call's groups).
Shapes: C2 (200 k x 384, k = 50) and C2' (200 k x 1024, k = 1000), nlist 447, nprobe 16 and 64, nq 1 / 2 / 4 / 8 / 16 / 32.

Gates (printed as PASS / FAIL; the exit code is 1 if one fails), each against the parent path in the same run:
  - nq = 16, nprobe = 64, both shapes: the WORST burst with the option on is below the BEST burst with it off;
  - nq = 1 (the same launches either way): the modes' means differ by no more than the bursts' own min-to-max spread.
nq = 2 and 4 are reported, not gated. The record goes to profiles/ab/ivf_small_batch.txt as well.

    python tools/ivf_small_batch_time.py     (ISB_SHAPES=0,1 ISB_NQS=1,2,4,8,16,32 ISB_REPEATS=5 ISB_CALLS=20)
"""
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from lean_explore_amd.id_selectors import SearchParametersIVF
from lean_explore_amd.ivf import IVFFlatIndex
from tests.test_ivf_gpu import mixture, queries

SHAPES = ((200_000, 384, 50), (200_000, 1024, 1000))  # C2, C2' (the reference's call shape)
if os.environ.get("ISB_SHAPES"):
    SHAPES = tuple(SHAPES[int(i)] for i in os.environ["ISB_SHAPES"].split(","))
NLIST = 447
NPROBES = tuple(int(x) for x in os.environ.get("ISB_NPROBES", "16,64").split(","))
NQS = tuple(int(x) for x in os.environ.get("ISB_NQS", "1,2,4,8,16,32").split(","))
REPEATS = int(os.environ.get("ISB_REPEATS", "5"))
CALLS = int(os.environ.get("ISB_CALLS", "20"))
OUT = ROOT / "profiles" / "ab" / "ivf_small_batch.txt"
lines, failed = [], []


def say(s):
    print(s, flush=True)
    lines.append(s)


def burst(ivf, q, k, par):
    """CALLS synchronous calls: (mean us per call, the calls' own times)"""
    t = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        ivf.search(q, k, normalize=True, params=par)
        t.append((time.perf_counter() - t0) * 1e6)
    return float(np.mean(t)), t


def fine_us(ivf, q, k, par):
    """the call's fine stage by the library's event pairs, us (mean of 5 calls), and the queries served again"""
    ivf.set_profiling(True)
    tot, resc = 0.0, 0
    for _ in range(5):
        ivf.search(q, k, normalize=True, params=par)
        _, f, r = ivf.last_kernel_ms()
        tot += f * 1e3
        resc = max(resc, r)
    ivf.set_profiling(False)
    return tot / 5, resc


def stats(v):
    return f"{np.mean(v):8.1f} [{np.min(v):7.1f} .. {np.max(v):7.1f}]"


def gate(name, ok, detail):
    say(f"  GATE {name}: {'PASS' if ok else 'FAIL'} ({detail})")
    if not ok:
        failed.append(name)


say(f"device: {torch.cuda.get_device_name(0)}; {REPEATS} bursts of {CALLS} synchronous calls per mode, interleaved off / on")
for (n, d, k) in SHAPES:
    corpus, cent = mixture(1000 + n + d, n, d, NLIST)
    ivf = IVFFlatIndex(d, NLIST)
    ivf.set_centroids(cent)
    ivf.add(corpus)
    sizes = ivf.list_sizes()
    qall = queries(77 + d, corpus, max(NQS))
    del corpus
    say(f"N={n} d={d} f32 k={k} nlist={NLIST}: lists of {sizes.min()}..{sizes.max()} rows")
    for nprobe in NPROBES:
        par = SearchParametersIVF(nprobe=nprobe)
        rows_q = int(np.sort(sizes)[::-1][:nprobe].sum())
        say(f" nprobe={nprobe}: one query probes at most {rows_q} rows ({100.0 * rows_q / n:.1f} % of the index)")
        for nq in NQS:
            q = np.ascontiguousarray(qall[:nq])
            ivf.set_small_batch(False)
            D0, I0 = ivf.search(q, k, normalize=True, params=par)
            ivf.set_small_batch(True)
            D1, I1 = ivf.search(q, k, normalize=True, params=par)
            passes, urows = ivf.last_passes()
            if not (np.array_equal(I0, I1) and np.array_equal(D0.view(np.uint32), D1.view(np.uint32))):
                say(f"  nq={nq}: RESULTS DIFFER between option off and on: nothing timed")
                failed.append(f"d={d} nprobe={nprobe} nq={nq} equality")
                continue
            res, every = {0: [], 1: []}, {0: [], 1: []}
            for mode in (0, 1):  # warm-up, both modes
                ivf.set_small_batch(bool(mode))
                for _ in range(5):
                    ivf.search(q, k, normalize=True, params=par)
            for _ in range(REPEATS):
                for mode in (0, 1):
                    ivf.set_small_batch(bool(mode))
                    m, t = burst(ivf, q, k, par)
                    res[mode].append(m)
                    every[mode] += t
            fine, resc = {}, {}
            for mode in (0, 1):
                ivf.set_small_batch(bool(mode))
                fine[mode], resc[mode] = fine_us(ivf, q, k, par)
            g = {mode: np.array(res[mode]) for mode in (0, 1)}
            grouped = sum(min(16, nq - i) for i in range(0, nq, 16) if nq - i >= 2) if passes else 0
            model = urows * d * 4 / 7.09e12 * 1e6
            for mode in (0, 1):
                say(f"  nq={nq:2d} {'on ' if mode else 'off'}: host us/call {stats(g[mode])}  p50 {np.median(every[mode]):8.1f}  "
                    f"fine stage {fine[mode]:8.1f} us  served again {resc[mode]}")
            say(f"  nq={nq:2d} on/off: host p50 {np.median(every[0]):.1f} -> {np.median(every[1]):.1f} us "
                f"({np.median(every[1]) / np.median(every[0]):.3f}); worst burst on {np.max(g[1]):.1f} vs best burst off "
                f"{np.min(g[0]):.1f}; on: {passes} pass(es), {nq - grouped} chain(s); off: {nq} chains; union rows {urows} "
                f"({urows * d * 4 / 1e6:.1f} MB: {model:.1f} us at 7.09 TB/s, measured union + pass + selection {fine[1]:.1f} us)"
                + ("" if passes or nq == 1 else "  [the plan declines: the same launches either way]"))
            if nq == 16 and nprobe == 64:
                gate(f"d={d} nprobe=64 nq=16 worst-on < best-off", np.max(g[1]) < np.min(g[0]),
                     f"{np.max(g[1]):.1f} vs {np.min(g[0]):.1f} us")
            if nq == 1:
                spread = max(np.max(g[0]) - np.min(g[0]), np.max(g[1]) - np.min(g[1]))
                gate(f"d={d} nprobe={nprobe} nq=1 on == off within the burst spread", abs(np.mean(g[1]) - np.mean(g[0])) <= spread,
                     f"|{np.mean(g[1]):.1f} - {np.mean(g[0]):.1f}| vs spread {spread:.1f} us")
    ivf.close()
OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text("\n".join(lines) + "\n")
if failed:
    say(f"FAILED gates: {failed}")
    sys.exit(1)
