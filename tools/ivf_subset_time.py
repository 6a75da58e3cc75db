#!/usr/bin/env python
"""IVF subset search timing on one box (ls_ivf_search_subset):
    python tools/ivf_subset_time.py [--bursts 6] [--calls 8] [--reps 200] [--shapes c2,c2p,c2_sq8]
                                    [--out profiles/ab/ivf_subset.txt]
Per shape ONE child process and ONE IVF handle (seeded Gaussian mixture, the mixture's centres as centroids, the
library's default assignment) plus a flat index of the same rows for the control row. Modes:
    unfiltered     ls_ivf_search
    ones           the all-ones subset
    r50, r10, r1   random 50 / 10 / 1 % subsets
    block10        one contiguous 10 % block of original rows
    flat_r10       ls_search_subset on the flat index for the r10 selection (no probing: every selected row is scanned)
Fine-stage kernel time: the library's hipEvents (ls_ivf_set_profiling / ls_ivf_last_kernel_ms: the probed-list scan and
its selection, summed over the queries of a call) over 16-query calls, per query. The modes are INTERLEAVED in bursts:
every burst runs `--calls` calls of every mode, in an order rotated from burst to burst; a mode's burst value is the mean
over its calls, and the record gives mean [min .. max] of the bursts. flat_r10 is the flat handle's event pair (scan and
selection) per query. Host p50 / p90: single-query calls with profiling off, interleaved round by round. Subset creation:
bitmap in hand -> IVFFlatIndex.subset returns (host compaction and three uploads), median of 5.
Two conditions are judged on the record:
    (A) ones / unfiltered <= 1 + max(0.05, (max - min) / mean of the unfiltered bursts)
    (B) r10 < unfiltered
Each child runs under its own time limit and the run stops at the first child that fails.
A counters-only follow-up, in a run of its own: rocprofv3 --pmc <counters> -- python tools/ivf_subset_time.py --child c2
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

# name: (rows, d, dtype, k, nlist, nprobe, child time limit in seconds)
SHAPES = {
    "c2": (200_000, 384, "f32", 50, 447, 64, 300),
    "c2p": (200_000, 1024, "f32", 1000, 447, 64, 420),
    "c2_sq8": (200_000, 384, "sq8", 50, 447, 64, 300),
}
NQ = 16


def mixture(seed, n, d, comps):
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((comps, d), dtype=np.float32)
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    w = 1.0 / (np.arange(comps) + 3.0)
    x = np.empty((n, d), np.float32)
    for r0 in range(0, n, 100_000):  # in slabs: bounded temporaries
        m = min(100_000, n - r0)
        blk = rng.standard_normal((m, d), dtype=np.float32) * np.float32(0.35 / np.sqrt(d))
        blk += cent[rng.choice(comps, size=m, p=w / w.sum())]
        blk /= np.linalg.norm(blk, axis=1, keepdims=True)
        x[r0:r0 + m] = blk
    return x, cent


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return {"mean": round(float(v.mean()), 2), "min": round(float(v.min()), 2), "max": round(float(v.max()), 2)}


def child(name, bursts, calls, reps):
    from lean_explore_amd.id_selectors import IDSelectorBitmap, SearchParameters, SearchParametersIVF
    from lean_explore_amd.index import FlatIPIndex
    from lean_explore_amd.ivf import IVFFlatIndex

    n, d, dtype, k, nlist, nprobe, _ = SHAPES[name]
    corpus, cent = mixture(11, n, d, nlist)
    rng = np.random.default_rng(12)
    q = corpus[rng.choice(n, 64, replace=False)] + np.float32(0.05) * rng.standard_normal((64, d), dtype=np.float32)
    q = np.ascontiguousarray(q, dtype=np.float32)
    ivf = IVFFlatIndex(d, nlist, dtype=dtype)
    ivf.set_centroids(cent)
    ivf.add(corpus)
    ivf.nprobe = nprobe
    sizes = ivf.list_sizes()
    flat = FlatIPIndex.from_array(corpus, dtype=dtype)
    masks = {"ones": np.ones(n, bool), "r50": rng.random(n) < 0.5, "r10": rng.random(n) < 0.1, "r1": rng.random(n) < 0.01,
             "block10": (np.arange(n) >= int(0.45 * n)) & (np.arange(n) < int(0.55 * n))}
    create_ms, subs = {}, {}
    for mname, mask in masks.items():
        bm = np.packbits(mask, bitorder="little")
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            s = ivf.subset(IDSelectorBitmap(bm))
            ts.append(time.perf_counter() - t0)
            s.close()
        subs[mname] = ivf.subset(mask)
        create_ms[mname] = {"rows": subs[mname].rows, "ms_median": round(float(np.median(ts)) * 1e3, 3)}
    fsub = flat.subset(masks["r10"])
    modes = ["unfiltered"] + list(masks) + ["flat_r10"]

    def call(mode, x):
        if mode == "unfiltered":
            return ivf.search(x, k, normalize=True)
        if mode == "flat_r10":
            return flat.search(x, k, normalize=True, params=SearchParameters(sel=fsub))
        return ivf.search(x, k, normalize=True, params=SearchParametersIVF(sel=subs[mode], nprobe=nprobe))

    # results must not change: the all-ones subset is the unfiltered search, bit for bit, at the size timed
    Du, Iu = call("unfiltered", q)
    Do, Io = call("ones", q)
    assert np.array_equal(Iu, Io) and np.array_equal(Du, Do), "all-ones subset != unfiltered search"
    _, I10 = call("r10", q)
    assert masks["r10"][I10[I10 >= 0]].all()

    for mode in modes:  # warm-up: every mode at both call sizes
        for i in range(4):
            call(mode, q[:NQ])
            call(mode, q[i:i + 1])
    ivf.set_profiling(True)
    flat.set_profiling(True)
    fine = {m: [] for m in modes}
    rescued = {m: 0 for m in modes}
    for b in range(bursts):
        for j in range(len(modes)):
            mode = modes[(j + b) % len(modes)]  # rotated: no mode always follows the same neighbour
            vals = []
            for c in range(calls):
                x = q[(c % 4) * NQ:(c % 4 + 1) * NQ]
                call(mode, x)
                if mode == "flat_r10":
                    vals.append(flat.last_kernel_ms()[1] * 1e3)  # (mean over the call's queries already)
                else:
                    _, f, r = ivf.last_kernel_ms()
                    vals.append(f * 1e3 / NQ)
                    rescued[mode] += r
            fine[mode].append(float(np.mean(vals)))
    ivf.set_profiling(False)
    flat.set_profiling(False)
    host = {m: [] for m in modes}
    for r in range(reps):
        for mode in modes:
            x = q[r % 64:r % 64 + 1]
            t0 = time.perf_counter()
            call(mode, x)
            host[mode].append(time.perf_counter() - t0)
    # rows a query reads: probed, and probed AND selected
    _, P = ivf.quantizer.search(q, min(nprobe, nlist), normalize=True)
    assign = ivf.assignment()
    rows_read = {"unfiltered": float(np.mean([sizes[P[i][P[i] >= 0]].sum() for i in range(64)]))}
    for mname, mask in masks.items():
        per_list = np.bincount(assign[mask], minlength=nlist)
        rows_read[mname] = float(np.mean([per_list[P[i][P[i] >= 0]].sum() for i in range(64)]))
    rows_read["flat_r10"] = float(masks["r10"].sum())
    out = {"shape": name, "rows": n, "d": d, "dtype": dtype, "k": k, "nlist": nlist, "nprobe": nprobe,
           "bursts": bursts, "calls_per_burst": calls, "queries_per_call": NQ, "host_reps": reps,
           "list_rows_min_mean_max": [int(sizes.min()), round(float(sizes.mean()), 1), int(sizes.max())],
           "modes": {}, "subset_create": create_ms}
    for mode in modes:
        out["modes"][mode] = {"rows_read_mean": round(rows_read[mode]), "fine_us_per_query": spread(fine[mode]),
                              "second_launch_queries": rescued[mode],
                              "host_p50_us": round(float(np.percentile(np.asarray(host[mode]) * 1e6, 50)), 1),
                              "host_p90_us": round(float(np.percentile(np.asarray(host[mode]) * 1e6, 90)), 1)}
    u = out["modes"]["unfiltered"]["fine_us_per_query"]
    allow = max(0.05, (u["max"] - u["min"]) / u["mean"])
    ra = out["modes"]["ones"]["fine_us_per_query"]["mean"] / u["mean"]
    rb = out["modes"]["r10"]["fine_us_per_query"]["mean"] / u["mean"]
    out["condition_A"] = {"ones_over_unfiltered": round(ra, 4), "allowance": round(allow, 4), "holds": bool(ra <= 1 + allow)}
    out["condition_B"] = {"r10_over_unfiltered": round(rb, 4), "holds": bool(rb < 1.0)}
    for s in subs.values():
        s.close()
    fsub.close()
    ivf.close()
    flat.close()
    print("IVF_SUBSET_TIME " + json.dumps(out), flush=True)


ap = argparse.ArgumentParser()
ap.add_argument("--bursts", type=int, default=6)
ap.add_argument("--calls", type=int, default=8)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--shapes", default="c2,c2p,c2_sq8")
ap.add_argument("--out", default=str(ROOT / "profiles" / "ab" / "ivf_subset.txt"))
ap.add_argument("--child", default=None)
args = ap.parse_args()
if args.child:
    child(args.child, args.bursts, args.calls, args.reps)
    sys.exit(0)
lines = []
for name in args.shapes.split(","):
    limit = SHAPES[name][-1]
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, __file__, "--child", name, "--bursts",
                        str(args.bursts), "--calls", str(args.calls), "--reps", str(args.reps)],
                       capture_output=True, text=True)
    got = [ln[len("IVF_SUBSET_TIME "):] for ln in p.stdout.splitlines() if ln.startswith("IVF_SUBSET_TIME ")]
    if p.returncode != 0 or not got:
        print(f"{name}: child failed (exit {p.returncode}); stopping here\n{p.stderr[-2000:]}", file=sys.stderr)
        break
    lines.append(json.dumps(json.loads(got[0]), indent=1))
    print(lines[-1], flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("# tools/ivf_subset_time.py --bursts %d --calls %d --reps %d (one child process and one IVF "
                              "handle per shape, modes interleaved in bursts)\n" % (args.bursts, args.calls, args.reps)
                              + "\n".join(lines) + "\n")
sys.exit(0 if len(lines) == len(args.shapes.split(",")) else 1)
