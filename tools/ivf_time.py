#!/usr/bin/env python
"""IVF-flat search timing on one box (ls_ivf_search):
    python tools/ivf_time.py [--reps 300] [--shapes c2,c2p,c2m,c2_f16] [--out profiles/ab/ivf_search.txt]
Per shape ONE child process builds a flat index and an IVF index of the same rows (seeded Gaussian mixture, centroids
from IVFFlatIndex.train) and times single-query host calls of both, INTERLEAVED round by round: ls_search on the flat
index against ls_ivf_search at every nprobe of the shape. Each child runs under its own time limit and the run stops at
the first child that fails. Recorded per (shape, nprobe): rows and bytes probed (mean, max over the queries), coarse
and fine kernel time (the library's hipEvents, ls_ivf_set_profiling / ls_ivf_last_kernel_ms; a separate pass), the
fine time over the one-stream model t = bytes / 7.09 TB/s + 3.1 us applied to the probed bytes,
host p50 / p90 of both calls, queries that needed the second launch, recall@k against exact.
Cross-check of the event times (its own run; counters are never combined with tracing):
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/ivf_time.py --child c2m --reps 50
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

# name: (rows, d, dtype, k, nlist, nprobes, child time limit in seconds)
SHAPES = {
    "c2": (200_000, 384, "f32", 50, 447, (64,), 240),
    "c2p": (200_000, 1024, "f32", 1000, 447, (64,), 300),
    "c2m": (1_000_000, 384, "f32", 50, 1000, (16, 64, 256), 420),
    "c2_f16": (200_000, 384, "f16", 100, 447, (64,), 240),
}
MODEL_BW, MODEL_FLOOR_US = 7.09e12, 3.1


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
    return x


def pct(a, p):
    return round(float(np.percentile(np.asarray(a) * 1e6, p)), 1)


def child(name, reps):
    from lean_explore_amd.index import FlatIPIndex
    from lean_explore_amd.ivf import IVFFlatIndex

    n, d, dtype, k, nlist, nprobes, _ = SHAPES[name]
    elem = 2 if dtype == "f16" else 4
    corpus = mixture(11, n, d, nlist)
    rng = np.random.default_rng(12)
    q = corpus[rng.choice(n, 64, replace=False)] + np.float32(0.05) * rng.standard_normal((64, d), dtype=np.float32)
    q = np.ascontiguousarray(q, dtype=np.float32)
    t0 = time.perf_counter()
    ivf = IVFFlatIndex(d, nlist, dtype=dtype)
    ivf.train(corpus, niter=5)
    t_train = time.perf_counter() - t0
    ivf.add(corpus)
    t0 = time.perf_counter()
    sizes = ivf.list_sizes()
    t_build = time.perf_counter() - t0
    assign = ivf.assignment()
    flat = FlatIPIndex.from_array(corpus, dtype=dtype)
    De, Ie = flat.search(q, k, normalize=True)
    cases = [("exact", None)] + [(f"ivf nprobe {p}", p) for p in nprobes]

    def call(p, i):
        if p is None:
            return flat.search(q[i:i + 1], k, normalize=True)
        ivf.nprobe = p
        return ivf.search(q[i:i + 1], k, normalize=True)

    for _, p in cases:  # warm-up
        for i in range(10):
            call(p, i)
    t = {c: [] for c, _ in cases}
    for r in range(reps):  # interleaved rounds
        for c, p in cases:
            t0 = time.perf_counter()
            call(p, r % 64)
            t[c].append(time.perf_counter() - t0)
    out = {"shape": name, "rows": n, "d": d, "dtype": dtype, "k": k, "nlist": nlist, "reps": reps,
           "list_rows_min_mean_max": [int(sizes.min()), round(float(sizes.mean()), 1), int(sizes.max())],
           "train_s": round(t_train, 2), "build_s": round(t_build, 2),
           "exact": {"p50_us": pct(t["exact"], 50), "p90_us": pct(t["exact"], 90)}}
    flat.set_profiling(True)
    for i in range(50):
        call(None, i)
    out["exact"]["kernel_us"] = round(flat.last_kernel_ms()[1] * 1e3, 1)  # (mean over the 50 launches)
    flat.set_profiling(False)
    for c, p in cases[1:]:
        _, P = ivf.quantizer.search(q, min(p, nlist), normalize=True)
        probed = np.array([int(sizes[P[i][P[i] >= 0]].sum()) for i in range(64)])
        ivf.nprobe = p
        D, I = ivf.search(q, k, normalize=True)
        recall = float(np.mean([len(set(I[i][I[i] >= 0]) & set(Ie[i])) / k for i in range(64)]))
        ivf.set_profiling(True)
        coarse, fine, rescued = [], [], 0
        for i in range(64):
            ivf.search(q[i:i + 1], k, normalize=True)
            a, b, r = ivf.last_kernel_ms()
            coarse.append(a * 1e3)
            fine.append(b * 1e3)
            rescued += r
        ivf.set_profiling(False)
        model = probed * d * elem / MODEL_BW * 1e6 + MODEL_FLOOR_US
        ratio = np.array(fine) / model
        out[c] = {"rows_probed_mean": round(float(probed.mean())), "rows_probed_max": int(probed.max()),
                  "bytes_probed_mean": int(probed.mean() * d * elem), "bytes_probed_max": int(probed.max() * d * elem),
                  "coarse_kernel_us_p50": round(float(np.median(coarse)), 1),
                  "fine_kernel_us_p50": round(float(np.median(fine)), 1),
                  "fine_over_model_p50": round(float(np.median(ratio)), 3),
                  "fine_over_model_max": round(float(ratio.max()), 3),
                  "fine_target_applies": bool(probed.mean() * d * elem >= 100e6),
                  "second_launch_queries_of_64": rescued,
                  "p50_us": pct(t[c], 50), "p90_us": pct(t[c], 90),
                  "p50_over_exact_p50": round(pct(t[c], 50) / out["exact"]["p50_us"], 3),
                  f"recall_at_{k}": round(recall, 4)}
        assert (I[I >= 0] < n).all() and assign.size == n
    ivf.close()
    flat.close()
    print("IVF_TIME " + json.dumps(out), flush=True)


ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=300)
ap.add_argument("--shapes", default="c2,c2p,c2m,c2_f16")
ap.add_argument("--out", default=str(ROOT / "profiles" / "ab" / "ivf_search.txt"))
ap.add_argument("--child", default=None)
args = ap.parse_args()
if args.child:
    child(args.child, args.reps)
    sys.exit(0)
lines = []
for name in args.shapes.split(","):
    limit = SHAPES[name][-1]
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, __file__, "--child", name, "--reps",
                        str(args.reps)], capture_output=True, text=True)
    got = [ln[len("IVF_TIME "):] for ln in p.stdout.splitlines() if ln.startswith("IVF_TIME ")]
    if p.returncode != 0 or not got:
        print(f"{name}: child failed (exit {p.returncode}); stopping here\n{p.stderr[-2000:]}", file=sys.stderr)
        break
    lines.append(json.dumps(json.loads(got[0]), indent=1))
    print(lines[-1], flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("# tools/ivf_time.py --reps %d (one child process per shape, IVF and exact interleaved)\n"
                              % args.reps + "\n".join(lines) + "\n")
sys.exit(0 if len(lines) == len(args.shapes.split(",")) else 1)
