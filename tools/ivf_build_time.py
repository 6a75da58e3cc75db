#!/usr/bin/env python
"""IVF build timing on one box (include/leansearch_ivf_build.h):
    python tools/ivf_build_time.py [--rows 200000] [--d 1024] [--nlist 447] [--niter 2] [--rounds 2] [--steps 6]
                                   [--out profiles/ab/ivf_build.txt]
ONE process, the host and the device path INTERLEAVED round by round over the same rows (a seeded Gaussian mixture):
    train      wall time of IVFFlatIndex.train(x, niter) with on_device False / True; `niter` is kept small (default 2:
               2 updates and 3 to 6 assignments) so that the host path - n / 8 launches per assignment and a host
               reduceat per update - finishes; both paths must return the same centroids, bit for bit.
    kernels    hipEvent times of the two kernels (ls_ivf_trainer_last_kernel_ms) over `--steps` Lloyd steps on one trainer
               of the sampled rows: the assignment kernel's FMA rate (2 * rows * nlist * stored row length flops) next to
               the 157.3 TFLOP/s vector fp32 peak, the means kernel's bytes per second (the rows once; and with the
               nlist reads of the assignment, which L2 serves) next to 8 TB/s.
    add        wall time of building the device index (add + first use) with and without build_on_device, same lists.
The one gated line: the device train is faster than the host train in every round. Everything else is reported.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

PEAK_TFLOPS, PEAK_TBS = 157.3, 8.0


def mixture(seed, n, d, comps):
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((comps, d), dtype=np.float32)
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    w = 1.0 / (np.arange(comps) + 3.0)
    x = np.empty((n, d), np.float32)
    for r0 in range(0, n, 50_000):  # in slabs: bounded temporaries
        m = min(50_000, n - r0)
        blk = rng.standard_normal((m, d), dtype=np.float32) * np.float32(0.35 / np.sqrt(d))
        blk += cent[rng.choice(comps, size=m, p=w / w.sum())]
        blk /= np.linalg.norm(blk, axis=1, keepdims=True)
        x[r0:r0 + m] = blk
    return x


def spread(v, nd=3):
    v = np.asarray(v, dtype=np.float64)
    return {"mean": round(float(v.mean()), nd), "min": round(float(v.min()), nd), "max": round(float(v.max()), nd)}


ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=200_000)
ap.add_argument("--d", type=int, default=1024)
ap.add_argument("--nlist", type=int, default=447)
ap.add_argument("--niter", type=int, default=2)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--steps", type=int, default=6)
ap.add_argument("--out", default=str(ROOT / "profiles" / "ab" / "ivf_build.txt"))
args = ap.parse_args()

from lean_explore_amd.ivf import MAX_POINTS_PER_CENTROID, IVFFlatIndex, _Trainer

n, d, nlist = args.rows, args.d, args.nlist
x = mixture(11, n, d, nlist)
print(f"rows {n} x {d}, nlist {nlist}: data ready", flush=True)

train_s = {"host": [], "device": []}
cents = {}
for r in range(args.rounds):
    for mode in (("host", "device") if r % 2 == 0 else ("device", "host")):
        ix = IVFFlatIndex(d, nlist)
        t0 = time.perf_counter()
        ix.train(x, niter=args.niter, on_device=(mode == "device"))
        train_s[mode].append(time.perf_counter() - t0)
        cents[mode] = ix.centroids.copy()
        ix.close()
        print(f"round {r} train[{mode}] {train_s[mode][-1]:.3f} s", flush=True)
same = bool(np.array_equal(cents["host"], cents["device"]))

# the two kernels, step by step, on the rows train() samples
rng = np.random.default_rng(1234)
cap = MAX_POINTS_PER_CENTROID * nlist
xs = x[np.sort(rng.choice(n, cap, replace=False))] if n > cap else x
cent = xs[np.sort(rng.choice(xs.shape[0], nlist, replace=False))].copy()
tr = _Trainer(np.ascontiguousarray(xs), nlist, 0)
assign_ms, means_ms = [], []
for s in range(args.steps + 1):
    tr.assign(cent)
    new = tr.means()
    a, m = tr.last_kernel_ms()
    if s:  # (step 0 warms up)
        assign_ms.append(a)
        means_ms.append(m)
    cent = new.astype(np.float32)
tr.close()
d_pad = -(-d // 4) * 4
for c in (16, 32, 48, 64, 96, 128, 192, 256):  # the stored row length (ls_pick_geom's table), in 16-byte chunks
    if c * 4 >= d:
        d_pad = c * 4
        break
ns = xs.shape[0]
flops = 2.0 * ns * nlist * d_pad
row_bytes = float(ns) * d_pad * 4
all_bytes = row_bytes + float(nlist) * ns * 4

# index build: the lists of add()
build_s = {}
lists = {}
for mode in ("host", "device"):
    ix = IVFFlatIndex(d, nlist, build_on_device=(mode == "device"))
    ix.set_centroids(cents["device"])
    ix.add(x)
    t0 = time.perf_counter()
    lists[mode] = ix.assignment()  # (builds the device index)
    build_s[mode] = time.perf_counter() - t0
    ix.close()

out = {
    "rows": n, "d": d, "nlist": nlist, "sampled_rows": int(ns), "niter": args.niter, "rounds": args.rounds,
    "train_wall_s": {m: spread(v) for m, v in train_s.items()},
    "train_same_centroids": same,
    "gate_device_train_faster_every_round": bool(all(dv < h for dv, h in zip(train_s["device"], train_s["host"]))),
    "assign_kernel_ms": spread(assign_ms),
    "assign_kernel_tflops": round(flops / (np.mean(assign_ms) * 1e-3) / 1e12, 2),
    "assign_kernel_fraction_of_vector_fp32_peak": round(flops / (np.mean(assign_ms) * 1e-3) / 1e12 / PEAK_TFLOPS, 4),
    "means_kernel_ms": spread(means_ms),
    "means_kernel_rows_TBps": round(row_bytes / (np.mean(means_ms) * 1e-3) / 1e12, 3),
    "means_kernel_rows_plus_assignment_reads_TBps": round(all_bytes / (np.mean(means_ms) * 1e-3) / 1e12, 3),
    "means_kernel_rows_fraction_of_8TBps": round(row_bytes / (np.mean(means_ms) * 1e-3) / 1e12 / PEAK_TBS, 4),
    "index_build_wall_s": {m: round(v, 3) for m, v in build_s.items()},
    "index_build_same_lists": bool(np.array_equal(lists["host"], lists["device"])),
}
text = json.dumps(out, indent=1)
print(text, flush=True)
Path(args.out).parent.mkdir(parents=True, exist_ok=True)
Path(args.out).write_text(f"# tools/ivf_build_time.py --rows {n} --d {d} --nlist {nlist} --niter {args.niter} --rounds "
                          f"{args.rounds} --steps {args.steps} (one process, host and device paths interleaved)\n"
                          + text + "\n")
sys.exit(0 if out["gate_device_train_faster_every_round"] and same else 1)
