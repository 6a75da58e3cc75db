#!/usr/bin/env python
"""L2 flat index, small batches: the query groups of ls_set_l2_small_batch against one launch per query, on one box
(include/leansearch_l2_batch.h):
    python tools/l2_batch_time.py --mode groups|single [--root TREE] [--rows 200000] [--dims 384,1024] [--nqs 4,8,16]
                                  [--ks 50,1000] [--calls 50] [--warm 10] [--out profiles/ab/l2_batch_groups.json]
ONE process, ls_set_profiling on. For every (d, dtype, k, nq): `warm` calls, then `calls` calls of ls_search; per call the
summed kernel time of its scan launches (ls_last_kernel_ms is the mean over the call's profiled launches, so it is
multiplied by their number: nq launches in `single` mode, the groups of 8 / 4 / 1 in `groups` mode - pass --group8 0
for a shape the plan serves in groups of 4) and the host time of the call. Medians.
--mode single never touches the switch, so it also runs on a tree without it (--root: the tree whose package and
library are loaded): that is how the parent commit's build is measured in the same session, as the baseline.
Nothing is gated: the numbers are reported. The share of the 8.0 TB/s HBM peak is corpus bytes / pass time."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("groups", "single"), required=True)
ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent))
ap.add_argument("--rows", type=int, default=200_000)
ap.add_argument("--dims", default="384,1024")
ap.add_argument("--nqs", default="4,8,16")
ap.add_argument("--ks", default="50,1000")
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--warm", type=int, default=10)
ap.add_argument("--group8", type=int, default=1)
ap.add_argument("--out", default="")
args = ap.parse_args()
sys.path.insert(0, str(Path(args.root).resolve()))

from lean_explore_amd.index import FlatL2Index  # noqa: E402

HBM_PEAK = 8.0e12


def launches(nq):
    if args.mode == "single":
        return nq
    count, left = 0, nq
    while left > 0:
        left -= min(8 if left >= 5 and args.group8 else (4 if left >= 2 else 1), left)
        count += 1
    return count


def med(v):
    return round(float(np.median(v)), 4)


rows_out = []
for d in [int(v) for v in args.dims.split(",")]:
    rng = np.random.default_rng(7 + d)
    x = rng.standard_normal((args.rows, d), dtype=np.float32)
    q_all = rng.standard_normal((16, d), dtype=np.float32)
    for dtype in ("f32", "f16"):
        ix = FlatL2Index.from_array(x, dtype=dtype)
        if args.mode == "groups":
            ix.set_l2_small_batch(True)
        ix.set_profiling(True)
        corpus_bytes = args.rows * ((d * (4 if dtype == "f32" else 2) + 15) // 16 * 16)
        for k in [int(v) for v in args.ks.split(",")]:
            for nq in [int(v) for v in args.nqs.split(",")]:
                q = np.ascontiguousarray(q_all[:nq])
                kern, call = [], []
                for rep in range(args.warm + args.calls):
                    t0 = time.perf_counter()
                    ix.search(q, k)
                    dt = (time.perf_counter() - t0) * 1e3
                    mean_ms, _ = ix.last_kernel_ms()
                    if rep >= args.warm:
                        kern.append(mean_ms * launches(nq))
                        call.append(dt)
                n_l = launches(nq)
                row = {"mode": args.mode, "d": d, "dtype": dtype, "k": k, "nq": nq, "launches": n_l,
                       "kernel_ms_sum_median": med(kern), "kernel_ms_per_launch_median": round(med(kern) / n_l, 4),
                       "call_ms_median": med(call),
                       "hbm_share_per_launch": round(corpus_bytes / (med(kern) / n_l * 1e-3) / HBM_PEAK, 3)}
                rows_out.append(row)
                print(json.dumps(row), flush=True)
        ix.close()

if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"args": vars(args), "rows": rows_out}, indent=1) + "\n")
    print("written", args.out, flush=True)
