#!/usr/bin/env python
"""IVF search, assignment and build under the inner product against L2, on one box (include/leansearch_ivf_l2.h,
DESIGN.md section 4.12):
    python tools/ivf_l2_time.py [--rows 200000] [--dims 384,1024] [--nlist 447] [--nprobe 64] [--nq 16] [--reps 5]
                                [--route-rows 20000] [--out profiles/ab/ivf_l2.txt]
ONE process; for every (d, dtype) an inner-product handle and an L2 handle of the SAME rows and lists, searched
alternately (ip, l2, ip, l2, ...), so that a pair is taken back to back:
    search   per k in (50, 1000): the coarse and fine kernel times of ls_ivf_last_kernel_ms (hipEvents, summed over the
             call's queries) and the host call time of ls_ivf_search, best and median of `reps` calls after one warm-up;
             the ratio l2 / ip of each.
    assign   ls_ivf_trainer_last_kernel_ms of the assignment kernel, inner-product form against L2 form, on the same
             rows and centroids (f32 rows only); 2 * rows * nlist * stored row length products per launch, so the L2
             form's rate is given in subtract + fma pairs per second next to the inner product's fma rate.
    routes   wall time of ls_ivf_create_l2(assign = NULL) over `route-rows` rows through the assignment kernel against
             the per-row search route (environment LS_IVF_L2_ASSIGN=search), same lists.
Nothing is gated: the numbers are reported."""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=200_000)
ap.add_argument("--dims", default="384,1024")
ap.add_argument("--nlist", type=int, default=447)
ap.add_argument("--nprobe", type=int, default=64)
ap.add_argument("--nq", type=int, default=16)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--route-rows", type=int, default=20_000)
ap.add_argument("--out", default=str(ROOT / "profiles" / "ab" / "ivf_l2.txt"))
args = ap.parse_args()

from lean_explore_amd.id_selectors import SearchParametersIVF  # noqa: E402
from lean_explore_amd.ivf import IVFFlatIndex, _Trainer  # noqa: E402


def data(seed, n, d, nlist):
    """Unnormalised rows around nlist centres, the centres as centroids, every row listed under its generating centre
    (both handles get the same lists: the comparison is of the kernels, not of two clusterings)."""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((nlist, d), dtype=np.float32)
    comp = rng.integers(0, nlist, n).astype(np.int32)
    x = rng.standard_normal((n, d), dtype=np.float32) * np.float32(0.35)
    x += cent[comp]
    return x, cent, comp


def med(v):
    return round(float(np.median(v)), 4)


out = {"rows": args.rows, "nlist": args.nlist, "nprobe": args.nprobe, "nq": args.nq, "reps": args.reps, "search": [],
       "assign": [], "routes": {}}
par = SearchParametersIVF(nprobe=args.nprobe)
for d in [int(v) for v in args.dims.split(",")]:
    x, cent, comp = data(7 + d, args.rows, d, args.nlist)
    q = x[:args.nq] + np.float32(0.05)
    for dtype in ("f32", "f16"):
        ix = {}
        for metric in ("ip", "l2"):
            ix[metric] = IVFFlatIndex(d, args.nlist, dtype=dtype, metric=metric)
            ix[metric].set_centroids(cent)
            ix[metric].add(x, assign=comp)
            ix[metric].set_profiling(True)
        for k in (50, 1000):
            t = {m: {"coarse_ms": [], "fine_ms": [], "call_ms": []} for m in ix}
            for rep in range(args.reps + 1):
                for m in ("ip", "l2"):
                    t0 = time.perf_counter()
                    ix[m].search(q, k, params=par)
                    dt = (time.perf_counter() - t0) * 1e3
                    c, f, _ = ix[m].last_kernel_ms()
                    if rep:  # (call 0 warms up)
                        t[m]["coarse_ms"].append(c)
                        t[m]["fine_ms"].append(f)
                        t[m]["call_ms"].append(dt)
            row = {"d": d, "dtype": dtype, "k": k}
            for key in ("coarse_ms", "fine_ms", "call_ms"):
                row[key] = {m: {"min": round(min(t[m][key]), 4), "median": med(t[m][key])} for m in ix}
                row[key]["l2_over_ip_median"] = round(med(t["l2"][key]) / med(t["ip"][key]), 3)
            out["search"].append(row)
            print(json.dumps(row), flush=True)
        for m in ix:
            ix[m].close()
    # the assignment kernel, both forms, on the same rows and centroids
    tr = {"ip": _Trainer(x, args.nlist, 0), "l2": _Trainer(x, args.nlist, 0, l2=True)}
    ms = {"ip": [], "l2": []}
    for rep in range(args.reps + 1):
        for m in ("ip", "l2"):
            tr[m].assign(cent)
            if rep:
                ms[m].append(tr[m].last_kernel_ms()[0])
    for m in tr:
        tr[m].close()
    d_pad = next(c * 4 for c in (16, 32, 48, 64, 96, 128, 192, 256) if c * 4 >= d)
    pairs = float(args.rows) * args.nlist * d_pad
    row = {"d": d, "assign_kernel_ms": {m: {"min": round(min(v), 4), "median": med(v)} for m, v in ms.items()},
           "l2_over_ip_median": round(med(ms["l2"]) / med(ms["ip"]), 3),
           "ip_tera_fma_per_s": round(pairs / (med(ms["ip"]) * 1e-3) / 1e12, 2),
           "l2_tera_sub_fma_pairs_per_s": round(pairs / (med(ms["l2"]) * 1e-3) / 1e12, 2)}
    out["assign"].append(row)
    print(json.dumps(row), flush=True)
    if d == 384:  # the two routes of the default assignment
        xr = np.ascontiguousarray(x[:args.route_rows])
        lists = {}
        for route in ("kernel", "search"):
            if route == "search":
                os.environ["LS_IVF_L2_ASSIGN"] = "search"
            r = IVFFlatIndex(d, args.nlist, metric="l2")
            r.set_centroids(cent)
            r.add(xr)
            t0 = time.perf_counter()
            lists[route] = r.assignment()  # (builds the handle: ls_ivf_create_l2 with assign = NULL)
            out["routes"][route + "_create_wall_s"] = round(time.perf_counter() - t0, 4)
            r.close()
        os.environ.pop("LS_IVF_L2_ASSIGN", None)
        out["routes"].update(rows=args.route_rows, d=d, same_lists=bool(np.array_equal(lists["kernel"], lists["search"])))
        print(json.dumps(out["routes"]), flush=True)

text = json.dumps(out, indent=1)
Path(args.out).parent.mkdir(parents=True, exist_ok=True)
Path(args.out).write_text(f"# tools/ivf_l2_time.py --rows {args.rows} --dims {args.dims} --nlist {args.nlist} --nprobe "
                          f"{args.nprobe} --nq {args.nq} --reps {args.reps} --route-rows {args.route_rows} (one process, "
                          "the inner-product and the L2 handle searched alternately)\n" + text + "\n")
print("written", args.out, flush=True)
