#!/usr/bin/env python
"""Subset search timing on one box, interleaved (ls_search_subset, DESIGN.md section 4, "Subset search"):
    python tools/subset_bench.py [--reps 200] [--create-rows 12500000]
For the C2 shape (200 k x 384 f32, k = 50), C2' (200 k x 1024 f32, k = 1000) and 200 k x 384 f16 (k = 100): plain
ls_search on the full index, ls_search_subset with the all-ones subset, random 50 / 10 / 1 % subsets and one
contiguous 5 % block, and per subset a plain index holding exactly the selected rows (control). Host-call p50 / p90
(us) of single-query calls, rounds interleaved over the cases; kernel time from the library's hipEvent pairs
(ls_set_profiling / ls_last_kernel_ms: a plain call's scan launch with its riding selection - k > 256 selects in a
launch of its own, outside the pair -, a subset call's scan + finalize launches); the selected bytes over the kernel
time as a fraction of 8 TB/s, and over the host p50 (a lower bound: the host time includes launch and wait latency).
Then ls_subset_create time at 200 k and at --create-rows rows. The rocprofv3 runs: tools/subset_prof.py."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from lean_explore_amd import faiss_compat as fc  # noqa: E402
from lean_explore_amd.index import FlatIPIndex  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--create-rows", type=int, default=12_500_000)
args = ap.parse_args()
HBM = 8e12


def pct(a, p):
    return float(np.percentile(np.asarray(a) * 1e6, p))


def shape(n, d, k, dtype, seed):
    rng = np.random.default_rng(seed)
    corpus = rng.standard_normal((n, d), dtype=np.float32)
    corpus /= np.linalg.norm(corpus, axis=1, keepdims=True)
    q = rng.standard_normal((64, d), dtype=np.float32)
    ix = FlatIPIndex.from_array(corpus, dtype=dtype)
    elem = 2 if dtype == "f16" else 4
    masks = {"all": np.ones(n, bool)}
    for f in (0.5, 0.1, 0.01):
        masks[f"rand{int(f * 100)}%"] = rng.random(n) < f
    blk = np.zeros(n, bool)
    blk[n // 3:n // 3 + n // 20] = True
    masks["block5%"] = blk
    subs = {name: ix.subset(m) for name, m in masks.items()}
    ctrl = {name: FlatIPIndex.from_array(corpus[m], dtype=dtype) for name, m in masks.items()}
    cases = [("plain", lambda i: ix.search(q[i:i + 1], k))]
    for name in masks:
        p = fc.SearchParameters(sel=subs[name])
        cases.append((f"subset {name}", lambda i, p=p: ix.search(q[i:i + 1], k, params=p)))
        cases.append((f"control {name}", lambda i, c=ctrl[name]: c.search(q[i:i + 1], k)))
    for _, fn in cases:  # warm-up
        for i in range(10):
            fn(i % 64)
    t = {name: [] for name, _ in cases}
    for r in range(args.reps):  # interleaved rounds
        for name, fn in cases:
            t0 = time.perf_counter()
            fn(r % 64)
            t[name].append(time.perf_counter() - t0)
    kern = {}
    for name, fn in cases:  # kernel time: a separate pass with the hipEvent pairs on
        owner = ix if name.split()[0] != "control" else ctrl[name.split()[1]]
        owner.set_profiling(True)
        for i in range(50):
            fn(i % 64)
        kern[name] = owner.last_kernel_ms()[1] * 1e3
        owner.set_profiling(False)
    out = {}
    for name, _ in cases:
        m = n if name == "plain" else int(masks[name.split()[1]].sum())
        p50 = pct(t[name], 50)
        out[name] = {"rows": m, "p50_us": round(p50, 1), "p90_us": round(pct(t[name], 90), 1),
                     "kernel_us": round(kern[name], 1),
                     "selected_bytes_over_kernel_of_hbm": round(m * d * elem / (kern[name] * 1e-6) / HBM, 3),
                     "selected_bytes_over_p50_of_hbm": round(m * d * elem / (p50 * 1e-6) / HBM, 3)}
    for name in masks:
        out[f"subset {name}"]["vs_control_p50"] = round(out[f"subset {name}"]["p50_us"] /
                                                       out[f"control {name}"]["p50_us"], 3)
    out["subset all"]["vs_plain_p50"] = round(out["subset all"]["p50_us"] / out["plain"]["p50_us"], 3)
    out["subset all"]["vs_plain_kernel"] = round(out["subset all"]["kernel_us"] / out["plain"]["kernel_us"], 3)
    for s in subs.values():
        s.close()
    for c in ctrl.values():
        c.close()
    ix.close()
    return out


def create_time(n, d=8):
    ix = FlatIPIndex.from_array(np.zeros((n, d), np.float32))
    mask = np.random.default_rng(0).random(n) < 0.5
    ix.subset(mask).close()  # warm-up
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        s = ix.subset(mask)
        ts.append(time.perf_counter() - t0)
        s.close()
    ix.close()
    return round(float(np.median(ts)) * 1e3, 2)


res = {"c2 200k x 384 f32 k=50": shape(200_000, 384, 50, "f32", 1),
       "c2' 200k x 1024 f32 k=1000": shape(200_000, 1024, 1000, "f32", 2),
       "200k x 384 f16 k=100": shape(200_000, 384, 100, "f16", 3),
       "ls_subset_create_ms": {"200k": create_time(200_000), f"{args.create_rows}": create_time(args.create_rows)}}
print(json.dumps(res, indent=1))
