#!/usr/bin/env python
"""ls_remove timing on one box (include/leansearch_remove.h):
    python tools/flat_remove_time.py [--rows 200000] [--rounds 3] [--out profiles/ab/flat_remove.txt]
ONE process, the measurements INTERLEAVED round by round over the same seeded rows. Two shapes - `rows` x 1024 fp32 and
`rows` x 384 fp16 - and three removals of 1 % of the rows each: a random 1 %, the last 1 % (nothing moves) and the first
1 % (everything moves). Per removal:
    remove        wall clock of FlatIPIndex.remove_ids on the built index (one ls_remove)
    move_ms       ls_remove_last: the time of the row mover (ls_rows.hip) and the copies on the handle's stream, and their bytes
                  (read + written) over that time next to the 8 TB/s HBM peak
    rebuild       FlatIPIndex.from_array(survivors) plus the first search: what an update cost before ls_remove
    ivf_remove    ls_ivf_remove of the same rows on an IVF handle of the same corpus (the second-copy design)
Nothing is gated: the figures are reported. Every changed index is checked against the rebuilt one (stored rows, one
search).
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

PEAK_TBS = 8.0

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=200_000)
ap.add_argument("--nlist", type=int, default=447)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=str(ROOT / "profiles" / "ab" / "flat_remove.txt"))
args = ap.parse_args()

from lean_explore_amd.index import FlatIPIndex
from lean_explore_amd.ivf import IVFFlatIndex

n, nlist = args.rows, args.nlist


def spread(v, nd=4):
    v = np.asarray(v, dtype=np.float64)
    return {"mean": round(float(v.mean()), nd), "min": round(float(v.min()), nd), "max": round(float(v.max()), nd)}


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t0


def shape(d, dtype):
    rng = np.random.default_rng(12 + d)
    x = rng.standard_normal((n, d), dtype=np.float32)
    q = rng.standard_normal((4, d), dtype=np.float32)
    cent = rng.standard_normal((nlist, d), dtype=np.float32)
    assign = rng.integers(0, nlist, n).astype(np.int32)
    cnt = n // 100
    stale = {"random_1pct": np.zeros(n, bool), "last_1pct": np.arange(n) >= n - cnt, "first_1pct": np.arange(n) < cnt}
    stale["random_1pct"][rng.choice(n, cnt, replace=False)] = True
    warm = FlatIPIndex.from_array(x[:3000], dtype=dtype)  # (warm-up: the runtime, the kernels' code objects)
    warm.search(q, 10)
    warm.remove_ids(np.arange(0, 3000, 7))
    warm.close()
    res = {k: {"remove_s": [], "move_ms": [], "move_bytes": 0, "moved_rows": 0, "slabs": 0, "rebuild_s": [], "ivf_remove_s": []}
           for k in stale}
    same = True
    for r in range(args.rounds):
        for name, gone in stale.items():
            ix = FlatIPIndex.from_array(x, dtype=dtype)
            ix.search(q, 10)  # (the index has served a search)
            ix.set_profiling(True)
            before = ix.host_corpus()
            removed, s = timed(lambda: ix.remove_ids(gone))
            assert removed == cnt
            moved, slabs, ms, nb = ix.remove_stats()
            surv = np.ascontiguousarray(before[~gone])  # (made outside every timer)

            def rebuild():
                re = FlatIPIndex.from_array(surv, dtype=dtype)
                return re, re.search(q, 10)

            (re, (Dr, Ir)), s_re = timed(rebuild)
            D, I = ix.search(q, 10)
            same &= bool(np.array_equal(D, Dr) and np.array_equal(I, Ir) and np.array_equal(ix.host_corpus(), re.host_corpus()))
            re.close()
            ix.close()
            ivf = IVFFlatIndex(d, nlist, dtype=dtype)
            ivf.set_centroids(cent)
            ivf.add(x, assign=assign)
            ivf.search(q, 10)
            _, s_ivf = timed(lambda: ivf.remove_ids(gone))
            ivf.close()
            e = res[name]
            e["remove_s"].append(s)
            e["move_ms"].append(ms)
            e["move_bytes"], e["moved_rows"], e["slabs"] = nb, moved, slabs
            e["rebuild_s"].append(s_re)
            e["ivf_remove_s"].append(s_ivf)
            print(f"{dtype} d={d} round {r} {name}: remove {s:.4f} s (move {ms:.3f} ms, {moved} rows, {slabs} slabs), "
                  f"rebuild {s_re:.4f} s, ivf_remove {s_ivf:.4f} s", flush=True)
    out = {}
    for name, e in res.items():
        ms = float(np.mean(e["move_ms"]))
        out[name] = {"remove_s": spread(e["remove_s"]), "move_ms": spread(e["move_ms"]), "move_bytes": int(e["move_bytes"]),
                     "moved_rows": int(e["moved_rows"]), "slabs": int(e["slabs"]),
                     "move_TBps": round(e["move_bytes"] / (ms * 1e-3) / 1e12, 3) if ms > 0 else None,
                     "move_fraction_of_8TBps": round(e["move_bytes"] / (ms * 1e-3) / 1e12 / PEAK_TBS, 4) if ms > 0 else None,
                     "rebuild_s": spread(e["rebuild_s"]), "ivf_remove_s": spread(e["ivf_remove_s"])}
    return out, same


result = {"rows": n, "nlist": nlist, "rounds": args.rounds}
all_same = True
for d, dtype in ((1024, "f32"), (384, "f16")):
    result[f"{dtype}_d{d}"], ok = shape(d, dtype)
    all_same &= ok
result["changed_index_equals_rebuilt"] = bool(all_same)
text = json.dumps(result, indent=1)
print(text, flush=True)
Path(args.out).parent.mkdir(parents=True, exist_ok=True)
Path(args.out).write_text(f"# tools/flat_remove_time.py --rows {n} --nlist {nlist} --rounds {args.rounds} (one process, the "
                          "measurements interleaved)\n" + text + "\n")
sys.exit(0 if all_same else 1)
