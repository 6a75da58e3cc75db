#!/usr/bin/env python
"""ls_ivf_remove timing on one box (include/leansearch_ivf_remove.h):
    python tools/ivf_remove_time.py [--rows 200000] [--d 1024] [--nlist 447] [--rounds 3] [--out profiles/ab/ivf_remove.txt]
ONE process, the measurements INTERLEAVED round by round over the same seeded rows, explicit lists throughout (the
assignment's time is excluded), every call timed at the C ABI (wall clock around the ctypes call):
    remove_1pct / remove_10pct  ls_ivf_remove of a random 1 % / 10 % of the rows of the built index of `rows` rows ...
    rebuild_1pct / _10pct       ... against ls_ivf_create over the survivors from scratch
    update_1pct                 the 1 % removal followed by ls_ivf_add of as many fresh rows ...
    rebuild_update_1pct         ... against ONE ls_ivf_create over the survivors followed by the fresh rows
    compact kernel              hipEvent time of the row mover (ls_rows.hip) in each of the removals above, and its bytes (every
                                surviving stored row read once and written once) over that time next to the 8 TB/s HBM peak
Nothing is gated: the figures are reported. Every changed index is checked against the rebuilt one (list sizes, one
search).
"""
import argparse
import ctypes
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
ap.add_argument("--d", type=int, default=1024)
ap.add_argument("--nlist", type=int, default=447)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=str(ROOT / "profiles" / "ab" / "ivf_remove.txt"))
args = ap.parse_args()

from lean_explore_amd import native

lib = native.load()
n, d, nlist = args.rows, args.d, args.nlist
rng = np.random.default_rng(12)
x = rng.standard_normal((n, d), dtype=np.float32)
fresh = rng.standard_normal((n // 100, d), dtype=np.float32)
cent = rng.standard_normal((nlist, d), dtype=np.float32)
assign = rng.integers(0, nlist, n).astype(np.int32)
assign_fresh = rng.integers(0, nlist, n // 100).astype(np.int32)
q = rng.standard_normal((4, d), dtype=np.float32)
stale = {}
for name, count in (("1pct", n // 100), ("10pct", n // 10)):
    gone = np.zeros(n, bool)
    gone[rng.choice(n, count, replace=False)] = True
    stale[name] = gone
# what the rebuilds are given: made here, outside every timer
surv = {name: (np.ascontiguousarray(x[~g]), np.ascontiguousarray(assign[~g])) for name, g in stale.items()}
updated = (np.concatenate([surv["1pct"][0], fresh]), np.concatenate([surv["1pct"][1], assign_fresh]))
print(f"rows {n} x {d}, nlist {nlist}: data ready", flush=True)


def create(rows, lists):
    """(handle, seconds) of ls_ivf_create over `rows`."""
    h = ctypes.c_void_p()
    t0 = time.perf_counter()
    native.check(lib.ls_ivf_create(ctypes.byref(h), rows.ctypes.data, rows.shape[0], d, native.LS_DTYPE_F32,
                                   cent.ctypes.data, nlist, lists.ctypes.data, 0))
    return h, time.perf_counter() - t0


def remove(h, gone):
    """(seconds, compact kernel ms, compact bytes) of ls_ivf_remove of the rows `gone` marks."""
    bm = np.packbits(gone, bitorder="little")
    removed = ctypes.c_int64()
    native.check(lib.ls_ivf_set_profiling(h, 1))
    t0 = time.perf_counter()
    native.check(lib.ls_ivf_remove(h, bm.ctypes.data, bm.size, ctypes.byref(removed)))
    s = time.perf_counter() - t0
    assert removed.value == gone.sum()
    ms, nb = ctypes.c_float(), ctypes.c_int64()
    native.check(lib.ls_ivf_remove_last_kernel_ms(h, ctypes.byref(ms), ctypes.byref(nb)))
    return s, ms.value, nb.value


def add(h, rows, lists):
    t0 = time.perf_counter()
    native.check(lib.ls_ivf_add(h, rows.ctypes.data, rows.shape[0], lists.ctypes.data))
    return time.perf_counter() - t0


def observe(h):
    sizes = np.zeros(nlist, np.int64)
    native.check(lib.ls_ivf_list_sizes(h, sizes.ctypes.data))
    D, I = np.empty((4, 10), np.float32), np.empty((4, 10), np.int64)
    native.check(lib.ls_ivf_search(h, q.ctypes.data, 4, 10, 8, 0, D.ctypes.data, I.ctypes.data))
    return sizes, D, I


def spread(v, nd=4):
    v = np.asarray(v, dtype=np.float64)
    return {"mean": round(float(v.mean()), nd), "min": round(float(v.min()), nd), "max": round(float(v.max()), nd)}


wall = {k: [] for k in ("remove_1pct", "rebuild_1pct", "update_1pct", "rebuild_update_1pct", "remove_10pct",
                        "rebuild_10pct")}
compact = {k: {"ms": [], "bytes": 0} for k in ("remove_1pct", "remove_10pct")}
same = True
h, _ = create(x[:2000], assign[:2000])  # (warm-up: the runtime, the kernels' code objects)
remove(h, stale["1pct"][:2000] | (np.arange(2000) == 0))
add(h, fresh[:100], assign_fresh[:100])
lib.ls_ivf_destroy(h)
for r in range(args.rounds):
    for name in ("1pct", "10pct"):
        h, _ = create(x, assign)
        observe(h)  # (the index has served a search)
        s_rm, ms, nb = remove(h, stale[name])
        wall["remove_" + name].append(s_rm)
        compact["remove_" + name]["ms"].append(ms)
        compact["remove_" + name]["bytes"] = nb
        h_re, s = create(*surv[name])
        wall["rebuild_" + name].append(s)
        same &= all(np.array_equal(a, b) for a, b in zip(observe(h), observe(h_re)))
        lib.ls_ivf_destroy(h_re)
        if name == "1pct":  # the update: the removal above, then as many fresh rows
            wall["update_1pct"].append(s_rm + add(h, fresh, assign_fresh))
            h_re, s = create(*updated)
            wall["rebuild_update_1pct"].append(s)
            same &= all(np.array_equal(a, b) for a, b in zip(observe(h), observe(h_re)))
            lib.ls_ivf_destroy(h_re)
        lib.ls_ivf_destroy(h)
    print(f"round {r}: " + ", ".join(f"{k} {v[-1]:.4f} s" for k, v in wall.items()), flush=True)

out = {
    "rows": n, "d": d, "nlist": nlist, "rounds": args.rounds,
    "wall_s": {k: spread(v) for k, v in wall.items()},
    "compact_kernel": {k: {"ms": spread(v["ms"]), "bytes": int(v["bytes"]),
                           "TBps": round(v["bytes"] / (np.mean(v["ms"]) * 1e-3) / 1e12, 3),
                           "fraction_of_8TBps": round(v["bytes"] / (np.mean(v["ms"]) * 1e-3) / 1e12 / PEAK_TBS, 4)}
                       for k, v in compact.items()},
    "changed_index_equals_rebuilt": bool(same),
}
text = json.dumps(out, indent=1)
print(text, flush=True)
Path(args.out).parent.mkdir(parents=True, exist_ok=True)
Path(args.out).write_text(f"# tools/ivf_remove_time.py --rows {n} --d {d} --nlist {nlist} --rounds {args.rounds} (one process, "
                          "the measurements interleaved; explicit lists)\n" + text + "\n")
sys.exit(0 if same else 1)
