#!/usr/bin/env python
"""ls_ivf_add timing on one box (include/leansearch_ivf_add.h):
    python tools/ivf_add_time.py [--rows 200000] [--d 1024] [--nlist 447] [--rounds 3] [--out profiles/ab/ivf_add.txt]
ONE process, the measurements INTERLEAVED round by round over the same seeded rows, explicit lists throughout (the
assignment's time is excluded), every call timed at the C ABI (wall clock around the ctypes call):
    create_all           ls_ivf_create over all rows: placement and the row permutation on the host, one upload
    create_empty_add_all ls_ivf_create over zero rows, then ONE ls_ivf_add of all rows: upload as given, lists merged in HBM
    add_1pct / add_10pct ls_ivf_add of 1 % / 10 % more rows onto the built index of `rows` rows ...
    rebuild_1pct / _10pct ... against ls_ivf_create over all of them from scratch
    merge kernel         hipEvent time of the row mover (ls_rows.hip) in each of the adds above, and its bytes (every stored row
                         read once and written once) over that time next to the 8 TB/s HBM peak
Nothing is gated: the figures are reported. The added index is checked against the rebuilt one (list sizes, one search).
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
ap.add_argument("--out", default=str(ROOT / "profiles" / "ab" / "ivf_add.txt"))
args = ap.parse_args()

from lean_explore_amd import native

lib = native.load()
n, d, nlist = args.rows, args.d, args.nlist
extra = n // 10
rng = np.random.default_rng(11)
x = rng.standard_normal((n + extra, d), dtype=np.float32)
cent = rng.standard_normal((nlist, d), dtype=np.float32)
assign = rng.integers(0, nlist, n + extra).astype(np.int32)
q = rng.standard_normal((4, d), dtype=np.float32)
print(f"rows {n} (+{extra}) x {d}, nlist {nlist}: data ready", flush=True)


def create(rows):
    """(handle, seconds) of ls_ivf_create over the first `rows` rows."""
    h = ctypes.c_void_p()
    t0 = time.perf_counter()
    native.check(lib.ls_ivf_create(ctypes.byref(h), x.ctypes.data if rows else None, rows, d, native.LS_DTYPE_F32,
                                   cent.ctypes.data, nlist, assign.ctypes.data if rows else None, 0))
    return h, time.perf_counter() - t0


def add(h, r0, r1):
    """(seconds, merge kernel ms, merge bytes) of ls_ivf_add of rows [r0, r1)."""
    native.check(lib.ls_ivf_set_profiling(h, 1))
    t0 = time.perf_counter()
    native.check(lib.ls_ivf_add(h, x[r0:r1].ctypes.data, r1 - r0, assign[r0:r1].ctypes.data))
    s = time.perf_counter() - t0
    ms, nb = ctypes.c_float(), ctypes.c_int64()
    native.check(lib.ls_ivf_add_last_kernel_ms(h, ctypes.byref(ms), ctypes.byref(nb)))
    return s, ms.value, nb.value


def observe(h):
    sizes = np.zeros(nlist, np.int64)
    native.check(lib.ls_ivf_list_sizes(h, sizes.ctypes.data))
    D, I = np.empty((4, 10), np.float32), np.empty((4, 10), np.int64)
    native.check(lib.ls_ivf_search(h, q.ctypes.data, 4, 10, 8, 0, D.ctypes.data, I.ctypes.data))
    return sizes, D, I


def spread(v, nd=4):
    v = np.asarray(v, dtype=np.float64)
    return {"mean": round(float(v.mean()), nd), "min": round(float(v.min()), nd), "max": round(float(v.max()), nd)}


wall = {k: [] for k in ("create_all", "create_empty_add_all", "add_1pct", "rebuild_1pct", "add_10pct", "rebuild_10pct")}
merge = {k: {"ms": [], "bytes": 0} for k in ("add_all", "add_1pct", "add_10pct")}
same = True
h, _ = create(1000)  # (warm-up: the runtime, the kernels' code objects)
add(h, 1000, 2000)
lib.ls_ivf_destroy(h)
for r in range(args.rounds):
    h_all, s = create(n)
    wall["create_all"].append(s)
    want = observe(h_all)
    h_add, s0 = create(0)
    s1, ms, nb = add(h_add, 0, n)
    wall["create_empty_add_all"].append(s0 + s1)
    merge["add_all"]["ms"].append(ms)
    merge["add_all"]["bytes"] = nb
    same &= all(np.array_equal(a, b) for a, b in zip(observe(h_add), want))
    lib.ls_ivf_destroy(h_add)
    for name, more in (("1pct", n // 100), ("10pct", n // 10)):
        if name == "10pct":  # (h_all carries the 1 % by now: a fresh index of `rows` rows)
            lib.ls_ivf_destroy(h_all)
            h_all, _ = create(n)
        s, ms, nb = add(h_all, n, n + more)
        wall["add_" + name].append(s)
        merge["add_" + name]["ms"].append(ms)
        merge["add_" + name]["bytes"] = nb
        h_re, s = create(n + more)
        wall["rebuild_" + name].append(s)
        same &= all(np.array_equal(a, b) for a, b in zip(observe(h_all), observe(h_re)))
        lib.ls_ivf_destroy(h_re)
    lib.ls_ivf_destroy(h_all)
    print(f"round {r}: " + ", ".join(f"{k} {v[-1]:.3f} s" for k, v in wall.items()), flush=True)

out = {
    "rows": n, "d": d, "nlist": nlist, "rounds": args.rounds,
    "wall_s": {k: spread(v) for k, v in wall.items()},
    "merge_kernel": {k: {"ms": spread(v["ms"]), "bytes": int(v["bytes"]),
                         "TBps": round(v["bytes"] / (np.mean(v["ms"]) * 1e-3) / 1e12, 3),
                         "fraction_of_8TBps": round(v["bytes"] / (np.mean(v["ms"]) * 1e-3) / 1e12 / PEAK_TBS, 4)}
                     for k, v in merge.items()},
    "added_index_equals_rebuilt": bool(same),
}
text = json.dumps(out, indent=1)
print(text, flush=True)
Path(args.out).parent.mkdir(parents=True, exist_ok=True)
Path(args.out).write_text(f"# tools/ivf_add_time.py --rows {n} --d {d} --nlist {nlist} --rounds {args.rounds} (one process, "
                          "the measurements interleaved; explicit lists)\n" + text + "\n")
sys.exit(0 if same else 1)
