#!/usr/bin/env python
"""bf16 rows against fp16 rows of the same values, scan kernel time on one box (include/leansearch_bf16.h, DESIGN.md
section 4.13):
    python tools/bf16_time.py [--rows 200000] [--dims 384,1024] [--nlist 447] [--nprobe 64] [--k 50] [--calls 200]
                              [--warm 20] [--out profiles/ab/bf16_scan.txt]
ONE process, profiling on (hipEvent pairs around every scan launch: ls_set_profiling / ls_ivf_set_profiling). Per shape
the fp16 index and the bf16 index of the same rows serve the same single query in turn - fp16, bf16, fp16 again - so
that the two fp16 series give the run-to-run spread the bf16 series is read against. Medians of the scan kernel's time
(flat: the single-query scan launch; IVF: the fine stage), their ratio, and the share of the 8.0 TB/s HBM peak
(bytes of the stored rows the launch reads / time). The fp16 instantiations are those of ls_scan.hip and ls_ivf.hip, which
this dtype leaves as they were. Nothing is gated: the numbers are reported."""
import argparse
import sys
from pathlib import Path

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent))
ap.add_argument("--rows", type=int, default=200_000)
ap.add_argument("--dims", default="384,1024")
ap.add_argument("--nlist", type=int, default=447)
ap.add_argument("--nprobe", type=int, default=64)
ap.add_argument("--k", type=int, default=50)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--warm", type=int, default=20)
ap.add_argument("--out", default="")
args = ap.parse_args()
sys.path.insert(0, str(Path(args.root).resolve()))

from lean_explore_amd import native  # noqa: E402
from lean_explore_amd.id_selectors import SearchParametersIVF  # noqa: E402
from lean_explore_amd.index import FlatIPIndex  # noqa: E402
from lean_explore_amd.ivf import IVFFlatIndex  # noqa: E402

HBM_PEAK = 8.0e12
lines = []


def say(text):
    lines.append(text)
    print(text, flush=True)


def series(serve, names):
    """serve[name]() -> kernel ms of one call; the names served in turn, `warm` rounds dropped."""
    out = {n: [] for n in names}
    for rep in range(args.warm + args.calls):
        for n in names:
            ms = serve[n.split("#")[0]]()
            if rep >= args.warm:
                out[n].append(ms)
    return {n: np.array(v) for n, v in out.items()}


def report(what, d, got, bytes_read):
    a, b, c = (float(np.median(got[n])) for n in ("f16#1", "bf16", "f16#2"))
    f16 = 0.5 * (a + c)
    say(f"{what} d={d}: fp16 {a * 1e3:.2f} us / {c * 1e3:.2f} us (two series, spread {abs(a - c) / f16 * 100:.2f} %), "
        f"bf16 {b * 1e3:.2f} us, ratio bf16 / fp16 {b / f16:.4f}, HBM share fp16 {bytes_read / (f16 * 1e-3) / HBM_PEAK:.3f} "
        f"bf16 {bytes_read / (b * 1e-3) / HBM_PEAK:.3f} ({bytes_read / 1e6:.1f} MB read)")


say(f"{native.version()}; rows {args.rows}, k {args.k}, {args.calls} calls after {args.warm}, one query per call")
for d in [int(v) for v in args.dims.split(",")]:
    rng = np.random.default_rng(7 + d)
    x = rng.standard_normal((args.rows, d), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = rng.standard_normal((1, d), dtype=np.float32)
    # (a stored 2-byte row: the first of the eight geometries that holds d elements - ls_pick_geom)
    row_bytes = 16 * next(c for c in (16, 32, 48, 64, 96, 128, 192, 256) if c * 8 >= d)
    # ---- flat ----
    flat = {t: FlatIPIndex.from_array(x, dtype=t) for t in ("f16", "bf16")}
    serve = {}
    for t, ix in flat.items():
        ix.set_profiling(True)
        serve[t] = (lambda ix=ix: (ix.search(q, args.k), ix.last_kernel_ms()[0])[1])
    report("flat", d, series(serve, ("f16#1", "bf16", "f16#2")), args.rows * row_bytes)
    for ix in flat.values():
        ix.close()
    # ---- IVF: nlist centroids drawn from the rows, the library's own assignment, nprobe lists probed ----
    cent = np.ascontiguousarray(x[rng.choice(args.rows, args.nlist, replace=False)])
    ivf, serve, probed = {}, {}, {}
    for t in ("f16", "bf16"):
        v = IVFFlatIndex(d, args.nlist, dtype=t)
        v.set_centroids(cent)
        v.add(x)
        v.set_profiling(True)
        p = SearchParametersIVF(nprobe=args.nprobe)
        serve[t] = (lambda v=v, p=p: (v.search(q, args.k, params=p), v.last_kernel_ms()[1])[1])
        ivf[t] = v
    sizes = ivf["f16"].list_sizes()
    _, lists = FlatIPIndex.from_array(cent).search(q, args.nprobe)
    rows_probed = int(sizes[lists[0][lists[0] >= 0]].sum())
    report(f"ivf nlist={args.nlist} nprobe={args.nprobe} ({rows_probed} rows probed)", d,
           series(serve, ("f16#1", "bf16", "f16#2")), rows_probed * row_bytes)
    for v in ivf.values():
        v.close()

if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
    print("written", args.out, flush=True)
