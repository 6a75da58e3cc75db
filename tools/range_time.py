"""Range search against top-k search of the same handle: what `range_search` costs beside `search(k = 50)`.

One process per shape (this script starts itself once per shape and collects the lines); inside a process the compared
calls are interleaved in bursts of synchronous host calls, one query per call:
  - search(k = 50);
  - range_search at the radius that gives about 50 hits (the 51st score of a prior search);
  - range_search at the radius that gives about 1 % of the rows (the 2001st score of a prior search, 200 k rows);
  - range_search at radius -inf (every probeable row comes back).
For each it prints the host p50 over all calls (us) and the bursts' mean [min .. max], and for the range calls the
hipEvent time of count + offsets + emit alone (ls_range_kernel_ms with profiling on, mean of 5 calls). Results are checked
before anything is timed: the ~50-hit range result must equal search(k = 100) filtered by D > radius and sorted by row.
Shapes: C2 (200 k x 384 f32), C2' (200 k x 1024 f32), and the IVF handle of C2 (nlist 447, nprobe 64).
No gate: there is no range call before this one to compare against. The record goes to profiles/ab/range_search.txt.

    python tools/range_time.py     (RT_SHAPES=0,1,2 RT_REPEATS=5 RT_CALLS=40)
"""
import ctypes
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = (("C2 flat", 200_000, 384, False), ("C2' flat", 200_000, 1024, False), ("C2 IVF nlist 447 nprobe 64", 200_000, 384, True))
NLIST, NPROBE = 447, 64
REPEATS = int(os.environ.get("RT_REPEATS", "5"))
CALLS = int(os.environ.get("RT_CALLS", "40"))
OUT = ROOT / "profiles" / "ab" / "range_search.txt"


def child(which):
    import numpy as np
    import torch

    from lean_explore_amd import native
    from lean_explore_amd.index import FlatIPIndex
    from lean_explore_amd.ivf import IVFFlatIndex
    from tests.test_ivf_gpu import mixture, queries

    name, n, d, is_ivf = SHAPES[which]
    corpus, cent = mixture(1000 + n + d, n, d, NLIST)
    q = queries(77 + d, corpus, 1)
    if is_ivf:
        ix = IVFFlatIndex(d, NLIST)
        ix.set_centroids(cent)
        ix.add(corpus)
        ix.nprobe = NPROBE
    else:
        ix = FlatIPIndex.from_array(corpus)
    del corpus
    lib = native.load()
    print(f"{name}: N={n} d={d} f32, one query per call, device {torch.cuda.get_device_name(0)}; "
          f"{REPEATS} bursts of {CALLS} synchronous calls per mode, interleaved", flush=True)
    Dk, Ik = ix.search(q, 2001, normalize=True)
    r50, r1pct = float(Dk[0, 50]), float(Dk[0, 2000])
    D100, I100 = ix.search(q, 100, normalize=True)
    lims, Dr, Ir = ix.range_search(q, r50, normalize=True)
    ok = (I100[0] >= 0) & (D100[0] > np.float32(r50))
    order = np.argsort(I100[0][ok])
    assert np.array_equal(Ir, I100[0][ok][order]) and np.array_equal(Dr, D100[0][ok][order]), "range != filtered top-k"
    modes = [("search(k=50)", lambda: ix.search(q, 50, normalize=True), None)]
    for label, radius in ((f"range ~50 hits (radius {r50:.6f})", r50), (f"range ~1 % (radius {r1pct:.6f})", r1pct),
                          ("range -inf", float("-inf"))):
        modes.append((label, (lambda r=radius: ix.range_search(q, r, normalize=True)), radius))
    for _, call, _ in modes:  # warm-up (the result buffers grow here, not in the timed calls)
        for _ in range(5):
            call()
    bursts = {label: [] for label, _, _ in modes}
    every = {label: [] for label, _, _ in modes}
    for _ in range(REPEATS):
        for label, call, _ in modes:
            t = []
            for _ in range(CALLS):
                t0 = time.perf_counter()
                call()
                t.append((time.perf_counter() - t0) * 1e6)
            bursts[label].append(float(np.mean(t)))
            every[label] += t
    # the compaction's launches alone, by the library's events
    ix.set_profiling(True)
    h = ix._handle
    kern = {}
    for label, _, radius in modes[1:]:
        ms, hits = [], 0
        for _ in range(5):
            res = ctypes.c_void_p()
            if is_ivf:
                rc = lib.ls_ivf_range_search(h, native.addr(q), 1, radius, NPROBE, native.LS_FLAG_NORMALIZE, ctypes.byref(res))
            else:
                rc = lib.ls_range_search(h, native.addr(q), 1, radius, native.LS_FLAG_NORMALIZE, ctypes.byref(res))
            native.check(rc)
            ms.append(float(lib.ls_range_kernel_ms(res)))
            hits = int(ctypes.c_int64.from_address(lib.ls_range_lims(res) + 8).value)
            lib.ls_range_free(res)
        kern[label] = (float(np.mean(ms)) * 1e3, hits)
    ix.set_profiling(False)
    base = float(np.median(every[modes[0][0]]))
    for label, _, radius in modes:
        b = np.array(bursts[label])
        line = (f"  {label:42s} host p50 {np.median(every[label]):8.1f} us  bursts {b.mean():8.1f} [{b.min():7.1f} .. "
                f"{b.max():7.1f}]")
        if radius is not None:
            us, hits = kern[label]
            line += f"  hits {hits:7d}  count + offsets + emit {us:6.1f} us  vs search(k=50) {np.median(every[label]) - base:+7.1f} us"
        print(line, flush=True)
    ix.close()


def main():
    which = os.environ.get("RT_SHAPES", "0,1,2").split(",")
    lines = []
    for w in which:
        p = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--shape", w], capture_output=True, text=True,
                           timeout=900)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        lines.append(p.stdout.rstrip("\n"))
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            sys.exit(p.returncode)
    OUT.parent.mkdir(parents=True, exist_ok=True)
    OUT.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--shape":
        child(int(sys.argv[2]))
    else:
        main()
