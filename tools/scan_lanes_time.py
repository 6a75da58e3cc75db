"""Pipelined scan-path steps on two lanes vs one stream (debug option 24 = 1 / 0; --force: 2 / 0, two lanes
whatever the corpus size - the default keeps corpora under 240 MiB on one stream), one process, one handle per shape:
interleaved bursts of 2000 pipelined steps, 7 per mode, device us per step from an event pair around each burst
(the closing check inside it), wall clock next to it. Prints median [min .. max] per mode and the verdict the
lanes are held to: c2 must gain 1.5 us with disjoint ranges, no other shape may lose more than its own one-stream
spread.

    python tools/scan_lanes_time.py                 # every shape
    python tools/scan_lanes_time.py c2 c2x8         # some
    python tools/scan_lanes_time.py --blocks 384,448,512,640,896   # c2, lanes on: workgroups per launch (option 7)
"""
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from lean_explore_amd.index import FlatIPIndex  # noqa: E402
from tests import helpers as H  # noqa: E402

SHAPES = {  # label: n, d, dtype, nq, k
    "c2": (200_000, 384, "f32", 1, 50),
    "c2p": (200_000, 1024, "f32", 1, 1000),
    "c2m": (1_000_000, 384, "f32", 1, 50),
    "c2x8": (200_000, 384, "f32", 8, 50),
    "c2px8": (200_000, 1024, "f32", 8, 1000),
    "c2x32": (200_000, 384, "f32", 32, 50),
    "fp16": (200_000, 384, "f16", 1, 50),
}
STEPS, BURSTS, RING = 2000, 7, 256
LANES_ON = 1


def burst(ix, tq, outs, nq, k, steps=STEPS):
    """(device, wall, host queueing) us per step of `steps` pipelined calls and the check that closes them."""
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev0.record()
    for j in range(steps):
        o = outs[j % RING]
        ix.search_device(tq[j % 4], k, o[0], o[1], pipeline=True)
    host = (time.perf_counter() - t0) / steps * 1e6  # (queueing alone; it includes the library's own check every 256 launches)
    ix.check()
    ev1.record()
    ev1.synchronize()
    wall = (time.perf_counter() - t0) / steps * 1e6
    return ev0.elapsed_time(ev1) / steps * 1e3, wall, host


def fmt(xs):
    return f"{statistics.median(xs):7.2f} [{min(xs):7.2f} .. {max(xs):7.2f}]"


def build(label):
    n, d, dtype, nq, k = SHAPES[label]
    ix = FlatIPIndex.from_array(H.gauss(1234, n, d), dtype=dtype)
    q = torch.from_numpy(H.gauss(5678, max(nq, 4), d)).cuda()
    tq = [q.roll(r, dims=0)[:nq].contiguous() for r in range(4)]
    outs = [(torch.empty((nq, k), dtype=torch.float32, device="cuda"),
             torch.empty((nq, k), dtype=torch.int64, device="cuda")) for _ in range(RING)]
    return ix, tq, outs, nq, k


def ab(label):
    ix, tq, outs, nq, k = build(label)
    dev = {0: [], 1: []}
    wall = {0: [], 1: []}
    host = {0: [], 1: []}
    for mode in (0, 1):  # warm both modes (clocks, allocations)
        ix.debug_option(24, mode * LANES_ON)
        burst(ix, tq, outs, nq, k, 500)
    lanes0 = ix.debug_counter(35)
    for _ in range(BURSTS):
        for mode in (0, 1):
            ix.debug_option(24, mode * LANES_ON)
            a, b, c = burst(ix, tq, outs, nq, k)
            dev[mode].append(a)
            wall[mode].append(b)
            host[mode].append(c)
    lane_launches = ix.debug_counter(35) - lanes0
    served_again = ix.debug_counter(25)
    ix.close()
    off, on = statistics.median(dev[0]), statistics.median(dev[1])
    spread = max(dev[0]) - min(dev[0])
    if label == "c2":
        ok = on <= off - 1.5 and (max(dev[1]) < min(dev[0]) or max(dev[0]) < min(dev[1]))
        rule = "on <= off - 1.5 us, ranges disjoint"
    else:
        ok = on <= off + spread
        rule = f"on <= off + one-stream spread ({spread:.2f} us)"
    print(f"{label:6s} device us/step  one stream {fmt(dev[0])} | lanes {fmt(dev[1])} | delta {on - off:+6.2f}  "
          f"{'PASS' if ok else 'MISS'} ({rule})", flush=True)
    print(f"{'':6s} wall   us/step  one stream {fmt(wall[0])} | lanes {fmt(wall[1])} | lane launches {lane_launches} "
          f"of {BURSTS * STEPS} | served again {served_again}", flush=True)
    print(f"{'':6s} host queueing us/step  one stream {fmt(host[0])} | lanes {fmt(host[1])}", flush=True)
    return ok


def blocks_sweep(cands):
    ix, tq, outs, nq, k = build("c2")
    ix.debug_option(24, 1)
    burst(ix, tq, outs, nq, k, 500)
    res = {b: [] for b in cands}
    for _ in range(3):
        for b in cands:
            ix.debug_option(7, b)
            burst(ix, tq, outs, nq, k, 300)
            res[b].append(burst(ix, tq, outs, nq, k)[0])
    ix.close()
    for b in cands:
        print(f"c2 lanes on, blocks={b:5d} (0 = automatic): device us/step {fmt(res[b])}", flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--force":
        LANES_ON, args = 2, args[1:]
    if args and args[0] == "--blocks":
        blocks_sweep([0] + [int(x) for x in args[1].split(",")])
    else:
        results = [ab(label) for label in (args or list(SHAPES))]
        sys.exit(0 if all(results) else 1)
