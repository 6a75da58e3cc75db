"""Do consecutive scan launches overlap? Reads the kernel trace of a pipelined run, e.g.

    rocprofv3 --kernel-trace --output-format csv -d out -o t -- python bench.py --workload c2 --steps 2000 \
        --secondary none --no-host-api --no-cpu-baseline
    python tools/scan_lanes_trace.py out/**/t_kernel_trace.csv [kernel-name substring, default ls_scan_kernel]

and prints, over the longest run of back-to-back launches of that kernel: the share of launches that begin before
their predecessor ends, the mean begin-to-begin distance, the mean kernel duration and the queues they ran on.
A share near zero with option 24 on means the two lanes share a hardware queue or wait for each other."""
import csv
import statistics
import sys

path = sys.argv[1]
name = sys.argv[2] if len(sys.argv) > 2 else "ls_scan_kernel"
rows = []
with open(path, newline="") as f:
    for r in csv.DictReader(f):
        if name in r["Kernel_Name"]:
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", "?")))
rows.sort()
# the timed region: the longest stretch without a gap of more than 1 ms between two begins
best, cur = [], []
for r in rows:
    if cur and r[0] - cur[-1][0] > 1_000_000:
        best, cur = (cur if len(cur) > len(best) else best), []
    cur.append(r)
best = cur if len(cur) > len(best) else best
pairs = list(zip(best, best[1:]))
overlap = sum(1 for a, b in pairs if b[0] < a[1])
b2b = [b[0] - a[0] for a, b in pairs]
over_ns = [a[1] - b[0] for a, b in pairs if b[0] < a[1]]
print(f"{name}: {len(rows)} launches in the trace, {len(best)} in the longest back-to-back stretch")
print(f"begin before the predecessor's end: {overlap} of {len(pairs)} = {overlap / max(1, len(pairs)):.3f}"
      + (f" (median overlap {statistics.median(over_ns) / 1e3:.2f} us)" if over_ns else ""))
print(f"begin-to-begin: mean {statistics.mean(b2b) / 1e3:.2f} us, median {statistics.median(b2b) / 1e3:.2f} us")
print(f"kernel duration: mean {statistics.mean(e - s for s, e, _ in best) / 1e3:.2f} us")
queues = {}
for _, _, q in best:
    queues[q] = queues.get(q, 0) + 1
print("queues:", queues)
