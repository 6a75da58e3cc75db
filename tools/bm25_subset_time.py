"""Host p50 of BM25 retrieval over a document subset against the full call.

200 000 synthetic names, the bench's BM25 shape (3-token query, k = 1000). One handle; for every row the full call
(`retrieve(q, k)`) and the subset call (`retrieve(q, k, subset=...)`) are interleaved in one process: 5 bursts of 100 calls
each, host p50 per burst. Rows: random subsets of 100 / 50 / 10 / 1 % of the documents and a contiguous 10 % block.
Columns: p50 mean [min .. max] over the bursts for both calls, their ratio, and the rise of debug counters 0 (selection
left the fast path) and 1 (general path) over the subset calls and over the full calls of the row.

Condition reported (not enforced): at the random 10 % subset the subset call's p50 is not above the full call's p50 of the
same run by more than the full call's own burst-to-burst spread (max - min). The all-ones ratio and the 1 % row are
reported only.

    python tools/bm25_subset_time.py [--out profiles/ab/bm25_subset.txt] [--docs 200000] [--k 1000]
"""

from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

BURSTS, CALLS = 5, 100


def names_of(n_docs: int) -> list[str]:
    words = ("add comm assoc zero one mul le lt succ pred map filter append length nil cons sum prod "
             "continuous measurable integral deriv norm inner dist open closed compact").split()
    rng = np.random.default_rng(3)
    names = []
    for i in range(n_docs):
        parts = [words[j] for j in rng.integers(0, len(words), size=rng.integers(1, 5))]
        ns = ["Nat", "List", "Real", "MeasureTheory", "Mathlib"][rng.integers(0, 5)]
        names.append(f"{ns}.{'_'.join(parts)}{i % 97 if i % 3 == 0 else ''}")
    return names


def burst(call) -> float:
    lat = np.empty(CALLS)
    for i in range(CALLS):
        t0 = time.perf_counter()
        call()
        lat[i] = time.perf_counter() - t0
    return float(np.median(lat)) * 1e6


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ab" / "bm25_subset.txt"))
    ap.add_argument("--docs", type=int, default=200_000)
    ap.add_argument("--k", type=int, default=1000)
    args = ap.parse_args()

    from lean_explore_amd import native
    from lean_explore_amd.bm25 import BM25Index
    from lean_explore_amd.search.tokenization import tokenize_spaced

    if native.device_count() < 1:
        print("bm25_subset_time: no HIP device visible; nothing is measured without one", file=sys.stderr)
        return 2
    n, k = args.docs, args.k
    ix = BM25Index().index([list(dict.fromkeys(tokenize_spaced(nm))) for nm in names_of(n)])
    q = ["nat", "add", "comm"]
    rng = np.random.default_rng(11)
    rows = [(f"random {int(f * 100)} %", rng.random(n) < f if f < 1.0 else np.ones(n, dtype=bool))
            for f in (1.0, 0.5, 0.1, 0.01)]
    block = np.zeros(n, dtype=bool)
    block[n // 3: n // 3 + n // 10] = True
    rows.append(("contiguous 10 %", block))

    lines = [f"bm25 subset vs full call: {n} names, query {q}, k = {k}; {BURSTS} bursts x {CALLS} calls, interleaved, "
             "host p50 per burst (us): mean [min .. max]",
             f"{'subset':<16} {'docs':>7}  {'full call':>24}  {'subset call':>24}  {'ratio':>6}  "
             f"{'c0/c1 subset':>12}  {'c0/c1 full':>10}"]
    verdict = None
    for label, mask in rows:
        sub = ix.subset(mask)
        d0, s0 = ix.retrieve(q, k)
        d1, s1 = ix.retrieve(q, k, subset=sub)
        if label.startswith("random 100") and not (np.array_equal(d0, d1) and np.array_equal(s0, s1)):
            print("bm25_subset_time: the all-ones subset differs from the full call", file=sys.stderr)
            return 1
        for _ in range(20):
            ix.retrieve(q, k)
            ix.retrieve(q, k, subset=sub)
        full, part = [], []
        rise = {"full": [0, 0], "sub": [0, 0]}
        for _ in range(BURSTS):
            c = [ix.debug_counter(0), ix.debug_counter(1)]
            full.append(burst(lambda: ix.retrieve(q, k)))
            c2 = [ix.debug_counter(0), ix.debug_counter(1)]
            part.append(burst(lambda: ix.retrieve(q, k, subset=sub)))
            c3 = [ix.debug_counter(0), ix.debug_counter(1)]
            for j in range(2):
                rise["full"][j] += c2[j] - c[j]
                rise["sub"][j] += c3[j] - c2[j]
        fm, pm = float(np.mean(full)), float(np.mean(part))
        lines.append(f"{label:<16} {sub.docs:>7}  {fm:7.1f} [{min(full):6.1f} .. {max(full):6.1f}]  "
                     f"{pm:7.1f} [{min(part):6.1f} .. {max(part):6.1f}]  {pm / fm:6.3f}  "
                     f"{rise['sub'][0]:>5}/{rise['sub'][1]:<6}  {rise['full'][0]:>4}/{rise['full'][1]:<5}")
        if label == "random 10 %":
            spread = max(full) - min(full)
            ok = pm <= fm + spread
            verdict = (f"condition (random 10 %): subset p50 {pm:.1f} us <= full p50 {fm:.1f} us + its burst-to-burst spread "
                       f"{spread:.1f} us: {'MET' if ok else 'MISSED'}")
        sub.close()
    lines.append(verdict or "condition: the random 10 % row did not run")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text)
    ix.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
