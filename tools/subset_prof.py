#!/usr/bin/env python
"""100 single-query searches over 200 k x 384 f32 (k = 50): plain ls_search, or ls_search_subset over a random subset of
the given fraction. The driver of the rocprofv3 records in profiles/ab/subset_search.txt, one run per case, counters
in runs of their own:
    rocprofv3 --kernel-trace --stats -d OUT/kt_F -o run -- python tools/subset_prof.py F     (F = plain, 1.0, 0.1, 0.01)
    rocprofv3 --pmc FETCH_SIZE -d OUT/pmc_F -o run -- python tools/subset_prof.py F"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from lean_explore_amd import faiss_compat as fc  # noqa: E402
from lean_explore_amd.index import FlatIPIndex  # noqa: E402

n, d, k = 200_000, 384, 50
rng = np.random.default_rng(1)
corpus = rng.standard_normal((n, d), dtype=np.float32)
q = rng.standard_normal((1, d), dtype=np.float32)
ix = FlatIPIndex.from_array(corpus)
which = sys.argv[1] if len(sys.argv) > 1 else "plain"
if which == "plain":
    for _ in range(100):
        ix.search(q, k)
else:
    sub = ix.subset(rng.random(n) < float(which))
    p = fc.SearchParameters(sel=sub)
    for _ in range(100):
        ix.search(q, k, params=p)
print(which, "done")
