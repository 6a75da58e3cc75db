"""What tests/test_ivf_batch_cpu.py and tests/test_ivf_batch_gpu.py share: the corpora and explicit lists of the GPU
cases (built on the host, so that the CPU test can hold the plan to every one of them), and a numpy model of the union
step of csrc/ls_ivf_batch.hip (masks, prefix, position -> (storage row, original row, mask))."""

from functools import lru_cache

import numpy as np

MIN_ROWS = 4096       # LS_MQ_MIN_ROWS
MAX_NLIST = 4096      # LS_IVF_BATCH_MAX_NLIST
GROUP = 16            # LS_MQ_NQ

DIMS = (64, 128, 192, 256, 384, 512, 768, 1024)
GEO_N, GEO_NLIST, GEO_NPROBE, GEO_K = 10_000, 40, 8, 10
GEO_NQS = (2, 3, 16, 17, 33)


def groups(nq):
    """Sizes of the groups of >= 2 queries a call of nq queries is cut into (a lone rest takes the chain)."""
    out, left = [], nq
    while left >= 2:
        out.append(min(left, GROUP))
        left -= out[-1]
    return out


def host_assign(corpus, cent):
    """Explicit lists computed on the host (any assignment is a legal index): the centroid of largest inner product."""
    return np.argmax(corpus @ cent.T, axis=1).astype(np.int32)


def layout(assign, nlist):
    """(sizes [nlist], off [nlist + 1], ids [n]: storage row -> original row) of ls_ivf_create's counting sort."""
    sizes = np.bincount(assign, minlength=nlist).astype(np.int64)
    off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    ids = np.argsort(assign, kind="stable").astype(np.int64)
    return sizes, off, ids


def top_rows(sizes, nprobe):
    """Rows of the nprobe largest lists: what one query probes at most."""
    return int(np.sort(sizes)[::-1][:nprobe].sum())


def union_model(probe, off, ids):
    """probe: int [g, nprobe] list numbers (-1: none). Returns (lmask [nlist], lpre [nlist + 1], urow, uid, umask), the
    three arrays padded with mask 0 to a whole tile of 16 (an empty union: one such tile)."""
    nlist = off.shape[0] - 1
    lmask = np.zeros(nlist, dtype=np.uint32)
    for qi in range(probe.shape[0]):
        for l in probe[qi]:
            if 0 <= l < nlist:
                lmask[l] |= np.uint32(1 << qi)
    sizes = np.where(lmask != 0, off[1:] - off[:-1], 0)
    lpre = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    m = int(lpre[-1])
    end = max((m + 15) // 16 * 16, 16)
    urow = np.zeros(end, dtype=np.int64)
    uid = np.zeros(end, dtype=np.int64)
    umask = np.zeros(end, dtype=np.uint32)
    for l in np.flatnonzero(lmask):
        p0, cnt = lpre[l], off[l + 1] - off[l]
        urow[p0:p0 + cnt] = np.arange(off[l], off[l + 1])
        uid[p0:p0 + cnt] = ids[off[l]:off[l + 1]]
        umask[p0:p0 + cnt] = lmask[l]
    return lmask, lpre, urow, uid, umask


# ---- the corpora of the GPU cases ------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def geometry(d):
    """About 10 000 clustered rows of dimension d in 40 uneven lists (tests/test_ivf_gpu.py's mixture), explicit lists."""
    from tests.test_ivf_gpu import mixture, queries

    corpus, cent = mixture(4100 + d, GEO_N, d, GEO_NLIST)
    assign = host_assign(corpus, cent)
    q = queries(91 + d, corpus, max(GEO_NQS))
    return corpus, cent, assign, q


AX_D, AX_NLIST = 64, 16
AX_BIG, AX_TINY = 5, 15  # list 5 holds 5000 rows, list 15 five; the others 1101 + 7 l (no multiple of 16)


def axes_sizes():
    s = np.array([1101 + 7 * l for l in range(AX_NLIST)], dtype=np.int64)
    s[AX_BIG], s[AX_TINY] = 5000, 5
    return s


@lru_cache(maxsize=None)
def axes():
    """Centroids on the coordinate axes e_0 .. e_15 of a 64-dimensional space: a query probes the lists of its largest
    coordinates. Rows are Gaussian in dimensions 16..63 only (they do not decide a probe), dealt to the lists in
    interleaved original-row order except list 5, which also owns the consecutive rows PLANT .. PLANT + 11."""
    rng = np.random.default_rng(515)
    sizes = axes_sizes()
    n = int(sizes.sum())
    assign = np.repeat(np.arange(AX_NLIST, dtype=np.int32), sizes)
    rng.shuffle(assign)
    corpus = np.zeros((n, AX_D), dtype=np.float32)
    corpus[:, AX_NLIST:] = rng.standard_normal((n, AX_D - AX_NLIST), dtype=np.float32)
    cent = np.zeros((AX_NLIST, AX_D), dtype=np.float32)
    cent[np.arange(AX_NLIST), np.arange(AX_NLIST)] = 1.0
    return corpus, cent, assign


def axes_query(rng, lists, weights=None):
    """A query that probes exactly `lists` (in that order) at nprobe = len(lists): coordinates 5, 4, .. on their axes,
    Gaussian in the dimensions the rows live in."""
    q = np.zeros(AX_D, dtype=np.float32)
    q[AX_NLIST:] = rng.standard_normal(AX_D - AX_NLIST, dtype=np.float32)
    for j, l in enumerate(lists):
        q[l] = (weights[j] if weights is not None else 5.0 - j)
    return q


def axes_plant(corpus, assign, q, lists, count, scale):
    """`count` CONSECUTIVE original rows that belong to one of `lists` become the best rows of q (scale x q's row part,
    growing with the row so that they do not tie). Returns (corpus copy, assign copy, first row): the rows are moved
    into lists[0], so they are adjacent in storage as well."""
    corpus, assign = corpus.copy(), assign.copy()
    r0 = corpus.shape[0] // 2
    for j in range(count):
        # swap list membership with a row of lists[0] further on, so that every list keeps its size
        r = r0 + j
        if assign[r] != lists[0]:
            other = r0 + count + int(np.flatnonzero(assign[r0 + count:] == lists[0])[0])
            assign[other], assign[r] = assign[r], lists[0]
        corpus[r] = 0.0
        corpus[r, AX_NLIST:] = np.float32(scale + 0.01 * j) * q[AX_NLIST:]
    return corpus, assign, r0


@lru_cache(maxsize=None)
def ties():
    """Integer-valued rows (scores are exact in fp32): 12 000 rows e_0 * v with v = 3 for four rows, v = 2 for thousands
    (the tie straddles rank 10), else 1; the lists are forced so that the HIGHEST original rows sit in the LOWEST lists:
    union position order contradicts row order."""
    n, d, nlist = 12_000, 64, 8
    rng = np.random.default_rng(77)
    v = np.ones(n, dtype=np.float32)
    v[rng.choice(n, 5000, replace=False)] = 2.0
    v[[1234, 7, 11_000, 6001]] = 3.0
    corpus = np.zeros((n, d), dtype=np.float32)
    corpus[:, 0] = v
    corpus[:, 1] = 1.0
    cent = rng.standard_normal((nlist, d), dtype=np.float32)
    assign = ((n - 1 - np.arange(n)) * nlist // n).astype(np.int32)
    q = np.zeros((4, d), dtype=np.float32)
    q[:, 0] = [1.0, 2.0, 4.0, -1.0]  # (the last query prefers v = 1: thousands tie at its top)
    q[:, 1] = [0.0, 1.0, -2.0, 8.0]
    return corpus, cent, assign, q


def expected_order(scores, rows, k):
    """(score descending, row ascending) top-k of the given (exact) scores."""
    order = np.lexsort((rows, -scores.astype(np.float64)))[:k]
    return scores[order], rows[order]


SMALL_N = 3000        # an index below the row threshold: every group's bound is
K_DECLINED = 2000     # a k the key lists of the geometry corpus decline


def plan_cases():
    """(name, ntotal, rows_q, k, nlist, group, served) of every launch the GPU tests expect: the CPU test runs the
    host plan over them at 256 CUs."""
    out = []
    for d in DIMS:
        _, _, assign, _ = geometry(d)
        rq = top_rows(layout(assign, GEO_NLIST)[0], GEO_NPROBE)
        for g in sorted({g for nq in GEO_NQS for g in groups(nq)}):
            out.append((f"geometry d={d}", GEO_N, rq, GEO_K, GEO_NLIST, g, True))
        out.append((f"geometry d={d} k declined", GEO_N, rq, K_DECLINED, GEO_NLIST, 2, False))
        out.append((f"geometry d={d} all lists", GEO_N, GEO_N, GEO_K, GEO_NLIST, 5, True))
    sizes = axes_sizes()
    n = int(sizes.sum())
    for nprobe, g in ((2, 2), (1, 16), (1, 2), (3, 3)):
        out.append((f"axes nprobe={nprobe}", n, top_rows(sizes, nprobe), 10, AX_NLIST, g, True))
    tn = ties()[0].shape[0]
    out.append(("ties", tn, tn, 10, 8, 4, True))
    out.append(("small index", SMALL_N, SMALL_N, 10, 8, 2, False))
    return out
