"""The selection step (csrc/ls_select_dev.h: lds_topk, general_select, finalize_body) with injected scores and key
lists, bit for bit against tests/selection_cases.ref_topk. Three injectors put chosen numbers in front of it:

* merge : ls_merge_topk is lds_topk on 256 threads over a key list written here;
* dense : a FlatIPIndex whose corpus is zero except column 0 = s, asked a * e0, scores exactly a * s[r] (every other
          product is 0 * 0, so any summation order and the FMA path give the same bits); debug options 0, 1, 7 and 9
          choose the path and counters 0, 1 and 20 name it;
* BM25  : a BM25Index whose arrays are set by hand scores document r as (0 + s[r]) + shift in float32, and
          get_scores_host is the float32 reference in the same order.

tests/test_selection_cpu.py shows that ref_topk is the oracle's answer on these inputs and that the merge cases reach
every path of lds_topk. The 1024-thread variant of the fourth row-half pass (tied rows >= 2^24 inside one shard) is
the one piece no test here runs: it would need a 16.7 M-row index.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

from lean_explore_amd import native
from lean_explore_amd.bm25 import BM25Index
from lean_explore_amd.index import FlatIPIndex
from oracle import oracle
from tests import selection_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _ieee_denormals():
    """The host references must see the denormals the GPU sees (selection_cases.ieee_denormals)."""
    with C.ieee_denormals():
        assert C.denormals_are_seen()
        yield


def assert_bits(D, I, Dr, Ir, what=""):
    assert C.bits_equal(D, I, Dr, Ir), f"{what}: {C.first_difference(np.asarray(D), np.asarray(I), Dr, Ir)}"


# =============================================================================================== merge injector
MERGE_CASES = {c["id"]: c for c in C.merge_cases()}


def run_merge(S, R, strided=False):
    """ls_merge_topk (or its strided form over the packed exchange layout) on [n_lists, nq, k] host arrays."""
    import torch

    n_lists, nq, k = S.shape
    dev = torch.device("cuda:0")
    So = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    Io = torch.zeros((nq, k), dtype=torch.int64, device=dev)
    lib = native.load()
    stream = torch.cuda.current_stream().cuda_stream
    if not strided:
        tS, tR = torch.from_numpy(S).to(dev), torch.from_numpy(R).to(dev)
        rc = lib.ls_merge_topk(tS.data_ptr(), tR.data_ptr(), n_lists, nq, k, So.data_ptr(), Io.data_ptr(), 0, stream)
    else:  # per list [scores | pad to 8 bytes | rows]
        sbytes = (nq * k * 4 + 7) & ~7
        block = sbytes + nq * k * 8
        packed = np.zeros((n_lists, block), np.uint8)
        for l in range(n_lists):
            packed[l, : nq * k * 4] = S[l].reshape(-1).view(np.uint8)
            packed[l, sbytes:] = R[l].reshape(-1).view(np.uint8)
        tP = torch.from_numpy(packed).to(dev)
        rc = lib.ls_merge_topk_strided(tP.data_ptr(), tP.data_ptr() + sbytes, block, n_lists, nq, k, So.data_ptr(),
                                       Io.data_ptr(), 0, stream)
    if rc != native.LS_OK:
        return rc, None, None
    torch.cuda.synchronize()
    return rc, So.cpu().numpy(), Io.cpu().numpy()


def merge_ref(S, R):
    n_lists, nq, k = S.shape
    out = [C.ref_topk(S[:, qi].reshape(-1), R[:, qi].reshape(-1), k) for qi in range(nq)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@pytest.mark.parametrize("case_id", list(MERGE_CASES))
def test_merge(case_id):
    S, R = C.build_merge_case(MERGE_CASES[case_id])
    rc, D, I = run_merge(S, R)
    assert rc == native.LS_OK
    assert_bits(D, I, *merge_ref(S, R), what=case_id)


# one case per main path of lds_topk (tests/test_selection_cpu.py names the path of every case)
@pytest.mark.parametrize("case_id", ["4x16-gauss-interleaved-identity", "3x1000-gauss-interleaved-identity",
                                     "16x256-gauss-interleaved-identity", "8x1000-all_equal-interleaved-bit24"])
def test_merge_strided(case_id):
    S, R = C.build_merge_case(MERGE_CASES[case_id])
    rc, D, I = run_merge(S, R, strided=True)
    assert rc == native.LS_OK
    assert_bits(D, I, *merge_ref(S, R), what=case_id)


@pytest.mark.parametrize("n_lists,k", [(5, 2048), (1, 2049)])
def test_merge_refuses_what_lds_cannot_hold(n_lists, k):
    S = np.zeros((n_lists, 1, k), np.float32)
    R = np.arange(n_lists * k, dtype=np.int64).reshape(n_lists, 1, k)
    rc, _, _ = run_merge(S, R)
    assert rc == native.LS_ERR_K_TOO_LARGE


# =============================================================================================== dense injector
N_DENSE, D_DENSE = 24_576, 64
KS = (1, 50, 256, 257, 1000, 2048)
SCALES = (1.0, -1.0, 0.5)  # three different rankings per index


def one_hot_index(s, dtype="f32", d=D_DENSE):
    corpus = np.zeros((s.size, d), np.float32)
    corpus[:, 0] = s
    return FlatIPIndex.from_array(corpus, dtype=dtype)


def one_hot_queries(scales, d=D_DENSE):
    q = np.zeros((len(scales), d), np.float32)
    q[:, 0] = scales
    return q


class DenseRef:
    """ref_topk of a * s for every query scale, sorted once: the top k of any k <= LS_MAX_K is a prefix."""

    def __init__(self, s, scales=SCALES):
        with np.errstate(invalid="ignore", over="ignore"):
            self.scores = np.asarray(scales, np.float32)[:, None] * s[None, :]
        self.D, self.I = C.ref_topk_batch(self.scores, np.arange(s.size), min(C.LS_MAX_K, s.size))

    def top(self, k, qi=None):
        sel = slice(None) if qi is None else slice(qi, qi + 1)
        D = np.full((self.D[sel].shape[0], k), C.NEG_FLT_MAX, np.float32)
        I = np.full(D.shape, -1, np.int64)
        m = min(k, self.D.shape[1])
        D[:, :m], I[:, :m] = self.D[sel, :m], self.I[sel, :m]
        return D, I


def dense_vectors():
    out = {name: C.score_vector(name, N_DENSE, 5) for name in C.SCORES}
    for k in (50, 257, 2048):
        for where in C.TWO_VALUES_AT:
            out[f"two_values-{where}-k{k}"] = C.two_values_for_k(N_DENSE, 5, k, where)
    for m in (0, 49, 50, 51, 256, 257, 258):
        out[f"invalid-{m}valid"] = C.invalid(N_DENSE, 5, valid=m)
    return out


DENSE_NAMES = sorted(dense_vectors())


@functools.lru_cache(maxsize=None)
def dense_vector(name):
    return dense_vectors()[name]


def device_search(ix, q, k):
    import torch

    s, i = ix.search_device(torch.from_numpy(q).cuda(), k, asynchronous=True)
    ix.check()
    return s.cpu().numpy(), i.cpu().numpy()


def run_routes(ix, ref, k, what, routes=("host", "host_own_launch", "device1", "device3")):
    """The entry routes of one (index, k): (i) search, one query per call - the selection rides on the scan launch;
    (ii) the same with option 9 = 0 - its own launch; (iii) search_device(asynchronous) + check, one query and three -
    the piggy-backed 256-thread job with a score vector."""
    q = one_hot_queries(SCALES, ix.d)
    for route in routes:
        if route in ("host", "host_own_launch"):
            ix.debug_option(9, 1 if route == "host" else 0)
            try:
                for qi in range(len(SCALES)):
                    D, I = ix.search(q[qi:qi + 1], k)
                    assert_bits(D, I, *ref.top(k, qi), what=f"{what} k={k} {route} a={SCALES[qi]}")
            finally:
                ix.debug_option(9, 1)
        elif route == "device1":
            for qi in range(len(SCALES)):
                D, I = device_search(ix, q[qi:qi + 1], k)
                assert_bits(D, I, *ref.top(k, qi), what=f"{what} k={k} {route} a={SCALES[qi]}")
        else:
            D, I = device_search(ix, q, k)
            assert_bits(D, I, *ref.top(k), what=f"{what} k={k} {route}")


@pytest.mark.parametrize("name", DENSE_NAMES)
def test_dense_routes(name):
    s = dense_vector(name)
    ix = one_hot_index(s)
    try:
        ref = DenseRef(s)
        for k in KS:
            run_routes(ix, ref, k, name)
    finally:
        ix.close()


@pytest.mark.parametrize("name", C.F16_EXACT)
def test_dense_routes_f16(name):
    s = C.score_vector(name, N_DENSE, 5)
    assert np.array_equal(s.astype(np.float16).astype(np.float32), s)
    ix = one_hot_index(s, dtype="f16")
    try:
        ref = DenseRef(s)
        for k in KS:
            run_routes(ix, ref, k, name + "/f16")
    finally:
        ix.close()


class Counters:
    def __init__(self, ix, which=(0, 1, 20)):
        self.ix, self.which = ix, which
        self.at = {w: ix.debug_counter(w) for w in which}

    def delta(self):
        now = {w: self.ix.debug_counter(w) for w in self.which}
        d = {w: now[w] - self.at[w] for w in self.which}
        self.at = now
        return d


def restore(ix):
    for opt, val in ((0, 0), (1, 0), (7, 0), (9, 1)):
        ix.debug_option(opt, val)
    ix.close()


@pytest.mark.parametrize("name", DENSE_NAMES)
def test_dense_forced_general(name):
    """Option 1: general_select's four passes over S have their own digit logic - every score vector, among them
    `invalid` with fewer than k valid rows and `two_values` with the boundary inside the tie class."""
    s = dense_vector(name)
    ix = one_hot_index(s)
    try:
        ref = DenseRef(s)
        ix.debug_option(1, 1)
        for k in (1, 50, 257, 2048):
            c = Counters(ix)
            run_routes(ix, ref, k, name + "/general", routes=("host", "device3"))
            d = c.delta()
            assert d[0] == 6 and d[1] == 6, (k, d)  # 3 host calls + 3 queries of the device call, all general
    finally:
        restore(ix)


def shuffled_distinct(seed=3):
    return C.ascending(N_DENSE, 0)[np.random.default_rng(seed).permutation(N_DENSE)]


def test_dense_fast_path():
    """Automatic k', shuffled distinct scores: the emitted keys prove the result, nothing leaves the fast path."""
    s = shuffled_distinct()
    ix = one_hot_index(s)
    try:
        ref = DenseRef(s)
        c = Counters(ix)
        for k in (1, 50, 256):
            run_routes(ix, ref, k, "fast")
        d = c.delta()
        assert d[0] == 0 and d[1] == 0 and d[20] == 0, d
    finally:
        restore(ix)


def scan_tile_rows():
    """Rows per tile of the f32 scan at d = D_DENSE (csrc/ls_scan_plan.h: scan_unroll, ls_scan_tile_rows)."""
    L, V = oracle.geom_f32(D_DENSE)
    return (4 if V >= 3 else 8) * (64 // L)


def workgroup_of_row(rows, tile_rows, blocks):
    """csrc/ls_scan_kernel.h: tile t (tile_rows contiguous rows) goes to wave t mod (4 * blocks); a workgroup's four
    waves take four adjacent tiles. So "sorted by row" is not "clustered in a workgroup"."""
    return ((rows // tile_rows) % (4 * blocks)) // 4


def auto_kprime(k, blocks):
    """ls_kprime (csrc/ls_scan_plan.h) for the scan kernel: lambda + 5 sqrt(lambda) + 3, within [2, 15]."""
    lam = k / blocks
    kp = min(max(int(lam + 5.0 * np.sqrt(lam) + 3.0), 2), 15)
    while kp > 1 and blocks * kp > C.LS_FINAL_CAP:
        kp -= 1
    return kp


def scan_model(sc, k, blocks, kprime=None):
    """What finalize_body does with the keys a single-query scan launch emits for the DISTINCT valid scores `sc`:
    ("fast" | "rescue" | "general", rows the rescue sweep collects). Each workgroup emits its k' best rows and the
    next one as its bound; T is the k-th best emitted key; the proof holds iff every bound is below T - i.e. iff no
    workgroup holds more than k' of the top k. Else the sweep collects the rows at or above T, and general_select
    answers if they do not fit the job's keys (the smallest capacity of any route: max(256, blocks * k'))."""
    kp = kprime or auto_kprime(k, blocks)
    if blocks * kp < k:
        return "general", 0
    rank = np.empty(sc.size, np.int64)
    rank[np.argsort(-sc.astype(np.float64), kind="stable")] = np.arange(sc.size)
    wg = workgroup_of_row(np.arange(sc.size), scan_tile_rows(), blocks)
    emitted, bounds = [], []
    for b in range(blocks):
        r = np.sort(rank[wg == b])
        emitted.append(r[:kp])
        bounds.extend(r[kp:kp + 1])
    T = np.sort(np.concatenate(emitted))[k - 1]  # as a rank: smaller is better
    if min(bounds, default=sc.size) > T:
        return "fast", 0
    return ("rescue" if T + 1 <= max(256, blocks * kp) else "general"), int(T + 1)


SINGLE_ROUTES = ("host", "host_own_launch", "device1")  # one query per scan launch: scan_model's subject


def run_modelled(ix, ref, k, blocks, kprime, what, want=None):
    """Every single-query route at (k, blocks, k'), the results bit for bit and, per route, the exact rise of counters
    0 and 1 that scan_model names for the three query scales. `want`: the outcomes the case was built for."""
    got = [scan_model(sc, k, blocks, kprime)[0] for sc in ref.scores]
    if want is not None:
        assert got == list(want), (what, k, got)
    for route in SINGLE_ROUTES:
        c = Counters(ix)
        run_routes(ix, ref, k, what, routes=(route,))
        d = c.delta()
        assert (d[0], d[1]) == (sum(g != "fast" for g in got), sum(g == "general" for g in got)), (what, k, route, got, d)
    return got


def dealt_scores(blocks, extra_for_wg0=None):
    """Distinct scores whose rank r (best first) lies in scan workgroup r mod blocks, at a shuffled row of it: ANY k
    best - and, the same way, any k worst, which are the best of the query -e0 - are spread over the workgroups to
    within one row. extra_for_wg0 = (r_in, r_out): the scores of ranks r_in and r_out (a row of workgroup 0) change
    places, so workgroup 0 holds one row more of every top k with r_in < k <= r_out."""
    wg = workgroup_of_row(np.arange(N_DENSE), scan_tile_rows(), blocks)
    rng = np.random.default_rng(blocks)
    rows_of = [rng.permutation(np.flatnonzero(wg == b)) for b in range(blocks)]
    assert all(r.size == N_DENSE // blocks for r in rows_of)
    r = np.arange(N_DENSE)
    row_of_rank = np.array([rows_of[i % blocks][i // blocks] for i in r])
    by_rank = C.descending(N_DENSE, 0)
    if extra_for_wg0:
        r_in, r_out = extra_for_wg0
        assert r_out % blocks == 0 and r_in % blocks != 0
        by_rank = by_rank.copy()
        by_rank[[r_in, r_out]] = by_rank[[r_out, r_in]]
    s = np.empty(N_DENSE, np.float32)
    s[row_of_rank] = by_rank
    return s


@pytest.mark.parametrize("blocks", [32, 64])
def test_dense_prefilter_on_and_off(blocks):
    """The pivot pre-filter of finalize_body runs from 64 scan workgroups up (p.blocks >= 64): option 7 = 64 has it, 32
    does not, and neither do the other dense tests (24 576 rows plan 48 workgroups). (m_need > kprime cannot switch it
    off: the fast path needs blocks * kprime >= k.) Every case asserts the exact rise of counters 0 and 1 per route,
    named by scan_model from the placement of the rows.
      automatic k', shuffled scores, k = 1, 50, 256: the fast path at 64 workgroups; at 32 whatever the model names for
        k = 256 (lambda = 8 against the k' cap of 15);
      k' = 15, dealt scores: k = 257 and k = 15 x blocks stay on the FAST path - every workgroup holds at most 15 of the
        top k, m_need = ceil(k / blocks) is up to 15, the pivot is a workgroup's LAST key, and the returned bits are
        the pre-filter's and lds_topk's own;
      k' = 15, dealt scores with one more top row in workgroup 0: that row is withheld, the proof fails and the rescue
        sweep answers for the scales 1 and 0.5; -e0 ranks from the other end and stays fast."""
    kmax = 15 * blocks
    s = shuffled_distinct(4)
    ix = one_hot_index(s)
    try:
        ref = DenseRef(s)
        ix.debug_option(7, blocks)
        for k in (1, 50):
            run_modelled(ix, ref, k, blocks, None, f"prefilter blocks={blocks}", want=("fast",) * 3)
        got = run_modelled(ix, ref, 256, blocks, None, f"prefilter blocks={blocks}",
                           want=("fast",) * 3 if blocks == 64 else None)
        assert "general" not in got
        if blocks == 64:
            # three queries in one launch go to the f32 matrix-core pass, whose workgroups (four waves over 16-row tiles)
            # emit k' = lambda + 5 sqrt(lambda) + 3 = 17 keys for lambda = 4: none withholds a row of the top 256
            # (P(Poisson(4) > 17) < 1e-6). (At 32 workgroups that call is refused: test_forced_32_workgroups_...)
            c = Counters(ix)
            for k in (1, 50, 256):
                run_routes(ix, ref, k, "prefilter device3", routes=("device3",))
            d = c.delta()
            assert (d[0], d[1]) == (0, 0), d
    finally:
        restore(ix)
    for extra, ks, want in ((None, (257, kmax), ("fast",) * 3),
                            ((kmax - 11, kmax), (kmax - 10,), ("rescue", "fast", "rescue"))):
        s = dealt_scores(blocks, extra)
        ix = one_hot_index(s)
        try:
            ref = DenseRef(s)
            ix.debug_option(7, blocks)
            ix.debug_option(0, 15)
            for k in ks:
                run_modelled(ix, ref, k, blocks, 15, f"prefilter blocks={blocks} k'=15 extra={extra}", want=want)
        finally:
            restore(ix)


def test_forced_32_workgroups_refuse_a_three_query_device_call():
    """DESIGN.md 10.7, a known defect of the fp32 small-batch route that is left as it is: with 32 forced workgroups
    the 32-query plan grants a pass at k = 256 that the 2..16-query plan then declines, and the call is refused before
    any selection runs. Pinned so that a fix - or another message - is noticed; the index keeps answering."""
    import torch

    s = shuffled_distinct(4)
    ix = one_hot_index(s)
    try:
        ref = DenseRef(s)
        ix.debug_option(7, 32)
        q = torch.from_numpy(one_hot_queries(SCALES)).cuda()
        with pytest.raises(ValueError, match=r"ls_launch_mq: bad arguments \(elem 4 nq 3 kprime 0 keys 0\)"):
            ix.search_device(q, 256, asynchronous=True)
        run_routes(ix, ref, 256, "after the refusal", routes=("device1",))
    finally:
        restore(ix)


def test_dense_rescue():
    """Option 0 = 1, 64 workgroups, k = 50: every workgroup emits its best row only, the 50th best of those 64 keys is
    T, and the workgroups' bounds (their second best rows) beat it - the proof fails. About 0.4 % of the rows lie at
    or above T (the 15th lowest of 64 maxima of 384 Gaussians): about 100, within the 256 keys of a piggy-backed job
    and the 8192 of the stand-alone one, so the rescue sweep serves every route."""
    s = C.gauss(N_DENSE, 7)
    ix = one_hot_index(s)
    try:
        ref = DenseRef(s)
        ix.debug_option(0, 1)
        ix.debug_option(7, 64)
        k = 50
        wg = workgroup_of_row(np.arange(N_DENSE), scan_tile_rows(), 64)
        for sc in ref.scores:  # (no score of this vector is invalid under any of the three scales)
            T = np.sort(np.array([sc[wg == b].max() for b in range(64)]))[::-1][k - 1]
            assert k < int((sc >= T).sum()) <= 256
        c = Counters(ix)
        run_routes(ix, ref, k, "rescue", routes=("host",))
        d = c.delta()
        assert d[0] == 3 and d[1] == 0 and d[20] >= 1, d
        run_routes(ix, ref, k, "rescue", routes=("host_own_launch", "device1", "device3"))
        d = c.delta()
        assert d[0] == 9 and d[1] == 0, d
    finally:
        restore(ix)


def test_dense_rescue_overflow_goes_general():
    """Option 0 = 1, 64 workgroups, k = 50 (mc = 64 >= k: the fast path is attempted). Workgroups 0..48 hold the high
    rows, 49..63 the low ones: the 50th best emitted key is the best LOW row, and all 49 x 384 = 18 816 high rows beat
    it - more than LS_FINAL_CAP = 8192: the rescue sweep overflows and general_select answers."""
    wg = workgroup_of_row(np.arange(N_DENSE), scan_tile_rows(), 64)
    assert np.bincount(wg, minlength=64).tolist() == [N_DENSE // 64] * 64
    for a in (1.0, -1.0):
        s = (C.gauss(N_DENSE, 8) + np.where(wg < 49, np.float32(10), np.float32(-10)) * np.float32(a)).astype(np.float32)
        ix = one_hot_index(s)
        try:
            ref = DenseRef(s, (a,))
            ix.debug_option(0, 1)
            ix.debug_option(7, 64)
            q = one_hot_queries((a,))
            c = Counters(ix)
            D, I = ix.search(q, 50)
            assert_bits(D, I, *ref.top(50), what="overflow host")
            d = c.delta()
            assert d[0] == 1 and d[1] == 1, d
            D, I = device_search(ix, q, 50)
            assert_bits(D, I, *ref.top(50), what="overflow device")
            d = c.delta()
            assert d[0] == 1 and d[1] == 1, d
        finally:
            restore(ix)


def test_dense_no_candidates_to_start_from():
    """Option 0 = 1 with k above the workgroup count: mc < keff, the fast path is not attempted."""
    s = shuffled_distinct(5)
    ix = one_hot_index(s)
    try:
        ref = DenseRef(s)
        ix.debug_option(0, 1)
        ix.debug_option(7, 64)
        for k in (65, 257, 2048):
            c = Counters(ix)
            run_routes(ix, ref, k, "mc < keff", routes=("host", "device3"))
            d = c.delta()
            assert d[0] == 6 and d[1] == 6, (k, d)
    finally:
        restore(ix)


# =============================================================================================== BM25 injector
def hand_built_bm25(s, s2):
    """Column a lists every document with data = s, column b every third document with s2, column c is empty."""
    n = s.size
    third = np.arange(0, n, 3, dtype=np.int32)
    ix = BM25Index()
    ix.vocab = {"a": 0, "b": 1, "c": 2}
    ix.indptr = np.array([0, n, n + third.size, n + third.size], np.int64)
    ix.indices = np.concatenate([np.arange(n, dtype=np.int32), third])
    ix.data = np.concatenate([s, s2[: third.size]]).astype(np.float32)
    ix.nonoccurrence = np.array([-1.5, 0.25, 0.0], np.float32)
    ix.num_docs = n
    return ix


BM25_QUERIES = (["a"], ["a", "b"], ["b", "a", "a"], ["c"])
BM25_KS = (1, 50, 1000, 2048)


def check_bm25(ix, ks=BM25_KS, queries=BM25_QUERIES, what=""):
    n = ix.num_docs
    with np.errstate(invalid="ignore", over="ignore"):
        scores = [ix.get_scores_host(q) for q in queries]
    subsets = {"all": np.arange(n), "every7th": np.arange(0, n, 7)}
    subs = {name: ix.subset(docs) for name, docs in subsets.items()}
    try:
        for q, sc in zip(queries, scores):
            for k in ks:
                docs, got = ix.retrieve(q, k)
                Dr, Ir = C.ref_topk(sc, np.arange(n), k)
                assert_bits(got, docs, Dr, Ir, what=f"{what} n={n} q={q} k={k}")
                for name, sel in subsets.items():
                    docs, got = ix.retrieve(q, k, subset=subs[name])
                    Dr, Ir = C.ref_topk(sc[sel], sel, k)
                    assert_bits(got, docs, Dr, Ir, what=f"{what} n={n} q={q} k={k} subset={name}")
    finally:
        for sub in subs.values():
            sub.close()


@pytest.mark.parametrize("n", [1, 3, 5, 255, 257, 2049, 20_000])
def test_bm25_sizes(n):
    ix = hand_built_bm25(C.gauss(n, 1), C.seven_values(n, 2))
    try:
        check_bm25(ix, what="gauss")
    finally:
        ix.close()


@pytest.mark.parametrize("name", ["descending", "ascending", "all_equal", "invalid", "straddle", "seven_values"])
def test_bm25_vectors(name):
    n = 20_000
    ix = hand_built_bm25(C.score_vector(name, n, 3), C.gauss(n, 4))
    try:
        check_bm25(ix, what=name)
    finally:
        ix.close()


def test_bm25_named_paths():
    """n = 20 000 documents: ls_bm25_create plans min(ceil(n / 256), CUs) = 79 -> 72 workgroups (a multiple of 8), rows
    dealt in granules of 4, so each holds ~278 documents and an even share of any run of rows.
    rescue : k = 1000 gives lambda = 13.9 and k' = min(13.9 + 5 sqrt(13.9) + 3, 15) = 15; mc = 1080 >= k, the fast path
             is attempted; with distinct Gaussian scores a workgroup holds Poisson(13.9) of the top 1000, above 15 with
             probability 0.3, so some of the 72 withhold a row of the top 1000, the proof fails, and the sweep finds
             little more than 1000 rows at or above the 1000th emitted key: counter 0 rises, counter 1 does not.
    general: k = 2048 > mc = 72 x 15 = 1080: too few keys were emitted, general_select answers: counter 1 rises.
    fast   : k = 50 gives k' = 0.69 + 4.2 + 3 = 7, and no workgroup holds 8 of the top 50: neither counter moves."""
    n = 20_000
    ix = hand_built_bm25(C.gauss(n, 11), C.seven_values(n, 12))
    try:
        with np.errstate(invalid="ignore"):
            sc = ix.get_scores_host(["a"])
        for k, want in ((50, (0, 0)), (1000, (1, 0)), (2048, (1, 1))):
            before = (ix.debug_counter(0), ix.debug_counter(1))
            docs, got = ix.retrieve(["a"], k)
            assert_bits(got, docs, *C.ref_topk(sc, np.arange(n), k), what=f"k={k}")
            after = (ix.debug_counter(0), ix.debug_counter(1))
            assert (after[0] - before[0], after[1] - before[1]) == want, (k, before, after)
    finally:
        ix.close()


# =============================================================================================== batched select kernels
# The smallest shape of tests/test_batched_gpu.py::test_batched_shapes that the MFMA path serves on both an fp16 and
# an fp32 index (more than 32 queries): n = 40 000, nq = 40, k = 20, d = 600.
B_N, B_NQ, B_K, B_D = 40_000, 40, 20, 600
# a_j = +-2^-j, j kept inside binary16's normal range so that the fp16 index sees the same queries
B_SCALES = tuple((-1.0 if j & 1 else 1.0) * 2.0 ** -(j % 14) for j in range(B_NQ))


def batched_vector(name):
    if name == "two_values":
        return C.two_values_for_k(B_N, 9, B_K, "inside_lower")
    return C.score_vector(name, B_N, 9)


@pytest.mark.parametrize("dtype,path", [("f16", 2), ("f32", 3)])
@pytest.mark.parametrize("name", C.F16_EXACT)
def test_batched_select_kernels(name, dtype, path):
    s = batched_vector(name)
    ix = one_hot_index(s, dtype=dtype, d=B_D)
    try:
        ref = DenseRef(s, B_SCALES)
        q = one_hot_queries(B_SCALES, B_D)
        for opt14 in (1, 0):
            for opt5 in (1, 0):
                ix.debug_option(14, opt14)
                ix.debug_option(5, opt5)
                repaired = ix.debug_counter(8)
                D, I = ix.search(q, B_K)
                assert ix.debug_counter(10) == path, f"left the batched path: counter 10 = {ix.debug_counter(10)}"
                print(f"{name}/{dtype} option14={opt14} option5={opt5}: repaired queries "
                      f"{ix.debug_counter(8) - repaired}")
                assert_bits(D, I, *ref.top(B_K), what=f"{name}/{dtype} option14={opt14} option5={opt5}")
    finally:
        ix.debug_option(14, 1)
        ix.debug_option(5, 1)
        ix.close()
