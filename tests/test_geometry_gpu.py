"""Every row geometry (L, V) of the scan kernels on the MI355X, per storage dtype and per path: the plain scan and the
row-list (subset) scan in their SMALL and non-SMALL variants, and the IVF probed-list scan with its second launch.

Every comparison is np.array_equal on scores and indices against a host-only reference (tests/test_geometry_cpu.py:
the oracle in the scan kernels' summation order for f32, the strict oracle on integer-valued data for f16,
tests/sq8_ref.c for sq8), except the Gaussian f16 cases, which go through the project's bars (scores within 1e-5, an
index may differ only where the float64 twin's scores are within 2e-6, recall 1.0). Nothing is timed.

Which variant a launch takes is decided on the host (ls_scan_launch in csrc/ls_scan_launch.h, by ls_scan_is_small of
csrc/ls_scan_plan.h):
    SMALL  <=>  one query in the launch  and  tiles_per_wave * TR <= 64  and  blocks <= 256,  TR = scan_unroll(V) * 64 / L
and debug option 7 sets `blocks` (ls_api.hip, ls_subset.hip). The library has no counter that tells the variants apart,
so the tests assert the restated rule (tests/test_geometry_cpu.py::is_small, held to the header by
test_restated_launch_rule_is_the_code_s_own there) for the launches they make: at n = 3001,
option 7 = 4 is non-SMALL and option 7 = 256 is SMALL for every geometry. Calls of several queries on an f32 / f16 index
share one launch (never SMALL), so every plain search also runs query by query."""

import numpy as np
import pytest

from lean_explore_amd import native
from lean_explore_amd.id_selectors import SearchParameters, SearchParametersIVF
from lean_explore_amd.index import FlatIPIndex
from lean_explore_amd.ivf import IVFFlatIndex
from oracle import oracle
from tests import helpers as H
from tests.test_geometry_cpu import (DIMS, GEOMS, IVF_MAX_D, N, NQ, PLAIN_K, PLAIN_OPTS, SUBSET_K, SUBSET_RUNS, Flat,
                                     assert_bars, default_blocks, geom_of, is_small, ivf_dims, ivf_reference,
                                     seen_queries, selections, uneven_assignment)
from tests.test_sq8_cpu import NEG

pytestmark = pytest.mark.gpu

FLAT_CASES = [(dtype, d, "gauss") for dtype in ("sq8", "f32") for d in DIMS[dtype]] + \
             [("f16", d, "int") for d in DIMS["f16"]] + \
             [("f16", max(d for d in DIMS["f16"] if geom_of("f16", d) == g), "gauss") for g in GEOMS["f16"]]
IVF_CASES = [(dtype, d, "gauss") for dtype in ("sq8", "f32") for d in ivf_dims(dtype)] + \
            [("f16", d, "int") for d in ivf_dims("f16")] + \
            [("f16", d, "gauss") for d in ivf_dims("f16")[0::2]]


def test_the_cases_cover_every_geometry():
    for dtype in ("sq8", "f32", "f16"):
        assert {geom_of(dtype, d) for t, d, _ in FLAT_CASES if t == dtype} == set(GEOMS[dtype])
        reachable = {geom_of(dtype, d) for d in range(1, IVF_MAX_D + 1)}
        assert {geom_of(dtype, d) for t, d, _ in IVF_CASES if t == dtype} == reachable
    assert {geom_of("f16", d) for t, d, kind in FLAT_CASES if t == "f16" and kind == "gauss"} == set(GEOMS["f16"])


def make_data(dtype, d, kind, n=N):
    """(corpus, [(queries, normalize)]): integer-valued data runs without normalisation only (it would leave the
    exact regime); Gaussian rows are unit norm, queries 0, 1 are rescaled and run with normalize=True."""
    seed = 7000 + 3 * d + {"sq8": 0, "f32": 1, "f16": 2}[dtype]
    if kind == "int":
        return H.int_corpus(seed, n, d), [(H.int_corpus(seed + 1, NQ, d), False)]
    q = H.gauss(seed + 1, NQ, d)
    q[:2] *= np.float32(2.5)
    return H.gauss(seed, n, d), [(np.ascontiguousarray(q[:2]), True), (np.ascontiguousarray(q[2:]), False)]


class Checker:
    """Exact comparison, or - Gaussian f16 - the project's bars against the float64 twin."""

    def __init__(self, corpus, dtype, kind):
        self.flat, self.corpus, self.bars = Flat(corpus, dtype), corpus, (dtype == "f16" and kind == "gauss")

    def __call__(self, D, I, rows, qn, k, what):
        if self.bars:
            assert_bars(D, I, self.corpus, rows, qn, k, f16=True)
            return
        Dr, Ir = self.flat.topk(rows, qn, k)
        assert np.array_equal(I, Ir), f"{what}: rows differ"
        assert np.array_equal(D, Dr), f"{what}: scores differ"


def search_both_ways(search, q):
    """One call of all the queries, then query by query: the same bits."""
    D, I = search(q)
    for i in range(q.shape[0]):
        D1, I1 = search(q[i:i + 1])
        assert np.array_equal(I1[0], I[i]) and np.array_equal(D1[0], D[i]), f"query {i} alone differs from the call"
    return D, I


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, d, kind", FLAT_CASES)
def test_flat_and_subset_search(dtype, d, kind):
    L, V = geom_of(dtype, d)
    corpus, groups = make_data(dtype, d, kind)
    check = Checker(corpus, dtype, kind)
    ix = FlatIPIndex.from_array(corpus, dtype=dtype)
    sel = selections()
    subs = {name: ix.subset(rows) for name, rows in sel.items()}
    everything = sel["ones"]
    rl = dtype == "sq8"
    try:
        assert [s.rows for s in subs.values()] == [r.size for r in sel.values()]
        for q, normalize in groups:
            qn = seen_queries(q, normalize)
            plain = {}
            for k in PLAIN_K:
                for opt in PLAIN_OPTS:
                    blocks = opt or default_blocks(N, L, V)
                    assert opt == 0 or is_small(N, blocks, L, V) == (opt == 256)  # (the rule quoted in the docstring)
                    ix.debug_option(7, opt)
                    D, I = search_both_ways(lambda x: ix.search(x, k, normalize=normalize), q)
                    if opt == 0:
                        check(D, I, everything, qn, k, f"plain k={k}")
                        plain[k] = (D, I)
                    else:  # the other variant: the same bits
                        assert np.array_equal(I, plain[k][1]) and np.array_equal(D, plain[k][0]), (k, opt)
            for k in SUBSET_K:
                first = {}
                for name, opt in SUBSET_RUNS:
                    m = sel[name].size
                    small = is_small(m, opt or default_blocks(m, L, V), L, V, sq8_rowlist=rl)
                    assert {("mask10", 1): not small, ("mask10", 256): small, ("forty", 0): small,
                            ("ones", 4): not small}.get((name, opt), True)
                    ix.debug_option(7, opt)
                    D, I = ix.search(q, k, normalize=normalize, params=SearchParameters(sel=subs[name]))
                    if name not in first:
                        check(D, I, sel[name], qn, k, f"subset {name} k={k}")
                        assert (I[:, m:] == -1).all() and (D[:, m:] == NEG).all() and (I[:, :min(k, m)] >= 0).all()
                        first[name] = (D, I)
                    else:
                        assert np.array_equal(I, first[name][1]) and np.array_equal(D, first[name][0]), (name, k, opt)
                if k in plain:  # the all-ones mask is the plain search
                    assert np.array_equal(first["ones"][1], plain[k][1]) and np.array_equal(first["ones"][0], plain[k][0])
            ix.debug_option(7, 0)
            D, I = ix.search(q, 50, normalize=normalize)
            Ds, Is = ix.search(q, 50, normalize=normalize, params=SearchParameters(sel=subs["ones"]))
            assert np.array_equal(Is, I) and np.array_equal(Ds, D)
    finally:
        ix.debug_option(7, 0)
        for s in subs.values():
            s.close()
        ix.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------
NLIST = 37


@pytest.mark.parametrize("dtype, d, kind", IVF_CASES)
def test_ivf_search(dtype, d, kind):
    corpus, groups = make_data(dtype, d, kind)
    assign = uneven_assignment()
    sizes = np.bincount(assign, minlength=NLIST)
    assert sizes[0] == 0 and sizes[20] == 0 and sizes[36] == 1 and sizes[7] == N // 3 and sizes.sum() == N
    cent = H.gauss(90 + d, NLIST, d)
    check = Checker(corpus, dtype, kind)
    ivf = IVFFlatIndex(d, NLIST, dtype=dtype)
    ivf.set_centroids(cent)
    ivf.add(corpus, assign=assign)
    try:
        assert np.array_equal(ivf.list_sizes(), sizes)
        for q, normalize in groups:
            nq = q.shape[0]
            qn = seen_queries(q, normalize)
            for nprobe in (1, 5, NLIST):
                for k in (10, 1500):
                    D, I = ivf.search(q, k, normalize=normalize, params=SearchParametersIVF(nprobe=nprobe))
                    second = ivf.last_kernel_ms()[2]
                    Dr, Ir, rows_of = ivf_reference(corpus, cent, assign, q, k, nprobe, normalize, dtype, flat=check.flat)
                    for i in range(nq):
                        if check.bars:
                            check(D[i:i + 1], I[i:i + 1], rows_of[i], qn[i:i + 1], k, "")
                        else:
                            assert np.array_equal(I[i], Ir[i]), (nprobe, k, i)
                            assert np.array_equal(D[i], Dr[i]), (nprobe, k, i)
                        D1, I1 = ivf.search(q[i:i + 1], k, normalize=normalize, params=SearchParametersIVF(nprobe=nprobe))
                        assert np.array_equal(I1[0], I[i]) and np.array_equal(D1[0], D[i]), (nprobe, k, i)
                    if nprobe == NLIST:
                        assert all(r.size == N for r in rows_of)
                        if k == 1500:
                            # all 3001 rows probed: at most 47 workgroups emit at most 15 keys each, which cannot
                            # prove 1500 ranks - every query is served by the second launch
                            assert second == nq, (second, nq)
                            assert ivf.last_kernel_ms()[2] == 1  # (the single-query call just made)
                        else:  # (nothing guarantees the first launch proves k = 10)
                            print(f"[{dtype} d={d} {kind}] nprobe {nprobe} k {k}: {second} of {nq} queries took the "
                                  "second launch")
    finally:
        ivf.close()


@pytest.mark.parametrize("dtype, d", [("sq8", 1025), ("f16", 1025), ("sq8", 4096)])
def test_ivf_refuses_rows_longer_than_an_f32_centroid(dtype, d):
    """The centroids are an f32 index (at most 1024 dimensions): the probed-list kernels of the geometries that begin
    past d = 1024 - sq8 (32,3) (32,4) (64,3) (64,4), f16 (64,3) (64,4) - cannot be reached. Pinned as a refusal."""
    ivf = IVFFlatIndex(d, 4, dtype=dtype)
    ivf.set_centroids(np.zeros((4, d), np.float32))
    ivf.add(H.gauss(1, 8, d))
    with pytest.raises(ValueError, match=f"unsupported d={d}"):  # (LS_ERR_INVALID_ARG)
        ivf.search(H.gauss(2, 1, d), 3)
    ivf.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------
P_N, P_D, P_NLIST = 6000, 32, 2500
RUNS = [(0, 300), (400, 1), (509, 2), (961, 63), (1200, 64), (1983, 65), (2435, 65)]  # (first rank, length) of empty lists
NPROBES = (3, 255, 256, 257, 511, 512, 513, 1023, 1025, 2047, 2048)


class ProbeData:
    """2500 lists over 6000 rows, most lists 0..3 rows, and two queries whose centroid ranking is known: query 0 lies
    along dimension 0, where the centroid of the list at rank r holds (2500 - r) / 2500, query 1 along dimension 1,
    which ranks the lists the other way round. By rank of query 0 the empty lists come in runs of 300 (ranks 0..299: the
    start; nprobe up to 257 probes nothing but empty lists), 1, 2 (ends at rank 510: the end of nprobe = 511), 63 (ends
    at 1023), 64, 65 (ends at 2047: the end of nprobe = 2048) and 65 (ranks 2435..2499: the start of query 1). Queries
    2, 3 are Gaussian."""

    def __init__(self):
        rng = np.random.default_rng(77)
        by_rank = rng.choice(4, size=P_NLIST, p=[0.25, 0.3, 0.25, 0.2])
        for a, ln in RUNS:
            by_rank[a:a + ln] = 0
            for edge in (a - 1, a + ln):
                if 0 <= edge < P_NLIST:
                    by_rank[edge] = max(by_rank[edge], 1)
        big = [350, 700, 1100, 1500, 1800, 2100, 2300, 2400]
        rem = P_N - int(by_rank.sum())
        assert rem > len(big)
        for j, r in enumerate(big):
            by_rank[r] += rem // len(big) + (j < rem % len(big))
        assert by_rank.sum() == P_N and (by_rank <= 3).mean() > 0.99
        self.by_rank = by_rank
        self.perm = rng.permutation(P_NLIST)  # list at rank r of query 0
        sizes = np.zeros(P_NLIST, np.int64)
        sizes[self.perm] = by_rank
        self.sizes = sizes
        self.assign = rng.permutation(np.repeat(np.arange(P_NLIST), sizes)).astype(np.int32)
        cent = np.float32(0.01) * H.gauss(78, P_NLIST, P_D, normalize=False)
        r = np.arange(P_NLIST, dtype=np.float32)
        cent[self.perm, 0] = (P_NLIST - r) / np.float32(P_NLIST)
        cent[self.perm, 1] = (r + 1) / np.float32(P_NLIST)
        self.cent = cent
        self.corpus = H.gauss(79, P_N, P_D)
        q = H.gauss(80, NQ, P_D)
        q[0], q[1] = 0.0, 0.0
        q[0, 0], q[1, 1] = 1.0, 1.0
        self.q = q


_probe_data = None


def probe_data():
    global _probe_data
    if _probe_data is None:
        _probe_data = ProbeData()
    return _probe_data


def run_probe_sweep(ivf, p, dtype, nprobes, ks, cent=None, assign=None):
    cent = p.cent if cent is None else cent
    assign = p.assign if assign is None else assign
    flat = Flat(p.corpus, dtype)
    for nprobe in nprobes:
        for k in ks:
            D, I = ivf.search(p.q, k, params=SearchParametersIVF(nprobe=nprobe))
            Dr, Ir, rows_of = ivf_reference(p.corpus, cent, assign, p.q, k, nprobe, False, dtype, flat=flat)
            assert np.array_equal(I, Ir), (nprobe, k)
            assert np.array_equal(D, Dr), (nprobe, k)
            yield nprobe, k, D, I, rows_of


def test_probe_list_prefix_and_search():
    p = probe_data()
    # the construction: query 0 ranks the lists as perm, query 1 the other way round, and the runs are where they should be
    _, P = oracle.c_search(p.cent, p.q[:2], 2048, order="scan")
    assert np.array_equal(P[0], p.perm[:2048]) and np.array_equal(P[1], p.perm[::-1][:2048])
    zero = p.by_rank == 0
    for a, ln in RUNS:
        assert zero[a:a + ln].all() and (a == 0 or not zero[a - 1]) and (a + ln == P_NLIST or not zero[a + ln])
    ivf = IVFFlatIndex(P_D, P_NLIST)
    ivf.set_centroids(p.cent)
    ivf.add(p.corpus, assign=p.assign)
    try:
        assert np.array_equal(ivf.list_sizes(), p.sizes)
        for nprobe, k, D, I, rows_of in run_probe_sweep(ivf, p, "f32", NPROBES, (5, 2048)):
            if nprobe <= 257:  # query 0 probes empty lists only; query 1 starts with 65 of them
                assert rows_of[0].size == 0 and (I[0] == -1).all() and (D[0] == NEG).all()
                assert (rows_of[1].size > 0) == (nprobe > 65)
            assert all((I[i] >= 0).sum() == min(k, rows_of[i].size) for i in range(NQ))
        # a query alone equals the query in company, where every thread owns several probe entries
        D, I = ivf.search(p.q, 2048, params=SearchParametersIVF(nprobe=2048))
        for i in range(NQ):
            D1, I1 = ivf.search(p.q[i:i + 1], 2048, params=SearchParametersIVF(nprobe=2048))
            assert np.array_equal(I1[0], I[i]) and np.array_equal(D1[0], D[i])
        # min(nprobe, nlist) beyond LS_MAX_K = 2048 probed lists: refused (include/leansearch_ivf.h), not clamped
        for nprobe in (2049, P_NLIST, 100_000):
            with pytest.raises(ValueError, match="exceeds LS_MAX_K = 2048"):  # (LS_ERR_INVALID_ARG)
                ivf.search(p.q, 5, params=SearchParametersIVF(nprobe=nprobe))
            D, I = np.empty((NQ, 5), np.float32), np.empty((NQ, 5), np.int64)
            assert native.load().ls_ivf_search(ivf._handle, p.q.ctypes.data, NQ, 5, nprobe, 0, D.ctypes.data,
                                               I.ctypes.data) == native.LS_ERR_INVALID_ARG
    finally:
        ivf.close()


def test_probe_list_prefix_and_search_sq8():
    p = probe_data()
    ivf = IVFFlatIndex(P_D, P_NLIST, dtype="sq8")
    ivf.set_centroids(p.cent)
    ivf.add(p.corpus, assign=p.assign)
    try:
        for nprobe, k, D, I, rows_of in run_probe_sweep(ivf, p, "sq8", (3, 257, 513, 2048), (5, 2048)):
            assert all((I[i] >= 0).sum() == min(k, rows_of[i].size) for i in range(NQ))
    finally:
        ivf.close()


@pytest.mark.parametrize("dtype", ["f32", "sq8"])
def test_nan_centroids_leave_unfilled_probe_entries(dtype):
    """nlist = LS_MAX_K = 2048 lists, three of them with a NaN centroid, nprobe = nlist: the coarse search returns
    2045 lists and three -1 entries, which the prefix must count as empty; the rows of those lists are never found."""
    p = probe_data()
    nlist = 2048
    cent = p.cent[:nlist].copy()
    nan_lists = [0, 1000, 2047]
    cent[nan_lists[0]] = np.nan
    cent[nan_lists[1], 5] = np.nan
    cent[nan_lists[2], 31] = np.nan
    assign = np.random.default_rng(81).integers(0, nlist, P_N).astype(np.int32)
    lost = np.flatnonzero(np.isin(assign, nan_lists))
    assert lost.size > 0
    ivf = IVFFlatIndex(P_D, nlist, dtype=dtype)
    ivf.set_centroids(cent)
    ivf.add(p.corpus, assign=assign)
    try:
        for nprobe, k, D, I, rows_of in run_probe_sweep(ivf, p, dtype, (2047, 2048, 100_000), (5, 2048), cent, assign):
            assert not np.isin(I, lost).any()
            if nprobe >= nlist:
                assert all(r.size == P_N - lost.size for r in rows_of)
    finally:
        ivf.close()
