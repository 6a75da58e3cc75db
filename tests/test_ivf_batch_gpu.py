"""The IVF small-batch pass on the MI355X (include/leansearch_ivf_batch.h, IVFFlatIndex(small_batch=True)): groups of
2..16 queries of a call share one pass over the union of the lists they probe. Every comparison is ``array_equal`` on
scores and indices: option on == option off == each query's lone call, and ``last_passes()`` proves which path ran.
tests/test_ivf_batch_cpu.py holds the host plan to every shape used here (a declined plan would turn these into tests of
the per-query chains). Corpora and explicit lists: tests/ivf_batch_shapes.py."""

import ctypes

import numpy as np
import pytest

from lean_explore_amd import native
from lean_explore_amd.id_selectors import SearchParametersIVF
from lean_explore_amd.index import FlatIPIndex
from lean_explore_amd.ivf import IVFFlatIndex
from tests import ivf_batch_shapes as SH
from tests.test_ivf_gpu import subset_reference

pytestmark = pytest.mark.gpu

NEG = np.float32(-np.finfo(np.float32).max)


def build(corpus, cent, assign, small_batch=True, dtype="f32"):
    ivf = IVFFlatIndex(corpus.shape[1], cent.shape[0], dtype=dtype, small_batch=small_batch)
    ivf.set_centroids(cent)
    ivf.add(corpus, assign=assign)
    return ivf


def n_passes(nq):
    return len(SH.groups(nq))


def on_off(ivf, q, k, nprobe, normalize=False, passes=None):
    """The call with the option off, then on: equal bits; the on call launched `passes` passes (default: one per group
    of >= 2 queries) and the off call none. Returns the result and the pass count / union rows of the on call."""
    par = SearchParametersIVF(nprobe=nprobe)
    ivf.set_small_batch(False)
    D0, I0 = ivf.search(q, k, normalize=normalize, params=par)
    assert ivf.last_passes() == (0, 0)
    ivf.set_small_batch(True)
    D1, I1 = ivf.search(q, k, normalize=normalize, params=par)
    got, rows = ivf.last_passes()
    assert got == (n_passes(q.shape[0]) if passes is None else passes), (got, q.shape[0])
    assert np.array_equal(I1, I0), np.argwhere(I1 != I0)[:5]
    assert np.array_equal(D1.view(np.uint32), D0.view(np.uint32))
    return D1, I1, rows


def lone_calls(ivf, q, k, nprobe, normalize=False):
    par = SearchParametersIVF(nprobe=nprobe)
    D = np.empty((q.shape[0], k), np.float32)
    I = np.empty((q.shape[0], k), np.int64)
    for i in range(q.shape[0]):
        D[i], I[i] = (a[0] for a in ivf.search(q[i:i + 1], k, normalize=normalize, params=par))
        assert ivf.last_passes() == (0, 0), "a lone query launches no pass"
    return D, I


def probed_lists(cent, q, nprobe, normalize=False):
    """The probe lists by an independent exact search over the centroids."""
    coarse = FlatIPIndex.from_array(cent)
    try:
        return coarse.search(q, min(nprobe, cent.shape[0]), normalize=normalize)[1]
    finally:
        coarse.close()


def assert_rows_in_own_lists(I, assign, P):
    for i in range(I.shape[0]):
        rows = I[i][I[i] >= 0]
        assert np.isin(assign[rows], P[i][P[i] >= 0]).all(), i


# ---- 1. every geometry -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", SH.DIMS)
def test_every_geometry_on_equals_off_equals_lone(d):
    corpus, cent, assign, q = SH.geometry(d)
    normalize = d != 64
    ivf = build(corpus, cent, assign)
    try:
        Dl, Il = lone_calls(ivf, q, SH.GEO_K, SH.GEO_NPROBE, normalize)
        sizes, off, ids = SH.layout(assign, SH.GEO_NLIST)
        P = probed_lists(cent, q, SH.GEO_NPROBE, normalize)
        for nq in SH.GEO_NQS:  # 17: one pass + one chain; 33: two passes + one chain
            D, I, rows = on_off(ivf, q[:nq], SH.GEO_K, SH.GEO_NPROBE, normalize)
            assert np.array_equal(I, Il[:nq]) and np.array_equal(D, Dl[:nq]), nq
            want, i0 = 0, 0
            for g in SH.groups(nq):  # the accessor's union rows are the model's
                want += int(SH.union_model(P[i0:i0 + g], off, ids)[1][-1])
                i0 += g
            assert rows == want, (nq, rows, want)
        assert_rows_in_own_lists(Il, assign, P)
        if d == 384:  # the definition: the flat index's subset search over the probed lists' rows
            flat, coarse = FlatIPIndex.from_array(corpus), FlatIPIndex.from_array(cent)
            try:
                Dr, Ir, _ = subset_reference(flat, coarse, assign, q[:16], SH.GEO_K, SH.GEO_NPROBE, normalize)
            finally:
                flat.close()
                coarse.close()
            assert np.array_equal(Il[:16], Ir) and np.array_equal(Dl[:16], Dr)
    finally:
        ivf.close()


# ---- 2. ties across lists, row order against position order ----------------------------------------------------------------
def test_ties_come_out_row_ascending_although_positions_run_the_other_way():
    corpus, cent, assign, q = SH.ties()
    n, nlist, k = corpus.shape[0], cent.shape[0], 10
    assert assign[0] == nlist - 1 and assign[n - 1] == 0  # the highest rows sit in the lowest lists
    ivf = build(corpus, cent, assign)
    try:
        D, I, rows = on_off(ivf, q, k, nlist)
        assert rows == n  # every list is probed: the union is the index, list-major
        for i in range(q.shape[0]):
            s = (corpus[:, 0] * q[i, 0] + corpus[:, 1] * q[i, 1]).astype(np.float32)  # (small integers: exact)
            Ds, Is = SH.expected_order(s, np.arange(n), k)
            assert np.array_equal(I[i], Is) and np.array_equal(D[i], Ds), i
        assert (D[0] == D[0][4]).sum() == 6 and (corpus[:, 0] == 2.0).sum() > 4000  # the tie straddles rank k
    finally:
        ivf.close()


# ---- 3. masks, 6. a served-again query ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def axes_case():
    """The axes index with twelve planted rows: consecutive original rows of lists 2 (the best rows of query 0 of case a,
    which probes lists 0 and 1 only) - see the cases."""
    corpus, cent, assign = SH.axes()
    rng = np.random.default_rng(99)
    qa = np.stack([SH.axes_query(rng, [0, 1]), SH.axes_query(rng, [2, 3])])
    corpus, assign, r0 = SH.axes_plant(corpus, assign, qa[0], [2], 12, 3.0)
    ivf = build(corpus, cent, assign)
    yield ivf, corpus, cent, assign, qa, r0
    ivf.close()


def test_masks_disjoint_probe_sets_do_not_leak_rows(axes_case):
    ivf, corpus, cent, assign, qa, r0 = axes_case
    P = probed_lists(cent, qa, 2)
    assert np.array_equal(P, [[0, 1], [2, 3]])
    planted = np.arange(r0, r0 + 12)
    assert (assign[planted] == 2).all()
    best = np.argsort(-(corpus @ qa[0]))[:12]
    assert set(best) == set(planted), "the best rows for query 0 lie only in a list query 1 probes"
    D, I, rows = on_off(ivf, qa, 10, 2)
    assert not np.isin(I[0], planted).any()
    assert_rows_in_own_lists(I, assign, P)
    Dl, Il = lone_calls(ivf, qa, 10, 2)
    assert np.array_equal(I, Il) and np.array_equal(D, Dl)
    # (d) the tile at the boundary between query 0's lists and query 1's carries both masks
    sizes, off, ids = SH.layout(assign, SH.AX_NLIST)
    _, lpre, _, _, umask = SH.union_model(P, off, ids)
    assert rows == int(lpre[-1]) and (sizes % 16 != 0).all()
    t = int(lpre[2]) // 16
    assert set(umask[16 * t:16 * t + 16]) == {1, 2}


def test_masks_sixteen_queries_probe_one_list(axes_case):
    ivf, corpus, cent, assign, _, _ = axes_case
    rng = np.random.default_rng(3)
    q = np.stack([SH.axes_query(rng, [SH.AX_BIG]) for _ in range(16)])
    P = probed_lists(cent, q, 1)
    assert (P == SH.AX_BIG).all()
    D, I, rows = on_off(ivf, q, 10, 1)
    assert rows == SH.axes_sizes()[SH.AX_BIG] >= SH.MIN_ROWS
    assert_rows_in_own_lists(I, assign, P)
    Dl, Il = lone_calls(ivf, q, 10, 1)
    assert np.array_equal(I, Il) and np.array_equal(D, Dl)


@pytest.mark.parametrize("normalize", [False, True])
def test_masks_sixteen_queries_with_pairwise_disjoint_probes_and_padding(axes_case, normalize):
    """Query i probes list i alone; list 15 holds five rows, so query 15 returns five rows and (-FLT_MAX, -1) padding."""
    ivf, corpus, cent, assign, _, _ = axes_case
    rng = np.random.default_rng(4)
    q = np.stack([SH.axes_query(rng, [l]) for l in range(16)])
    P = probed_lists(cent, q, 1, normalize)
    assert np.array_equal(P[:, 0], np.arange(16))
    D, I, rows = on_off(ivf, q, 10, 1, normalize)
    assert rows == corpus.shape[0]
    assert_rows_in_own_lists(I, assign, P)
    assert (I[SH.AX_TINY, :5] >= 0).all() and (I[SH.AX_TINY, 5:] == -1).all() and (D[SH.AX_TINY, 5:] == NEG).all()
    assert (I[:SH.AX_TINY] >= 0).all()
    Dl, Il = lone_calls(ivf, q, 10, 1, normalize)
    assert np.array_equal(I, Il) and np.array_equal(D, Dl)


def test_a_flagged_query_is_served_again_and_still_equals_the_off_path(axes_case):
    """Twelve adjacent storage rows of list 2 are the best rows of the query that probes it: four of them meet in one
    lane's list of three keys (the plan pins keys == 3 for this shape: test_ivf_batch_cpu.py), the dropped key lies above
    the k-th best, the selection cannot prove its keys and raises the query's flag: the second launch serves it."""
    ivf, corpus, cent, assign, qa, r0 = axes_case
    q = np.stack([qa[0].copy(), qa[0].copy()])
    q[:, :SH.AX_NLIST] = 0.0
    q[0, 2], q[1, 3] = 5.0, 5.0  # query 0 probes list 2, where its best rows are; query 1 list 3
    assert np.array_equal(probed_lists(cent, q, 1)[:, 0], [2, 3])
    D, I, _ = on_off(ivf, q, 10, 1)
    assert ivf.last_kernel_ms()[2] >= 1, "no query of the group was served again"
    assert np.array_equal(np.sort(I[0]), np.arange(r0 + 2, r0 + 12))  # (the planted rows score higher the later they come)
    Dl, Il = lone_calls(ivf, q, 10, 1)
    assert np.array_equal(I, Il) and np.array_equal(D, Dl)


# ---- 4. edges --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [False, True])
def test_edges_empty_lists_all_lists_and_non_finite_rows(normalize):
    corpus, cent, assign, q = SH.geometry(128)
    corpus, assign = corpus.copy(), assign.copy()
    assign[np.isin(assign, (3, 7, 39))] = 0  # empty lists inside (and at the end of) the union
    bad = np.array([5, 1000, 2000, 3000, 9999])
    corpus[bad[0]] = np.nan
    corpus[bad[1], 0] = np.inf
    corpus[bad[2], 1] = -np.inf
    corpus[bad[3]] = -np.finfo(np.float32).max
    corpus[bad[4], 2] = np.nan
    ivf = build(corpus, cent, assign)
    flat = FlatIPIndex.from_array(corpus)
    try:
        assert (ivf.list_sizes()[[3, 7, 39]] == 0).all()
        q = q[:5]
        D, I, rows = on_off(ivf, q, SH.GEO_K, SH.GEO_NLIST + 5, normalize)  # nprobe >= nlist: the flat search
        assert rows == SH.GEO_N
        for i in range(q.shape[0]):
            Df, If = flat.search(q[i:i + 1], SH.GEO_K, normalize=normalize)
            assert np.array_equal(I[i], If[0]) and np.array_equal(D[i], Df[0]), i
        assert not np.isnan(D).any() and not np.isin(I, bad[[0, 4]]).any()
        D8, I8, _ = on_off(ivf, q, SH.GEO_K, SH.GEO_NPROBE, normalize)
        Dl, Il = lone_calls(ivf, q, SH.GEO_K, SH.GEO_NPROBE, normalize)
        assert np.array_equal(I8, Il) and np.array_equal(D8, Dl) and not np.isnan(D8).any()
    finally:
        ivf.close()
        flat.close()


# ---- 5. the pass declines --------------------------------------------------------------------------------------------
def test_the_pass_declines_below_the_row_threshold_and_for_a_large_k():
    corpus, cent, assign, q = SH.geometry(64)
    ivf = build(corpus, cent, assign)
    try:  # a k the key lists decline
        on_off(ivf, q[:16], SH.K_DECLINED, SH.GEO_NPROBE, passes=0)
    finally:
        ivf.close()
    ivf = build(corpus[:SH.SMALL_N], cent[:8], SH.host_assign(corpus[:SH.SMALL_N], cent[:8]))
    try:  # every group's bound is below 4096 rows
        on_off(ivf, q[:16], 10, 8, passes=0)
    finally:
        ivf.close()


# ---- 7. what must not move -------------------------------------------------------------------------------------------
def test_subsets_lone_queries_and_other_dtypes_are_untouched():
    corpus, cent, assign, q = SH.geometry(64)
    ivf = build(corpus, cent, assign, small_batch=False)
    try:
        ivf.nprobe = SH.GEO_NPROBE
        sub = ivf.subset(np.arange(corpus.shape[0]) % 3 != 0)
        D0, I0 = ivf.search(q[:16], SH.GEO_K, params=sub)
        ivf.set_small_batch(True)
        D1, I1 = ivf.search(q[:16], SH.GEO_K, params=sub)
        assert ivf.last_passes() == (0, 0), "ls_ivf_search_subset keeps its chains"
        assert np.array_equal(I1, I0) and np.array_equal(D1, D0)
        ivf.search(q[:16], SH.GEO_K)
        assert ivf.last_passes()[0] == 1
        ivf.search(q[:1], SH.GEO_K)
        assert ivf.last_passes() == (0, 0), "a lone query launches no pass"
        ivf.set_small_batch(False)
        ivf.search(q[:16], SH.GEO_K)
        assert ivf.last_passes() == (0, 0), "switching the option off restores the chains"
        sub.close()
    finally:
        ivf.close()
    h16 = build(corpus[:2000], cent, assign[:2000], small_batch=False, dtype="f16")
    try:
        h16.list_sizes()  # (builds the device object)
        lib = native.load()
        assert lib.ls_ivf_set_small_batch(h16._handle, 1) == native.LS_ERR_INVALID_ARG
        assert b"fp16" in lib.ls_last_error()
        assert lib.ls_ivf_set_small_batch(h16._handle, 0) == native.LS_OK
        with pytest.raises(ValueError, match="small_batch"):
            h16.set_small_batch(True)
        p = ctypes.c_int32(-1)
        assert lib.ls_ivf_last_passes(h16._handle, ctypes.byref(p), None) == native.LS_OK and p.value == 0
    finally:
        h16.close()
