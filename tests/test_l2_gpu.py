"""The L2 metric on the MI355X (include/leansearch_l2.h): every row geometry of the L2 scan kernels in
both variants, plain and row-list; special values; range search; add / remove; concurrent callers and routing; the
inner-product handles beside it; faiss_compat.IndexFlatL2.

Every comparison is np.array_equal on D and I against tests/l2_ref.c (tests/test_l2_cpu.py holds it to integer
arithmetic and to float64) under the library's total order, or - integer-valued corpora - against plain integer
arithmetic. The shapes and the launch plan are those of tests/test_geometry_cpu.py: at n = 3001 debug option 7 = 4 is
the non-SMALL variant and 256 the SMALL one for every geometry. Nothing is timed."""

import threading

import numpy as np
import pytest

from lean_explore_amd import faiss_compat, native
from lean_explore_amd.id_selectors import SearchParameters
from lean_explore_amd.index import FlatIPIndex, FlatL2Index
from oracle import oracle
from tests import helpers as H
from tests.test_geometry_cpu import (DIMS, N, NQ, PLAIN_OPTS, SUBSET_RUNS, default_blocks, geom_of, is_small,
                                     seen_queries, selections)
from tests.test_l2_cpu import FMAX, int_dists, query_seen, range_l2, ref_dists, stored_values, topk_l2

pytestmark = pytest.mark.gpu

KS = (1, 10, 2048)
CASES = [(dtype, d, kind) for dtype in ("f32", "f16") for d in DIMS[dtype] for kind in ("gauss", "int")]


def make_data(dtype, d, kind, n=N):
    """(corpus, [(queries, normalize)]): integer-valued data runs without normalisation (it would leave the exact
    regime); Gaussian rows are unit norm, queries 0, 1 are rescaled and run with normalize=True."""
    seed = 9000 + 3 * d + {"f32": 1, "f16": 2}[dtype]
    if kind == "int":
        return H.int_corpus(seed, n, d), [(H.int_corpus(seed + 1, NQ, d), False)]
    q = H.gauss(seed + 1, NQ, d)
    q[:2] *= np.float32(2.5)
    return H.gauss(seed, n, d), [(np.ascontiguousarray(q[:2]), True), (np.ascontiguousarray(q[2:]), False)]


def dists_of(corpus, dtype, kind, q, normalize):
    """[nq, n] reference distances of every row: integer arithmetic, or tests/l2_ref.c."""
    if kind == "int":
        return int_dists(corpus, q)
    return ref_dists(corpus, dtype, query_seen(q, normalize, dtype))


def same(got, want, what):
    assert np.array_equal(got[1], want[1]), f"{what}: rows differ"
    assert np.array_equal(got[0], want[0]), f"{what}: distances differ"


def search_both_ways(search, q):
    """One call of all the queries, then query by query: the same bits."""
    D, I = search(q)
    for i in range(q.shape[0]):
        D1, I1 = search(q[i:i + 1])
        assert np.array_equal(I1[0], I[i]) and np.array_equal(D1[0], D[i]), f"query {i} alone differs from the call"
    return D, I


# ---- 1: every geometry, both variants, plain and row-list ---------------------------------------------------------------
@pytest.mark.parametrize("dtype, d, kind", CASES)
def test_flat_and_subset_search(dtype, d, kind):
    L, V = geom_of(dtype, d)
    corpus, groups = make_data(dtype, d, kind)
    ix = FlatL2Index.from_array(corpus, dtype=dtype)
    sel = selections()
    subs = {name: ix.subset(rows) for name, rows in sel.items()}
    try:
        assert ix.metric == "l2" and native.load().ls_metric(ix._handle) == native.LS_METRIC_L2
        for q, normalize in groups:
            dist = dists_of(corpus, dtype, kind, q, normalize)
            plain = {}
            for k in KS:
                for opt in PLAIN_OPTS:
                    blocks = opt or default_blocks(N, L, V)
                    assert opt == 0 or is_small(N, blocks, L, V) == (opt == 256)  # (the restated SMALL rule)
                    ix.debug_option(7, opt)
                    got = search_both_ways(lambda x: ix.search(x, k, normalize=normalize), q)
                    if opt == 0:
                        same(got, topk_l2(dist, k), f"plain k={k}")
                        plain[k] = got
                    else:  # the other variant: the same bits
                        same(got, plain[k], f"plain k={k} option 7={opt}")
                first = {}
                for name, opt in SUBSET_RUNS:
                    m = sel[name].size
                    small = is_small(m, opt or default_blocks(m, L, V), L, V)
                    assert {("mask10", 1): not small, ("mask10", 256): small, ("forty", 0): small,
                            ("ones", 4): not small}.get((name, opt), True)
                    ix.debug_option(7, opt)
                    got = ix.search(q, k, normalize=normalize, params=SearchParameters(sel=subs[name]))
                    if name not in first:
                        same(got, topk_l2(dist, k, sel[name]), f"subset {name} k={k}")
                        D, I = got
                        assert (I[:, m:] == -1).all() and (D[:, m:] == FMAX).all() and (I[:, :min(k, m)] >= 0).all()
                        first[name] = got
                    else:
                        same(got, first[name], f"subset {name} k={k} option 7={opt}")
                same(first["ones"], plain[k], f"all-ones subset k={k}")  # the all-ones mask is the plain search
            ix.debug_option(7, 0)
    finally:
        ix.debug_option(7, 0)
        for s in subs.values():
            s.close()
        ix.close()


# ---- 2: special values --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_special_values(dtype):
    d, n = 100, 500
    corpus = H.gauss(41, n, d)
    corpus[[17, 200]] = corpus[5]  # duplicates of row 5
    bad = {30: np.nan, 31: np.inf, 32: -np.inf}
    for r, v in bad.items():
        corpus[r, 7] = v
    if dtype == "f32":
        bad[33] = 3e38
        corpus[33, 3] = np.float32(3e38)  # (3e38 - q)^2 overflows: the distance is +inf
    q = np.ascontiguousarray(corpus[[5, 100]])
    ix = FlatL2Index.from_array(corpus, dtype=dtype)
    try:
        dist = ref_dists(corpus, dtype, query_seen(q, False, dtype))
        with np.errstate(invalid="ignore"):
            assert not (dist[:, list(bad)] < FMAX).any()
        for k in (3, n):
            D, I = search_both_ways(lambda x: ix.search(x, k), q)
            same((D, I), topk_l2(dist, k), f"k={k}")
            assert not np.isin(I, list(bad)).any()
            # an exact match: +0.0, rank 0, duplicates in row order
            assert I[0, :3].tolist() == [5, 17, 200] and (D[0, :3] == 0).all() and not np.signbit(D[0, :3]).any()
            assert I[1, 0] == 100 and D[1, 0] == 0 and not np.signbit(D[1, 0])
            assert (I[:, n - len(bad):] == -1).all() and (D[:, n - len(bad):] == FMAX).all()
    finally:
        ix.close()
    # k > n with n = 37, and a base
    small = np.ascontiguousarray(H.gauss(42, 37, d))
    ix = FlatL2Index.from_array(small, dtype=dtype, base=1000)
    try:
        D, I = ix.search(q, 50)
        same((D, I), topk_l2(ref_dists(small, dtype, query_seen(q, False, dtype)), 50, base=1000), "n = 37")
        assert (I[:, :37] >= 1000).all() and (I[:, 37:] == -1).all() and (D[:, 37:] == FMAX).all()
        lims, Dr, Ir = ix.range_search(q, np.inf)
        assert lims.tolist() == [0, 37, 74] and np.array_equal(Ir, np.tile(np.arange(1000, 1037), 2))
    finally:
        ix.close()
    # n = 0
    ix = FlatL2Index(d, dtype=dtype)
    D, I = ix.search(q, 4)
    assert (I == -1).all() and (D == FMAX).all() and ix.ntotal == 0
    assert ix.range_search(q, np.inf)[0].tolist() == [0, 0, 0]
    ix.close()


# ---- 3: range search ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, d", [(t, d) for t in ("f32", "f16") for d in (100, 384)])
def test_range_search(dtype, d):
    corpus = H.gauss(50 + d, N, d)
    q = H.gauss(51 + d, NQ, d)
    q[:2] *= np.float32(2.5)
    ix = FlatL2Index.from_array(corpus, dtype=dtype)
    rows = selections()["mask10"]
    sub = ix.subset(rows)
    try:
        for normalize in (True, False):
            dist = ref_dists(corpus, dtype, query_seen(q, normalize, dtype))
            radii = [float(np.median(dist[0])), float(dist[0].min()), np.inf, 0.0, -1.0, np.nan, -np.inf]
            for radius in radii:
                for r, params in ((None, None), (rows, SearchParameters(sel=sub))):
                    lims, D, I = ix.range_search(q, radius, normalize=normalize, params=params)
                    wl, wD, wI = range_l2(dist, radius, r)
                    assert np.array_equal(lims, wl), (radius, r is None)
                    assert np.array_equal(I, wI) and np.array_equal(D, wD), (radius, r is None)
                    for i in range(NQ):  # rows ascending inside a segment
                        assert (np.diff(I[int(lims[i]):int(lims[i + 1])]) > 0).all()
            lims, D, I = ix.range_search(q, np.inf, normalize=normalize)
            assert lims.tolist() == [0, N, 2 * N, 3 * N, 4 * N]
            assert ix.range_search(q, float(dist[0].min()), normalize=normalize)[0][1] == 0  # strict
            # the consequence of leansearch_range.h: the range result is the top-k result filtered, re-sorted by row
            # (one radius serves every query of the call: the smallest of the queries' 1500th distances, so that no
            # query has more hits than the top-k has slots)
            radius = float(np.sort(dist, axis=1)[:, 1500].min())
            lims, D, I = ix.range_search(q, radius, normalize=normalize)
            assert 1 <= int(np.diff(lims.astype(np.int64)).max()) <= 1500
            Dk, Ik = ix.search(q, 2048, normalize=normalize)
            for i in range(NQ):
                a, b = int(lims[i]), int(lims[i + 1])
                assert b - a <= 2048
                keep = (Dk[i] < np.float32(radius)) & (Ik[i] >= 0)
                order = np.argsort(Ik[i][keep], kind="stable")
                assert np.array_equal(I[a:b], Ik[i][keep][order]) and np.array_equal(D[a:b], Dk[i][keep][order])
    finally:
        sub.close()
        ix.close()


# ---- 4: mutation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, d", [("f32", 384), ("f16", 385)])
def test_add_and_remove(dtype, d):
    rng = np.random.default_rng(60 + d)
    first, more, last = H.gauss(61 + d, N, d), H.gauss(62 + d, 200, d), H.gauss(63 + d, 200, d)
    q = H.gauss(64 + d, NQ, d)
    ix = FlatL2Index.from_array(first, dtype=dtype)
    try:
        ix.search(q, 5)
        ix.add(more)
        everything = np.concatenate([first, more])
        picked = np.flatnonzero(rng.random(everything.shape[0]) < 0.3)
        sub = ix.subset(picked)
        gone = rng.random(everything.shape[0]) < 0.10
        assert ix.remove_ids(gone) == int(gone.sum()) and ix.metric == "l2"
        assert native.load().ls_metric(ix._handle) == native.LS_METRIC_L2
        ix.add(last)
        survivors = np.concatenate([everything[~gone], last])
        assert ix.ntotal == survivors.shape[0]
        new_of = np.cumsum(~gone) - 1
        picked_new = new_of[picked[~gone[picked]]]
        assert sub.rows == picked_new.size < picked.size
        fresh = FlatL2Index.from_array(survivors, dtype=dtype)
        try:
            for normalize in (False, True):
                dist = ref_dists(survivors, dtype, query_seen(q, normalize, dtype))
                for k in (10, 2048):
                    got = ix.search(q, k, normalize=normalize)
                    same(got, fresh.search(q, k, normalize=normalize), f"against a fresh index k={k}")
                    same(got, topk_l2(dist, k), f"against the reference k={k}")
                    same(ix.search(q, k, normalize=normalize, params=SearchParameters(sel=sub)),
                         topk_l2(dist, k, picked_new), f"the shrunken subset k={k}")
            radius = float(np.median(dist[0]))
            a, b = ix.range_search(q, radius, normalize=True), fresh.range_search(q, radius, normalize=True)
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
            assert np.array_equal(ix.host_corpus(), stored_values(survivors, dtype))
        finally:
            fresh.close()
            sub.close()
    finally:
        ix.close()


# ---- 5: concurrency and routing -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_concurrent_callers_and_routing(dtype):
    n, d, k = 5000, 384, 10  # (an inner-product index of this size serves small batches by its passes)
    corpus = H.gauss(70, n, d)
    q = H.gauss(71, 160, d)
    ix = FlatL2Index.from_array(corpus, dtype=dtype)
    try:
        serial = [ix.search(q[i:i + 1], k) for i in range(160)]
        dist = ref_dists(corpus, dtype, query_seen(q[:16], False, dtype))
        same(ix.search(q[:16], k), topk_l2(dist, k), "a 16-query call")
        D16, I16 = ix.search(q[:16], k)
        for i in range(16):  # a 16-query call equals 16 single calls
            assert np.array_equal(D16[i], serial[i][0][0]) and np.array_equal(I16[i], serial[i][1][0])
        D40, I40 = ix.search(q[:40], k)  # (more than one combined call carries)
        for i in range(40):
            assert np.array_equal(D40[i], serial[i][0][0]) and np.array_equal(I40[i], serial[i][1][0])
        out, errors = [None] * 160, []

        def worker(t):
            try:
                for j in range(20):
                    i = t * 20 + j
                    out[i] = ix.search(q[i:i + 1], k)
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for i in range(160):
            assert np.array_equal(out[i][0], serial[i][0]) and np.array_equal(out[i][1], serial[i][1]), i
        # never a small-batch pass: the ls_mq / ls_mq16 counters
        assert ix.debug_counter(23) == 0 and ix.debug_counter(34) == 0
        for setter in (ix.set_f16_small_batch, ix.set_sq8_small_batch, ix.set_subset_small_batch):
            with pytest.raises(ValueError):
                setter(True)
        lib = native.load()
        for fn in (lib.ls_set_f16_small_batch, lib.ls_set_sq8_small_batch, lib.ls_set_subset_small_batch):
            assert fn(ix._handle, 1) == native.LS_ERR_INVALID_ARG and b"L2" in lib.ls_last_error()
        with pytest.raises(ValueError, match="L2"):
            ix.search_device(q[:2], k)
        # (the refusal comes before anything is read or written: any non-null pointers do)
        os_, oi, fl = np.empty((2, k), np.float32), np.empty((2, k), np.int64), np.zeros(2, np.uint32)
        for flags in (0, native.LS_FLAG_ASYNC, native.LS_FLAG_PIPELINE, native.LS_FLAG_NORMALIZE):
            assert lib.ls_search_device(ix._handle, q.ctypes.data, 2, k, flags, os_.ctypes.data, oi.ctypes.data,
                                        None) == native.LS_ERR_INVALID_ARG
            assert b"L2" in lib.ls_last_error()
        assert lib.ls_export_flags(ix._handle, fl.ctypes.data, 2, None) == native.LS_ERR_INVALID_ARG
        assert b"L2" in lib.ls_last_error()
        same(ix.search(q[:16], k), (D16, I16), "after the refusals")
    finally:
        ix.close()


# ---- 6: inner-product handles beside it -----------------------------------------------------------------------------------
def test_inner_product_handles_are_unchanged():
    d = 384
    corpus, q = H.gauss(80, N, d), H.gauss(81, NQ, d)
    ip = FlatIPIndex.from_array(corpus)
    l2 = FlatL2Index.from_array(corpus)
    try:
        assert ip.metric == "ip" and native.load().ls_metric(ip._handle) == native.LS_METRIC_INNER_PRODUCT
        l2.search(q, 10)
        for k in (10, 2048):
            D, I = ip.search(q, k)
            Dr, Ir = oracle.c_search(corpus, seen_queries(q, False), k, order="scan")
            assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
            for i in range(NQ):
                D1, I1 = ip.search(q[i:i + 1], k, normalize=True)
                Dr, Ir = oracle.c_search(corpus, seen_queries(q[i:i + 1], True), k, order="scan")
                assert np.array_equal(I1, Ir) and np.array_equal(D1, Dr)
        lims, Dr_, Ir_ = ip.range_search(q, 0.1)
        S = np.stack([oracle.c_scores(corpus, qv, order="scan") for qv in q])
        assert np.array_equal(Ir_, np.concatenate([np.flatnonzero(s > np.float32(0.1)) for s in S]))
    finally:
        ip.close()
        l2.close()
    ci, qi = H.int_corpus(82, N, d), H.int_corpus(83, NQ, d)
    ip = FlatIPIndex.from_array(ci, dtype="f16")
    try:
        for k in (10, 2048):
            D, I = ip.search(qi, k)
            Dr, Ir = oracle.c_search(ci, qi, k, f16=True)
            assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
            want = (qi.astype(np.int64) @ ci.astype(np.int64).T).astype(np.float32)
            assert np.array_equal(D, np.take_along_axis(want, I, axis=1))
    finally:
        ip.close()


# ---- 7: faiss_compat ------------------------------------------------------------------------------------------------------
def test_faiss_compat_index_flat_l2(tmp_path):
    d = 100
    corpus, q = H.gauss(90, 800, d, normalize=False), H.gauss(91, NQ, d, normalize=False)
    ix = faiss_compat.IndexFlatL2(d)
    ix.add(corpus[:500])
    D, I = ix.search(q, 10)
    same((D, I), topk_l2(ref_dists(corpus[:500], "f32", q), 10), "after the first add")
    ix.add(corpus[500:])
    dist = ref_dists(corpus, "f32", q)
    same(ix.search(q, 10), topk_l2(dist, 10), "after the second add")
    radius = float(np.median(dist[0]))
    got = ix.range_search(q, radius)
    assert all(np.array_equal(a, b) for a, b in zip(got, range_l2(dist, radius)))
    sel = faiss_compat.IDSelectorRange(100, 300)
    same(ix.search(q, 10, params=faiss_compat.SearchParameters(sel=sel)), topk_l2(dist, 10, np.arange(100, 300)),
         "IDSelectorRange")
    assert ix.remove_ids(faiss_compat.IDSelectorRange(0, 50)) == 50 and ix.ntotal == 750
    want = topk_l2(ref_dists(corpus[50:], "f32", q), 10)
    same(ix.search(q, 10), want, "after remove_ids")
    p = tmp_path / "l2.index"
    faiss_compat.write_index(ix, p)
    assert p.read_bytes()[:4] == b"IxF2"
    back = faiss_compat.read_index(p)
    assert isinstance(back, faiss_compat.IndexFlatL2) and back.ntotal == 750
    same(back.search(q, 10), want, "after write_index / read_index")
    ix.close()
    back.close()
