"""The L2 metric on the IVF index on the MI355X (include/leansearch_ivf_l2.h).

Every comparison is np.array_equal on D and I against the host reference of tests/test_ivf_l2_cpu.py, which means
tests/l2_ref.c: the probed lists are the top min(nprobe, nlist) centroids under the f32 restatement (distance
ascending, list ascending), the result is the flat L2 order over the rows of those lists. The shapes are those of the
IVF geometry tests: N = 3001 rows, 37 lists with uneven_assignment() (two empty lists, one list of one row, one of a
third of the rows), one full and one ragged d per geometry an IVF index can reach. Nothing asserts a time."""

import ctypes

import numpy as np
import pytest

from lean_explore_amd import faiss_compat, native
from lean_explore_amd.id_selectors import SearchParametersIVF
from lean_explore_amd.index import FlatL2Index
from lean_explore_amd.ivf import IVFFlatIndex
from tests import helpers as H
from tests.test_geometry_cpu import N, NQ, ivf_dims, ivf_reference, selections, uneven_assignment
from tests.test_ivf_l2_cpu import (ivf_l2_range_reference, ivf_l2_reference, nearest_l2, probe_l2, probed_rows)
from tests.test_l2_cpu import FMAX, exact_topk_l2, int_dists, query_seen, ref_dists

pytestmark = pytest.mark.gpu

NLIST = 37
SEARCH_CASES = [(dtype, d, kind) for dtype in ("f32", "f16") for d in ivf_dims(dtype) for kind in ("gauss", "int")]


def make_data(dtype, d, kind, n=N):
    """(corpus, centroids, [(queries, normalize)]): integer-valued data (every distance an exact integer, ties abound)
    runs without normalisation only; Gaussian rows are NOT unit norm, queries 0, 1 are rescaled and run with
    normalize=True."""
    seed = 9000 + 3 * d + {"f32": 1, "f16": 2}[dtype]
    if kind == "int":
        return H.int_corpus(seed, n, d), H.int_corpus(seed + 2, NLIST, d), [(H.int_corpus(seed + 1, NQ, d), False)]
    q = H.gauss(seed + 1, NQ, d, normalize=False)
    q[:2] *= np.float32(2.5)
    return (H.gauss(seed, n, d, normalize=False), H.gauss(seed + 2, NLIST, d, normalize=False),
            [(np.ascontiguousarray(q[:2]), True), (np.ascontiguousarray(q[2:]), False)])


def l2_index(d, cent, corpus, assign=None, dtype="f32", **kw):
    ix = IVFFlatIndex(d, cent.shape[0], dtype=dtype, metric="l2", **kw)
    ix.set_centroids(cent)
    ix.add(corpus, assign=assign)
    return ix


def metric_of(ix):
    return native.load().ls_ivf_metric(ix._ensure_built())


# ---- 1: search at every geometry ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, d, kind", SEARCH_CASES)
def test_search_at_every_geometry(dtype, d, kind):
    corpus, cent, groups = make_data(dtype, d, kind)
    assign = uneven_assignment()
    sizes = np.bincount(assign, minlength=NLIST)
    assert sizes[0] == 0 and sizes[20] == 0 and sizes[36] == 1 and sizes[7] == N // 3 and sizes.sum() == N
    ivf = l2_index(d, cent, corpus, assign, dtype)
    flat = FlatL2Index.from_array(corpus, dtype=dtype)
    try:
        assert np.array_equal(ivf.list_sizes(), sizes) and metric_of(ivf) == native.LS_METRIC_L2
        for q, normalize in groups:
            nq = q.shape[0]
            dv = ref_dists(corpus, dtype, query_seen(q, normalize, dtype))
            if kind == "int":  # the restatement itself is plain integer arithmetic here
                assert np.array_equal(dv, int_dists(corpus, q))
            for nprobe in (1, 5, NLIST):
                for k in (10, 1500):
                    D, I = ivf.search(q, k, normalize=normalize, params=SearchParametersIVF(nprobe=nprobe))
                    second = ivf.last_kernel_ms()[2]
                    Dr, Ir, rows_of = ivf_l2_reference(corpus, cent, assign, q, k, nprobe, normalize, dtype, dists=dv)
                    assert np.array_equal(I, Ir), (nprobe, k)
                    assert np.array_equal(D, Dr), (nprobe, k)
                    for i in range(nq):
                        D1, I1 = ivf.search(q[i:i + 1], k, normalize=normalize, params=SearchParametersIVF(nprobe=nprobe))
                        assert np.array_equal(I1[0], I[i]) and np.array_equal(D1[0], D[i]), (nprobe, k, i)
                    if nprobe == NLIST:
                        assert all(r.size == N for r in rows_of)
                        Df, If = flat.search(q, k, normalize=normalize)
                        assert np.array_equal(I, If) and np.array_equal(D, Df), k
                        if k == 1500:
                            # all 3001 rows probed: at most 47 workgroups emit at most 15 keys each, which cannot
                            # prove 1500 ranks - every query is served by the second launch
                            assert second == nq, (second, nq)
                            assert ivf.last_kernel_ms()[2] == 1  # (the single-query call just made)
    finally:
        ivf.close()
        flat.close()


# ---- 2: probe ties ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, d", [("f32", 100), ("f16", 385)])
def test_probe_ties_keep_the_lower_list(dtype, d):
    """Centroids in identical pairs, odd nprobe: the cut falls inside a pair and the lower list number stays in."""
    n, nlist = 1201, 38
    corpus = H.gauss(11 + d, n, d, normalize=False)
    base = H.gauss(12 + d, nlist // 2, d, normalize=False)
    cent = np.repeat(base, 2, axis=0)
    assert np.array_equal(cent[1::2], cent[0::2])
    assign = np.random.default_rng(13).integers(0, nlist, n).astype(np.int32)
    assert np.bincount(assign, minlength=nlist).min() > 0  # (the mate that must stay out has rows to betray it)
    q = H.gauss(14 + d, NQ, d, normalize=False)
    ivf = l2_index(d, cent, corpus, assign, dtype)
    try:
        dv = ref_dists(corpus, dtype, query_seen(q, False, dtype))
        Pall, dc = probe_l2(cent, q, nlist, False)
        for nprobe in (1, 5, 19):
            for i in range(NQ):  # the cut is inside a pair, for every query used
                lo, hi = Pall[i][nprobe - 1], Pall[i][nprobe]
                assert lo % 2 == 0 and hi == lo + 1 and dc[i][lo] == dc[i][hi], (nprobe, i)
            D, I = ivf.search(q, n, params=SearchParametersIVF(nprobe=nprobe))
            Dr, Ir, rows_of = ivf_l2_reference(corpus, cent, assign, q, n, nprobe, False, dtype, dists=dv)
            assert np.array_equal(I, Ir) and np.array_equal(D, Dr), nprobe
            for i in range(NQ):  # k = n: the returned rows ARE the probed set
                got = np.sort(I[i][I[i] >= 0])
                assert np.array_equal(got, rows_of[i]), (nprobe, i)
                assert np.array_equal(np.unique(assign[got]), np.sort(Pall[i][:nprobe])), (nprobe, i)
    finally:
        ivf.close()


# ---- 3: special values ------------------------------------------------------------------------------------------------------
def test_special_values():
    d, nlist, n = 100, 8, 400
    corpus = H.gauss(21, n, d, normalize=False)
    cent = H.gauss(22, nlist, d, normalize=False)
    cent[3, 5] = np.nan
    cent[5, 7] = np.inf
    assign = (np.arange(n) % nlist).astype(np.int32)
    q = H.gauss(23, NQ, d, normalize=False)
    q[0] = corpus[17]  # an exact match
    ivf = l2_index(d, cent, corpus, assign)
    try:
        D, I = ivf.search(q, n, params=SearchParametersIVF(nprobe=nlist))
        Dr, Ir, rows_of = ivf_l2_reference(corpus, cent, assign, q, n, nlist, False, "f32")
        assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
        for i in range(NQ):  # a NaN centroid and an inf centroid are never probed
            got = I[i][I[i] >= 0]
            assert got.size == n - 2 * (n // nlist) and not np.isin(assign[got], [3, 5]).any()
            assert (D[i][got.size:] == FMAX).all() and (I[i][got.size:] == -1).all()
        assert I[0, 0] == 17 and D[0, 0] == 0 and not np.signbit(D[0, 0])
    finally:
        ivf.close()
    # a NaN row is never returned, and lands in list 0 under the default assignment
    cent = H.gauss(22, nlist, d, normalize=False)
    bad = corpus.copy()
    bad[33, 2] = np.nan
    ivf = l2_index(d, cent, bad)
    try:
        a = ivf.assignment()
        assert a[33] == 0 and np.array_equal(a, nearest_l2(cent, bad))
        D, I = ivf.search(q, n, params=SearchParametersIVF(nprobe=nlist))
        assert not (I == 33).any() and ((I >= 0).sum(axis=1) == n - 1).all()
        Dr, Ir, _ = ivf_l2_reference(bad, cent, a, q, n, nlist, False, "f32")
        assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
    finally:
        ivf.close()
    # n == 0, and probing only empty lists: (+FLT_MAX, -1)
    ivf = l2_index(d, cent, np.zeros((0, d), np.float32))
    try:
        D, I = ivf.search(q, 5, params=SearchParametersIVF(nprobe=nlist))
        assert (D == FMAX).all() and (I == -1).all() and D.dtype == np.float32
        lims, Dr_, Ir_ = ivf.range_search(q, np.inf, params=SearchParametersIVF(nprobe=nlist))
        assert lims.tolist() == [0] * (NQ + 1) and Dr_.size == 0 and Ir_.size == 0
    finally:
        ivf.close()
    assign = 1 + (np.arange(n) % (nlist - 1)).astype(np.int32)  # list 0 is empty ...
    ivf = l2_index(d, cent, corpus, assign)
    try:
        q0 = np.ascontiguousarray(cent[:1])  # ... and it is the nearest list of this query
        assert probe_l2(cent, q0, 1, False)[0][0].tolist() == [0]
        D, I = ivf.search(q0, 5, params=SearchParametersIVF(nprobe=1))
        assert (D == FMAX).all() and (I == -1).all()
        assert (ivf.search(q0, 5, params=SearchParametersIVF(nprobe=2))[1][0] >= 0).all()
    finally:
        ivf.close()


# ---- 4: subsets and range ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, d", [("f32", 385), ("f32", 1000), ("f16", 513), ("f16", 1024)])
def test_subsets_and_range(dtype, d):
    corpus, cent, _ = make_data(dtype, d, "gauss")
    assign = uneven_assignment()
    q = H.gauss(31 + d, NQ, d, normalize=False)
    ivf = l2_index(d, cent, corpus, assign, dtype)
    nprobe = 5
    par = SearchParametersIVF(nprobe=nprobe)
    try:
        for normalize in (False, True):
            dv = ref_dists(corpus, dtype, query_seen(q, normalize, dtype))
            _, _, rows_all = ivf_l2_reference(corpus, cent, assign, q, 1, nprobe, normalize, dtype, dists=dv)
            # radii from the reference's own distances: nothing (the smallest probed distance of the call, and the
            # predicate is strict), 50 rows of query 0, every probed row
            d0 = np.sort(dv[0][rows_all[0]])
            r50 = np.float32((np.float64(d0[49]) + np.float64(d0[50])) / 2)
            assert d0[49] < r50 < d0[50]
            rmin = np.float32(min(dv[i][rows_all[i]].min() for i in range(NQ)))
            radii = [rmin, r50, np.inf]
            for name, sel in [("all", None)] + list(selections().items()):
                sub = ivf.subset(sel) if sel is not None else None
                among = None if sel is None else np.asarray(sel)
                ivf.nprobe = nprobe
                for k in (10, 400):
                    Dr, Ir, rows_of = ivf_l2_reference(corpus, cent, assign, q, k, nprobe, normalize, dtype, dists=dv,
                                                       among=among)
                    D, I = ivf.search(q, k, normalize=normalize, params=par if sub is None else sub)
                    assert np.array_equal(I, Ir) and np.array_equal(D, Dr), (name, normalize, k)
                for radius in radii:
                    want = ivf_l2_range_reference(dv, rows_of, radius)
                    got = ivf.range_search(q, radius, normalize=normalize, params=par if sub is None else sub)
                    for g, w in zip(got, want):
                        assert np.array_equal(g, w), (name, normalize, float(radius))
                    if radius == np.inf:
                        assert np.diff(want[0]).tolist() == [r.size for r in rows_of]
                    if radius is rmin:
                        assert want[0][-1] == 0  # (strict: the nearest row itself is out)
                    if radius is r50 and sel is None:
                        assert want[0][1] == 50
                for radius in (0.0, -1.0, -np.inf, np.nan):
                    lims, Dg, Ig = ivf.range_search(q, radius, normalize=normalize, params=par if sub is None else sub)
                    assert lims.tolist() == [0] * (NQ + 1) and Dg.size == 0 and Ig.size == 0
                if sub is not None:
                    sub.close()
    finally:
        ivf.close()


# ---- 5: assignment and build --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ivf_dims("f32"))
def test_assignment_kernel_equals_the_k1_search(d, monkeypatch):
    lib = native.load()
    monkeypatch.setenv("LS_IVF_ASSIGN_STEP", "1300")  # (three upload steps, the last one short)
    for kind in ("gauss", "int"):
        corpus, cent, _ = make_data("f32", d, kind)
        if kind == "int":
            cent[5] = cent[4]  # (identical centroids on top of the integer ties)
        quant = FlatL2Index.from_array(cent)
        _, Iq = quant.search(corpus, 1)
        quant.close()
        want = np.where(Iq[:, 0] >= 0, Iq[:, 0], 0).astype(np.int32)
        got = np.full(N, -7, np.int32)
        native.check(lib.ls_ivf_assign_l2(native.addr(corpus), N, d, native.addr(cent), NLIST, native.addr(got), 0))
        assert np.array_equal(got, want), kind
        assert np.array_equal(got, nearest_l2(cent, corpus)), kind
        if kind == "int":
            assert not (got == 5).any() and np.unique(got).size > 5
    assert lib.ls_ivf_assign_l2(None, 0, d, native.addr(cent), NLIST, None, 0) == native.LS_OK


@pytest.mark.parametrize("build_on_device", [False, True])
def test_default_assignment_of_a_built_index(build_on_device, monkeypatch):
    d = 385
    corpus, cent, _ = make_data("f32", d, "int")
    want = nearest_l2(cent, corpus)
    ix = l2_index(d, cent, corpus, build_on_device=build_on_device)
    assert np.array_equal(ix.assignment(), want)
    ix.close()
    if not build_on_device:  # the per-row search route of ls_ivf_create_l2: the same lists
        monkeypatch.setenv("LS_IVF_L2_ASSIGN", "search")
        ix = l2_index(d, cent, corpus[:500])
        assert np.array_equal(ix.assignment(), want[:500])
        ix.close()


def reseeding_rows():
    rng = np.random.default_rng(100)
    base = rng.standard_normal((200, 96)).astype(np.float32)
    return base[rng.integers(0, 200, 6000)]


@pytest.mark.parametrize("case", ["spread", "reseed"])
def test_training_on_device_equals_training_on_the_host(case):
    if case == "spread":
        x, d, nlist, seed = H.gauss(41, 6000, 64, normalize=False), 64, 24, 1234
    else:  # duplicated rows: two of the initial centroids are the same row, the higher list gets nothing
        x, d, nlist, seed = reseeding_rows(), 96, 24, 9
        rng = np.random.default_rng(seed)
        first = x[np.sort(rng.choice(x.shape[0], nlist, replace=False))]
        assert np.unique(first, axis=0).shape[0] < nlist
        assert np.bincount(nearest_l2(first, x), minlength=nlist).min() == 0  # an empty cluster at the first step
    dev = IVFFlatIndex(d, nlist, metric="l2")
    dev.train(x, niter=4, seed=seed, on_device=True)
    host = IVFFlatIndex(d, nlist, metric="l2")
    host.train(x, niter=4, seed=seed, on_device=False)
    assert np.array_equal(dev.centroids, host.centroids)
    assert np.isfinite(host.centroids).all()
    if case == "spread":
        ip = IVFFlatIndex(d, nlist)
        ip.train(x, niter=4, seed=seed)
        assert not np.array_equal(ip.centroids, host.centroids)  # (the metric does take part)
        ip.close()
    dev.close()
    host.close()


# ---- 6: add and remove ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_add_and_remove_equal_the_index_built_at_once(dtype):
    d = 193
    corpus, cent, _ = make_data(dtype, d, "gauss")
    q = H.gauss(51, NQ, d, normalize=False)
    n0 = 2000
    par = SearchParametersIVF(nprobe=5)

    def same(a, b, rows):
        assert a.ntotal == b.ntotal == rows.shape[0]
        assert np.array_equal(a.list_sizes(), b.list_sizes())
        assert np.array_equal(a.assignment(), b.assignment())
        assert np.array_equal(a.assignment(), nearest_l2(cent, rows))
        assert np.array_equal(a.reconstruct_n(), b.reconstruct_n())
        for k in (10, 600):
            Da, Ia = a.search(q, k, params=par)
            Db, Ib = b.search(q, k, params=par)
            assert np.array_equal(Ia, Ib) and np.array_equal(Da, Db)
            Dr, Ir, _ = ivf_l2_reference(rows, cent, a.assignment(), q, k, 5, False, dtype)
            assert np.array_equal(Ia, Ir) and np.array_equal(Da, Dr)

    ix = l2_index(d, cent, corpus[:n0], dtype=dtype)
    sel = np.arange(0, n0, 3)
    sub = ix.subset(sel)  # (builds the handle)
    assert sub.rows == sel.size
    ix.add(corpus[n0:])  # ls_ivf_add: the default assignment under L2
    once = l2_index(d, cent, corpus, dtype=dtype)
    same(ix, once, corpus)
    once.close()
    # the subset stays valid across the add and covers the rows it covered
    D, I = ix.search(q, 50, params=sub)
    Dr, Ir, _ = ivf_l2_reference(corpus, cent, ix.assignment(), q, 50, ix.nprobe, False, dtype, among=sel)
    assert sub.valid and sub.rows == sel.size and np.array_equal(I, Ir) and np.array_equal(D, Dr)
    stale = np.arange(1, N, 4)
    assert ix.remove_ids(stale) == stale.size
    keep = np.setdiff1d(np.arange(N), stale)
    once = l2_index(d, cent, corpus[keep], dtype=dtype)
    same(ix, once, corpus[keep])
    once.close()
    # ... and shrinks across the remove: its surviving rows under their new numbers
    left = np.searchsorted(keep, np.intersect1d(sel, keep))
    assert sub.valid and sub.rows == left.size < sel.size
    D, I = ix.search(q, 50, params=sub)
    Dr, Ir, _ = ivf_l2_reference(corpus[keep], cent, ix.assignment(), q, 50, ix.nprobe, False, dtype, among=left)
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
    ix.close()


# ---- 7: beside it ---------------------------------------------------------------------------------------------------------------
def test_the_inner_product_index_is_unchanged_beside_it():
    d = 385
    corpus, cent = H.gauss(61, N, d), H.gauss(62, NLIST, d)
    assign = uneven_assignment()
    q = H.gauss(63, NQ, d)
    ip = IVFFlatIndex(d, NLIST)
    ip.set_centroids(cent)
    ip.add(corpus, assign=assign)
    l2 = l2_index(d, cent, corpus, assign)
    try:
        assert metric_of(ip) == native.LS_METRIC_INNER_PRODUCT == 0 and metric_of(l2) == native.LS_METRIC_L2
        assert ip.metric == "ip" and l2.metric == "l2"
        for small in (False, True):
            ip.set_small_batch(small)
            for nprobe, k in ((1, 10), (5, 10), (NLIST, 1500)):
                D, I = ip.search(q, k, params=SearchParametersIVF(nprobe=nprobe))
                Dr, Ir, _ = ivf_reference(corpus, cent, assign, q, k, nprobe, False, "f32")
                assert np.array_equal(I, Ir) and np.array_equal(D, Dr), (small, nprobe, k)
        with pytest.raises(ValueError, match="L2"):
            l2.set_small_batch(True)
        rc = native.load().ls_ivf_set_small_batch(l2._handle, 1)  # the library itself refuses
        assert rc == native.LS_ERR_INVALID_ARG and b"L2" in native.load().ls_last_error()
        assert native.load().ls_ivf_set_small_batch(l2._handle, 0) == native.LS_OK
        # the two metrics disagree on this data (unit rows, but the centroids are not): the L2 index is not the IP one
        D2, I2 = l2.search(q, 10, params=SearchParametersIVF(nprobe=NLIST))
        Df, If = exact_topk_l2(ref_dists(corpus, "f32", q)[0], 10)
        assert np.array_equal(I2[0], If) and np.array_equal(D2[0], Df)
    finally:
        ip.close()
        l2.close()


# ---- 8: faiss_compat ------------------------------------------------------------------------------------------------------------
def test_faiss_compat_index_ivf_flat_l2(tmp_path):
    d, nlist = 96, 16
    x = H.gauss(71, 5000, d, normalize=False)
    q = H.gauss(72, 6, d, normalize=False)
    ix = faiss_compat.IndexIVFFlatL2(faiss_compat.IndexFlatL2(d), d, nlist, build_on_device=True)
    assert not ix.is_trained
    ix.train(x, niter=3)
    ix.add(x)
    ix.nprobe = 4
    D, I = ix.search(q, 20)
    a = ix.assignment()
    assert np.array_equal(a, nearest_l2(ix.centroids, x))
    Dr, Ir, _ = ivf_l2_reference(x, ix.centroids, a, q, 20, 4, False, "f32")
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
    Dq, Iq = ix.quantizer.search(q, 4)  # faiss's index.quantizer: the probe lists themselves
    assert np.array_equal(Iq, probe_l2(ix.centroids, q, 4, False)[0])
    p = tmp_path / "ivf_l2.index"
    faiss_compat.write_index(ix, p)
    back = faiss_compat.read_index(p, ivf=True)
    assert back.metric == "l2" and back.nprobe == 4 and back.ntotal == 5000
    D2, I2 = back.search(q, 20)
    assert np.array_equal(I2, I) and np.array_equal(D2, D)
    assert np.array_equal(back.assignment(), a) and metric_of(back) == native.LS_METRIC_L2
    with pytest.raises(ValueError, match="not an inner-product index"):
        faiss_compat.read_index(p)
    ix.close()
    back.close()
