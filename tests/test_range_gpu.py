"""Range search on the GPU (include/leansearch_range.h): lims, rows and scores of ``range_search`` bit for bit against
host references thresholded in numpy - tests/test_geometry_cpu.py's ``Flat`` / ``ivf_reference`` /
``uneven_assignment`` (f32: the scan kernels' own summation order; f16: integer-valued rows; sq8: tests/sq8_ref.c).
A reference is a full score matrix [nq, n] with NaN where a row is not searched (or never returned); the expected
result of a radius is its rows above the radius, ascending."""

import ctypes
import functools

import numpy as np
import pytest

from lean_explore_amd import faiss_compat as fc
from lean_explore_amd import native
from lean_explore_amd.index import FlatIPIndex
from lean_explore_amd.ivf import IVFFlatIndex
from tests.test_geometry_cpu import Flat, ivf_reference, seen_queries, uneven_assignment

pytestmark = pytest.mark.gpu

NEG = np.float32(-np.finfo(np.float32).max)
INF = float("inf")
SLAB = 1024  # LS_RANGE_SLAB (csrc/ls_range_plan.h)


# ---- references ------------------------------------------------------------------------------------------------------------
def score_matrix(flat, rows, qn, n):
    """[nq, n] float32: the reference's score of every row of ``rows`` it would ever return, NaN elsewhere."""
    S = np.full((qn.shape[0], n), np.nan, np.float32)
    if rows.size:
        D, I = flat.topk(rows, qn, rows.size)
        for i in range(qn.shape[0]):
            ok = I[i] >= 0
            S[i, I[i][ok]] = D[i][ok]
    return S


def expected(S, radius, base=0):
    """(lims, D, I) of a score matrix: rows strictly above the radius, not NaN, above -FLT_MAX; row ascending."""
    with np.errstate(invalid="ignore"):
        hit = (S > np.float32(radius)) & (S > NEG)
    lims = np.concatenate([[0], np.cumsum(hit.sum(axis=1))]).astype(np.uint64)
    I = np.concatenate([np.flatnonzero(h) for h in hit]).astype(np.int64) + base
    return lims, (S[hit] + np.float32(0.0)).astype(np.float32), I


def assert_range(got, want, what=""):
    for name, g, w in zip(("lims", "D", "I"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name)


def quantile_radii(S):
    """About 0, about 1 %, about 50 % and 100 % of the rows hit: taken from the reference's own scores."""
    v = np.sort(S[~np.isnan(S)])
    return [float(v[-1]), float(v[int(0.99 * v.size)]), float(v[v.size // 2]), -INF]


def masked(S, rows_of):
    out = np.full_like(S, np.nan)
    for i, rows in enumerate(rows_of):
        out[i, rows] = S[i, rows]
    return out


# ---- shared data -------------------------------------------------------------------------------------------------------------
N, D_PAR, NQ = 6000, 100, 11  # (groups of 8 + 3)
D_IVF, NLIST = 64, 37


@functools.lru_cache(maxsize=None)
def data(dtype, d):
    rng = np.random.default_rng(17 + d)
    if dtype == "f16":  # integer-valued rows and queries: every f16 product and f32 sum is exact in any order
        x = rng.integers(-4, 5, (N, d)).astype(np.float32)
        q = rng.integers(-4, 5, (NQ, d)).astype(np.float32)
    else:
        x = rng.standard_normal((N, d), dtype=np.float32)
        q = rng.standard_normal((NQ, d), dtype=np.float32)
    return x, q


@functools.lru_cache(maxsize=None)
def flat_ref(dtype, d, normalize):
    """(Flat, full score matrix over all rows) of data(dtype, d) for the queries as the kernels see them."""
    x, q = data(dtype, d)
    flat = Flat(x, dtype)
    S = score_matrix(flat, np.arange(N), seen_queries(q, normalize), N)
    S.setflags(write=False)
    return flat, S


@functools.lru_cache(maxsize=None)
def ivf_parts():
    rng = np.random.default_rng(23)
    return rng.standard_normal((NLIST, D_IVF), dtype=np.float32), uneven_assignment(n=N, nlist=NLIST)


def make_ivf(dtype, x=None, assign=None, **kw):
    cent, a = ivf_parts()
    ivf = IVFFlatIndex(D_IVF, NLIST, dtype=dtype, **kw)
    ivf.set_centroids(cent)
    ivf.add(data(dtype, D_IVF)[0] if x is None else x, assign=a if assign is None else assign)
    return ivf


def probed_rows(dtype, nprobe, assign=None, x=None):
    cent, a = ivf_parts()
    xx, q = data(dtype, D_IVF)
    _, _, rows_of = ivf_reference(xx if x is None else x, cent, a if assign is None else assign, q, 1, nprobe, False,
                                  dtype, flat=flat_ref(dtype, D_IVF, False)[0] if x is None else None)
    return rows_of


# ---- 1. injected scores ------------------------------------------------------------------------------------------------------
N_INJ, D_INJ = 3 * SLAB + 17, 32
SCALES = (1.0, 0.5, -1.0)


def injected(name):
    n = N_INJ
    r = np.arange(n)
    if name == "all_equal":
        return np.full(n, 0.75, np.float32)
    if name == "all_above":  # (of the float just below 0.75, and of -inf)
        s = np.full(n, 1.5, np.float32)
        s[64] = 0.75
        return s
    if name == "slab_edges":
        s = np.zeros(n, np.float32)
        s[[0, 63, 64, SLAB - 1, SLAB, n - 1]] = 2.0
        s[64] = 0.75  # (the present score the radii are taken from)
        return s
    if name == "every_other":
        s = np.where(r % 2, 1.0, -1.0).astype(np.float32)
        s[64] = 0.75
        return s
    if name == "one_slab_full":
        s = np.zeros(n, np.float32)
        s[SLAB:2 * SLAB] = 1.0
        s[64] = 0.75
        return s
    assert name == "specials"
    s = np.random.default_rng(3).standard_normal(n).astype(np.float32)
    s[5::7] = np.nan
    s[6::11] = NEG
    s[9::13] = np.inf
    s[64] = 0.75
    return s


@pytest.mark.parametrize("name", ["all_equal", "all_above", "slab_edges", "every_other", "one_slab_full", "specials"])
def test_injected_scores(name):
    """The corpus is zero except column 0 = s and the queries are a * e0, so every score is exactly a * s[r] in any
    summation order. Radii: equal to a present score (that row is excluded), the float just below it (included), -inf,
    +inf, NaN."""
    s = injected(name)
    corpus = np.zeros((N_INJ, D_INJ), np.float32)
    corpus[:, 0] = s
    q = np.zeros((len(SCALES), D_INJ), np.float32)
    q[:, 0] = SCALES
    with np.errstate(invalid="ignore", over="ignore"):
        S = np.asarray(SCALES, np.float32)[:, None] * s[None, :]
    ix = FlatIPIndex.from_array(corpus)
    try:
        v = np.float32(0.75)
        for radius in (float(v), float(np.nextafter(v, np.float32(-np.inf))), -INF, INF, float("nan")):
            want = expected(S, radius)
            got = ix.range_search(q, radius)
            assert_range(got, want, (name, radius))
            if radius == float(v):
                assert 64 not in got[2][:int(got[0][1])]  # the row that scores exactly the radius is excluded
            if radius == float(np.nextafter(v, np.float32(-np.inf))):
                assert 64 in got[2][:int(got[0][1])]      # ... and included just below it
        if name == "all_equal":
            assert ix.range_search(q[:1], 0.75)[0].tolist() == [0, 0]
        if name == "specials":
            lims, Dv, Iv = ix.range_search(q[:1], -INF)
            assert not np.isnan(Dv).any() and (Dv > NEG).all() and np.isinf(Dv).any()
    finally:
        ix.close()


# ---- 2. parity per dtype -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16", "sq8"])
def test_parity(dtype):
    x, q = data(dtype, D_PAR)
    ix = FlatIPIndex.from_array(x, dtype=dtype)
    try:
        for normalize in ((False,) if dtype == "f16" else (False, True)):
            _, S = flat_ref(dtype, D_PAR, normalize)
            radii = quantile_radii(S)
            hits = [int(expected(S, r)[0][-1]) for r in radii]
            print(dtype, "normalize" if normalize else "raw", "radii", radii, "hits", hits)
            assert hits[0] == 0 and 0 < hits[1] < hits[2] < hits[3] == S.size
            for radius in radii:
                got = ix.range_search(q, radius, normalize=normalize)
                assert_range(got, expected(S, radius), (dtype, normalize, radius))
                if dtype == "f16":  # the option changes nothing: range search stays on the scan kernel
                    ix.set_f16_small_batch(True)
                    assert_range(ix.range_search(q, radius), got, "f16_small_batch on")
                    ix.set_f16_small_batch(False)
            # a query's result does not depend on its company
            lims, Dv, Iv = ix.range_search(q, radii[1], normalize=normalize)
            for i in (0, 8, NQ - 1):
                l1, D1, I1 = ix.range_search(q[i:i + 1], radii[1], normalize=normalize)
                a, b = int(lims[i]), int(lims[i + 1])
                assert l1.tolist() == [0, b - a] and np.array_equal(D1, Dv[a:b]) and np.array_equal(I1, Iv[a:b])
    finally:
        ix.close()


# ---- 3. agreement with top-k -------------------------------------------------------------------------------------------------
def filtered_topk(D, I, radius):
    """search(k) filtered by D > radius and re-sorted by row, as (lims, D, I)."""
    Ds, Is, lims = [], [], [0]
    for i in range(D.shape[0]):
        ok = (I[i] >= 0) & (D[i] > np.float32(radius))
        order = np.argsort(I[i][ok], kind="stable")
        Ds.append(D[i][ok][order])
        Is.append(I[i][ok][order])
        lims.append(lims[-1] + int(ok.sum()))
    return np.asarray(lims, np.uint64), np.concatenate(Ds).astype(np.float32), np.concatenate(Is).astype(np.int64)


@pytest.mark.parametrize("kind", ["flat", "subset", "ivf"])
def test_agrees_with_top_k(kind):
    """Where a query has at most 100 hits, search(k = 100) filtered by D > radius and sorted by row is the range
    result."""
    x, q = data("f32", D_IVF)
    params = None
    if kind == "ivf":
        ix = make_ivf("f32")
        ix.nprobe = 4
    else:
        ix = FlatIPIndex.from_array(x)
        if kind == "subset":
            params = ix.subset(np.random.default_rng(2).random(N) < 0.10)
    try:
        D100, I100 = ix.search(q, 100, params=params)
        radius = float(D100[:, 59].max())  # every query has fewer than 60 rows above it
        want = filtered_topk(D100, I100, radius)
        assert 0 < int(want[0][-1]) and (np.diff(want[0].astype(np.int64)) <= 60).all()
        assert_range(ix.range_search(q, radius, params=params), want, kind)
    finally:
        ix.close()


# ---- 4. subsets --------------------------------------------------------------------------------------------------------------
def test_subsets():
    x, q = data("f32", D_PAR)
    _, S = flat_ref("f32", D_PAR, False)
    radii = quantile_radii(S)[1:]
    rng = np.random.default_rng(8)
    ix = FlatIPIndex.from_array(x)
    based = FlatIPIndex.from_array(x, base=1000)
    try:
        for name, mask in (("random 10 %", rng.random(N) < 0.10), ("block", (np.arange(N) >= 1500) & (np.arange(N) < 2789)),
                           ("empty", np.zeros(N, bool))):
            rows = np.flatnonzero(mask)
            Sm = masked(S, [rows] * NQ)
            sub = ix.subset(mask)
            assert sub.rows == rows.size
            for radius in radii:
                assert_range(ix.range_search(q, radius, params=sub), expected(Sm, radius), (name, radius))
            sub.close()
            if name == "empty":
                assert ix.range_search(q, -INF, params=fc.SearchParameters(sel=mask))[0].tolist() == [0] * (NQ + 1)
        # a raw selector in params: a subset for this call only
        sel = fc.IDSelectorRange(100, 1333)
        Sm = masked(S, [np.arange(100, 1333)] * NQ)
        assert_range(ix.range_search(q, radii[0], params=fc.SearchParameters(sel=sel)), expected(Sm, radii[0]), "selector")
        assert_range(ix.range_search(q, -INF, params=fc.SearchParameters(sel=sel)), expected(Sm, -INF), "selector, all")
        # base: original rows plus base, on the plain call and on a subset
        assert_range(based.range_search(q, radii[0]), expected(S, radii[0], base=1000), "base")
        assert_range(based.range_search(q, radii[1], params=fc.SearchParameters(sel=sel)),
                     expected(Sm, radii[1], base=1000), "base, selector")
    finally:
        ix.close()
        based.close()


# ---- 5. IVF ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16", "sq8"])
def test_ivf(dtype):
    x, q = data(dtype, D_IVF)
    _, S = flat_ref(dtype, D_IVF, False)
    radii = quantile_radii(S)
    ivf = make_ivf(dtype)
    flat = FlatIPIndex.from_array(x, dtype=dtype)
    try:
        assert (ivf.list_sizes() == 0).sum() >= 2  # (empty lists included)
        for nprobe in (1, 4, NLIST):
            ivf.nprobe = nprobe
            Sp = masked(S, probed_rows(dtype, nprobe))
            for radius in radii:
                got = ivf.range_search(q, radius)
                assert_range(got, expected(Sp, radius), (dtype, nprobe, radius))
                if nprobe == NLIST:  # every list probed: the flat range search of the same rows
                    assert_range(got, flat.range_search(q, radius), (dtype, "flat", radius))
        # params.nprobe overrides the attribute for one call
        ivf.nprobe = 1
        assert_range(ivf.range_search(q, radii[2], params=fc.SearchParametersIVF(nprobe=4)),
                     expected(masked(S, probed_rows(dtype, 4)), radii[2]), "params.nprobe")
    finally:
        ivf.close()
        flat.close()


def test_ivf_subset_and_small_batch():
    dtype = "f32"
    x, q = data(dtype, D_IVF)
    _, S = flat_ref(dtype, D_IVF, False)
    radii = quantile_radii(S)
    mask = np.random.default_rng(4).random(N) < 0.3
    ivf = make_ivf(dtype)
    try:
        sub = ivf.subset(mask)
        for nprobe in (1, 4, NLIST):
            ivf.nprobe = nprobe
            rows_of = [r[mask[r]] for r in probed_rows(dtype, nprobe)]
            Sp = masked(S, rows_of)
            for radius in radii[1:]:
                assert_range(ivf.range_search(q, radius, params=sub), expected(Sp, radius), ("subset", nprobe, radius))
        empty = ivf.subset(np.zeros(N, bool))
        assert ivf.range_search(q, -INF, params=empty)[0].tolist() == [0] * (NQ + 1)
        # small_batch=True changes nothing (range search launches per query), and the searches around it stay the same
        ivf.nprobe = 4
        before = ivf.range_search(q, radii[1])
        Dk, Ik = ivf.search(q, 10)
        ivf.set_small_batch(True)
        assert_range(ivf.range_search(q, radii[1]), before, "small_batch")
        Dk2, Ik2 = ivf.search(q, 10)
        assert np.array_equal(Dk, Dk2) and np.array_equal(Ik, Ik2)
        assert_range(ivf.range_search(q, radii[1]), before, "small_batch, after a batched search")
    finally:
        ivf.close()


# ---- 6. after mutation -------------------------------------------------------------------------------------------------------
def test_flat_after_remove_and_add():
    x, q = data("f32", D_PAR)
    _, S = flat_ref("f32", D_PAR, False)
    rng = np.random.default_rng(12)
    gone = rng.random(N) < 0.10
    keep = np.flatnonzero(~gone)
    submask = rng.random(N) < 0.25
    ix = FlatIPIndex.from_array(x)
    try:
        sub = ix.subset(submask)  # made before the removal: covers its survivors under their new numbers
        assert ix.remove_ids(gone) == int(gone.sum())
        S1 = np.ascontiguousarray(S[:, keep])
        lims, Dv, Iv = ix.range_search(q, -INF)
        assert np.array_equal(Iv.reshape(NQ, -1), np.tile(np.arange(keep.size), (NQ, 1)))  # no pad row, none missing
        assert_range((lims, Dv, Iv), expected(S1, -INF), "after remove_ids")
        radius = quantile_radii(S1)[1]
        assert_range(ix.range_search(q, radius), expected(S1, radius), "after remove_ids, 1 %")
        sub_rows = np.flatnonzero(submask[keep])
        assert sub.rows == sub_rows.size
        assert_range(ix.range_search(q, radius, params=sub), expected(masked(S1, [sub_rows] * NQ), radius), "old subset")
        extra = np.random.default_rng(13).standard_normal((63, D_PAR), dtype=np.float32)
        ix.add(extra)
        x2 = np.concatenate([x[keep], extra])
        S2 = score_matrix(Flat(x2, "f32"), np.arange(x2.shape[0]), q, x2.shape[0])
        assert np.array_equal(S2[:, :keep.size], S1)
        lims, Dv, Iv = ix.range_search(q, -INF)
        assert np.array_equal(Iv.reshape(NQ, -1), np.tile(np.arange(x2.shape[0]), (NQ, 1)))
        assert_range((lims, Dv, Iv), expected(S2, -INF), "after add")
        assert_range(ix.range_search(q, radius, params=sub), expected(masked(S1, [sub_rows] * NQ), radius),
                     "old subset after add")  # (an add does not extend it)
    finally:
        ix.close()


def test_ivf_after_add_and_remove():
    dtype = "f32"
    x, q = data(dtype, D_IVF)
    cent, assign = ivf_parts()
    rng = np.random.default_rng(14)
    extra = rng.standard_normal((63, D_IVF), dtype=np.float32)
    extra_assign = rng.integers(1, NLIST, 63).astype(np.int32)
    gone = rng.random(N + 63) < 0.10
    keep = np.flatnonzero(~gone)
    x2, a2 = np.concatenate([x, extra])[keep], np.concatenate([assign, extra_assign])[keep]
    ivf = make_ivf(dtype)
    fresh = make_ivf(dtype, x=x2, assign=a2)
    try:
        ivf.nprobe = fresh.nprobe = 4
        ivf.range_search(q, 0.0)  # (built, and its range vectors sized for the old n)
        ivf.add(extra, assign=extra_assign)
        assert ivf.remove_ids(gone) == int(gone.sum())
        S2 = score_matrix(Flat(x2, dtype), np.arange(x2.shape[0]), q, x2.shape[0])
        Sp = masked(S2, probed_rows(dtype, 4, assign=a2, x=x2))
        for radius in (quantile_radii(S2)[1], -INF):
            got = ivf.range_search(q, radius)
            assert_range(got, fresh.range_search(q, radius), ("fresh", radius))
            assert_range(got, expected(Sp, radius), ("reference", radius))
    finally:
        ivf.close()
        fresh.close()


# ---- 7. neighbours undisturbed -----------------------------------------------------------------------------------------------
def test_neighbours_are_undisturbed():
    import torch

    x, q = data("f32", D_PAR)
    _, S = flat_ref("f32", D_PAR, False)
    radius = quantile_radii(S)[1]
    k = 10
    ix = FlatIPIndex.from_array(x)
    try:
        D0, I0 = ix.search(q, k)  # what every top-k call gives without range calls in between
        qd = torch.from_numpy(q[:3]).cuda()
        D1, I1 = ix.search(q, k)
        r1 = ix.range_search(q, radius)
        ds, di = ix.search_device(qd, k, pipeline=True)  # left pending
        r2 = ix.range_search(q, radius)
        ix.check()
        D2, I2 = ix.search(q, k)
        assert np.array_equal(D1, D0) and np.array_equal(I1, I0) and np.array_equal(D2, D0) and np.array_equal(I2, I0)
        assert np.array_equal(ds.cpu().numpy(), D0[:3]) and np.array_equal(di.cpu().numpy(), I0[:3])
        assert_range(r1, expected(S, radius), "first")
        assert_range(r2, r1, "second")
    finally:
        ix.close()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals():
    x, q = data("f32", D_IVF)
    lib = native.load()
    for kw, kind in ((dict(devices=[0, 0]), "sharded"), (dict(devices=[0, 0], replicate=True), "replicated")):
        grp = FlatIPIndex.from_array(x[:500], **kw)
        try:
            with pytest.raises(ValueError, match=kind):
                grp.range_search(q, 0.0)
            with pytest.raises(ValueError, match=kind):
                grp.range_search(q, 0.0, params=fc.SearchParameters(sel=np.ones(500, bool)))
            D1, I1 = grp.search(q, 5)  # the handle is as it was
            assert (I1 >= 0).all()
        finally:
            grp.close()
    ix = FlatIPIndex.from_array(x)
    other = FlatIPIndex.from_array(x[:100])
    ivf, ivf2 = make_ivf("f32"), make_ivf("f32")
    try:
        res = ctypes.c_void_p(0x5a5a)
        for flags in (native.LS_FLAG_ASYNC, native.LS_FLAG_NORMALIZE | native.LS_FLAG_PIPELINE):
            assert lib.ls_range_search(ix._handle, native.addr(q), NQ, 0.0, flags, ctypes.byref(res)) == native.LS_ERR_INVALID_ARG
            assert res.value is None and b"only LS_FLAG_NORMALIZE" in lib.ls_last_error()
            assert lib.ls_ivf_range_search(ivf._ensure_built(), native.addr(q), NQ, 0.0, 4, flags,
                                           ctypes.byref(res)) == native.LS_ERR_INVALID_ARG
        assert lib.ls_range_search(ix._handle, native.addr(q), NQ, 0.0, 0, None) == native.LS_ERR_INVALID_ARG
        assert lib.ls_ivf_range_search(ivf._handle, native.addr(q), NQ, 0.0, 4, 0, None) == native.LS_ERR_INVALID_ARG
        assert lib.ls_range_search_subset(ix._handle, 12345, native.addr(q), NQ, 0.0, 0, ctypes.byref(res)) == native.LS_ERR_INVALID_ARG
        assert res.value is None and b"no subset 12345" in lib.ls_last_error()
        assert lib.ls_ivf_range_search_subset(ivf._handle, 12345, native.addr(q), NQ, 0.0, 4, 0,
                                              ctypes.byref(res)) == native.LS_ERR_INVALID_ARG
        assert res.value is None and b"no subset 12345" in lib.ls_last_error()
        with pytest.raises(ValueError, match="another index"):
            ix.range_search(q, 0.0, params=other.subset(np.ones(100, bool)))
        with pytest.raises(ValueError, match="another index"):
            ivf.range_search(q, 0.0, params=ivf2.subset(np.ones(N, bool)))
        with pytest.raises(ValueError, match="range_search expects"):
            ix.range_search(q[:, :-1], 0.0)
        # nq = 0 through the C entry point: lims = [0]
        assert lib.ls_range_search(ix._handle, None, 0, 0.0, 0, ctypes.byref(res)) == native.LS_OK
        assert lib.ls_range_nq(res) == 0 and ctypes.c_int64.from_address(lib.ls_range_lims(res)).value == 0
        lib.ls_range_free(res)
        # an empty index launches nothing
        empty = FlatIPIndex(D_IVF)
        assert empty.range_search(q, -INF)[0].tolist() == [0] * (NQ + 1)
        empty.close()
    finally:
        for h in (ix, other, ivf, ivf2):
            h.close()


# ---- 9. many hits ------------------------------------------------------------------------------------------------------------
def test_many_hits():
    """8 x 70 000 results: slab offsets past 2^16 and device result buffers regrown between calls."""
    n, d, nq = 70_000, 16, 8
    rng = np.random.default_rng(21)
    x = rng.standard_normal((n, d), dtype=np.float32)
    q = rng.standard_normal((nq, d), dtype=np.float32)
    S = score_matrix(Flat(x, "f32"), np.arange(n), q, n)
    ix = FlatIPIndex.from_array(x)
    try:
        assert_range(ix.range_search(q[:1], float(np.sort(S[0])[-10])), expected(S[:1], float(np.sort(S[0])[-10])), "few")
        lims, Dv, Iv = ix.range_search(q, -INF)
        assert lims.tolist() == [i * n for i in range(nq + 1)]
        assert_range((lims, Dv, Iv), expected(S, -INF), "all")
    finally:
        ix.close()
