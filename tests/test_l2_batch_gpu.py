"""Several L2 queries per corpus pass on the MI355X (include/leansearch_l2_batch.h): every row geometry
of the scan kernel's L2 instantiations at 4 and 8 queries per launch, every group split of a call, the place of a query
in its group, special values and fp16 subnormals, forced retries, concurrent callers, mutation, the handles beside it,
faiss_compat.

Every comparison is np.array_equal on D and I: against tests/l2_ref.c (or integer arithmetic) under the library's order,
against the same call with the switch off, and against the queries served one by one. Debug counter 38 counts the
launches that carried more than one query. Nothing is timed."""

import threading

import numpy as np
import pytest

from lean_explore_amd import faiss_compat, native
from lean_explore_amd.index import FlatIPIndex, FlatL2Index
from lean_explore_amd.ivf import IVFFlatIndex
from tests import helpers as H
from tests.test_geometry_cpu import DIMS, GEOMS, N, PER_CHUNK, geom_of
from tests.test_l2_cpu import FMAX, int_dists, query_seen, ref_dists, topk_l2

pytestmark = pytest.mark.gpu

KS = (1, 10, 2048)
NQS = (2, 3, 4, 5, 7, 8, 9, 13, 16, 17)
NQ_MAX = max(NQS)


def batch_dims(dtype):
    """One full and one ragged d per shared geometry, taken from DIMS."""
    per, out = PER_CHUNK[dtype], []
    for g in GEOMS[dtype]:
        ds = [d for d in DIMS[dtype] if geom_of(dtype, d) == g]
        out += [max(d for d in ds if d % per == 0), max(d for d in ds if d % per)]
    return out


CASES = [(dtype, d, kind) for dtype in ("f32", "f16") for d in batch_dims(dtype) for kind in ("gauss", "int")]


def group_launches(nq, dtype="f32", d=384):
    """Launches of a call of nq queries that carry more than one query: groups of 8 (5 or more left), 4 (2..4), 1. The
    declined shapes: fp16 rows of 16 lanes x 2 chunks and of 4-chunk lanes go out in groups of 4."""
    declined8 = dtype == "f16" and (geom_of(dtype, d) == (16, 2) or geom_of(dtype, d)[1] == 4)
    count, left = 0, nq
    while left > 0:
        size = 8 if left >= 5 and not declined8 else (4 if left >= 2 else 1)
        count += size > 1
        left -= min(size, left)
    return count


def same(got, want, what):
    assert np.array_equal(got[1], want[1]), f"{what}: rows differ"
    assert np.array_equal(got[0], want[0]), f"{what}: distances differ"


def test_the_dimensions_cover_every_shared_geometry_twice():
    for dtype in ("f32", "f16"):
        dims = batch_dims(dtype)
        assert len(dims) == 16 and sorted({geom_of(dtype, d) for d in dims}) == sorted(GEOMS[dtype])
        for g in GEOMS[dtype]:
            mine = [d for d in dims if geom_of(dtype, d) == g]
            assert len(mine) == 2 and sum(d % PER_CHUNK[dtype] == 0 for d in mine) == 1
    assert [group_launches(nq) for nq in NQS] == [1, 1, 1, 1, 1, 1, 1, 2, 2, 2]
    assert [group_launches(nq, "f16", 256) for nq in NQS] == [1, 1, 1, 1, 2, 2, 2, 3, 4, 4]


# ---- 1: every geometry, every group split ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, d, kind", CASES)
def test_every_geometry_and_group_split(dtype, d, kind):
    seed = 12000 + 3 * d + {"f32": 1, "f16": 2}[dtype]
    if kind == "int":  # (no normalisation: it would leave the exact regime)
        corpus, q, runs = H.int_corpus(seed, N, d), H.int_corpus(seed + 1, NQ_MAX, d), (False,)
    else:
        corpus, q, runs = H.gauss(seed, N, d), H.gauss(seed + 1, NQ_MAX, d), (True, False)
        q[:2] *= np.float32(2.5)  # (queries 0, 1: the fused normalisation has something to do)
    ix = FlatL2Index.from_array(corpus, dtype=dtype)
    try:
        assert ix.l2_small_batch is False and native.load().ls_l2_small_batch(ix._handle) == 0
        for normalize in runs:
            dist = int_dists(corpus, q) if kind == "int" else ref_dists(corpus, dtype, query_seen(q, normalize, dtype))
            want = {k: topk_l2(dist, k) for k in KS}
            # the switch off: the calls as they were, and every query alone
            ix.set_l2_small_batch(False)
            c38 = ix.debug_counter(38)
            off = {(nq, k): ix.search(q[:nq], k, normalize=normalize) for nq in NQS for k in KS}
            alone = {k: [ix.search(q[i:i + 1], k, normalize=normalize) for i in range(NQ_MAX)] for k in KS}
            assert ix.debug_counter(38) == c38, "a group launch with the switch off"
            for k in KS:
                same(off[(NQ_MAX, k)], want[k], f"switch off k={k}")
            # the switch on
            ix.set_l2_small_batch(True)
            assert ix.l2_small_batch is True and native.load().ls_l2_small_batch(ix._handle) == 1
            for nq in NQS:
                for k in KS:
                    c38 = ix.debug_counter(38)
                    got = ix.search(q[:nq], k, normalize=normalize)
                    what = f"nq={nq} k={k} normalize={normalize}"
                    assert ix.debug_counter(38) - c38 == group_launches(nq, dtype, d), what  # (a retry is a single-query launch)
                    same(got, (want[k][0][:nq], want[k][1][:nq]), what + " against the reference")
                    same(got, off[(nq, k)], what + " against the switch off")
                    for i in range(nq):
                        assert np.array_equal(got[0][i], alone[k][i][0][0]) and np.array_equal(got[1][i], alone[k][i][1][0]), \
                            what + f": query {i} alone differs"
            # a lone query with the switch on is the single-query launch
            c38 = ix.debug_counter(38)
            same(ix.search(q[3:4], 10, normalize=normalize), alone[10][3], "a lone query")
            assert ix.debug_counter(38) == c38
        assert ix.debug_counter(23) == 0 and ix.debug_counter(34) == 0 and ix.debug_counter(36) == 0
    finally:
        ix.close()


# ---- 2: company does not matter ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, d", [("f32", 385), ("f16", 767)])  # (shapes served at 8 queries per launch)
def test_a_query_returns_the_same_bits_in_every_slot_of_a_group(dtype, d):
    corpus = H.gauss(300 + d, N, d)
    others = H.gauss(301 + d, 64, d, normalize=False)
    mine = H.gauss(302 + d, 1, d, normalize=False)[0] * np.float32(1.7)
    ix = FlatL2Index.from_array(corpus, dtype=dtype, l2_small_batch=True)
    try:
        for normalize in (False, True):
            for k in (10, 2048):
                ix.set_l2_small_batch(False)
                want = ix.search(mine[None, :], k, normalize=normalize)
                same(want, topk_l2(ref_dists(corpus, dtype, query_seen(mine[None, :], normalize, dtype)), k), "alone")
                ix.set_l2_small_batch(True)
                for slot in range(8):
                    q = np.ascontiguousarray(others[8 * slot:8 * slot + 8])  # (seven other queries each time)
                    q[slot] = mine
                    c38 = ix.debug_counter(38)
                    D, I = ix.search(q, k, normalize=normalize)
                    assert ix.debug_counter(38) - c38 == 1
                    assert np.array_equal(D[slot], want[0][0]) and np.array_equal(I[slot], want[1][0]), (slot, k, normalize)
                # ... and as the padded tail of a group of 4 and of 8
                for nq in (2, 3, 5, 7):
                    q = np.ascontiguousarray(others[:nq])
                    q[nq - 1] = mine
                    D, I = ix.search(q, k, normalize=normalize)
                    assert np.array_equal(D[nq - 1], want[0][0]) and np.array_equal(I[nq - 1], want[1][0]), (nq, k, normalize)
    finally:
        ix.close()


# ---- 3: special values -------------------------------------------------------------------------------------------------
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
    q = np.ascontiguousarray(corpus[[5, 100, 1, 2, 3, 4, 6, 7]])
    q[5] = np.nan  # one query all NaN inside the group of 8
    ix = FlatL2Index.from_array(corpus, dtype=dtype, l2_small_batch=True)
    try:
        dist = ref_dists(corpus, dtype, query_seen(q, False, dtype))
        with np.errstate(invalid="ignore"):
            assert not (dist[:, list(bad)] < FMAX).any() and not (dist[5] < FMAX).any()
        for k in (3, n, n + 11):
            c38 = ix.debug_counter(38)
            D, I = ix.search(q, k)
            assert ix.debug_counter(38) > c38
            same((D, I), topk_l2(dist, k), f"k={k}")
            ix.set_l2_small_batch(False)
            same((D, I), ix.search(q, k), f"k={k} against the switch off")
            ix.set_l2_small_batch(True)
            assert not np.isin(I, list(bad)).any()
            # an exact match: +0.0, rank 0, duplicates in row order
            assert I[0, :3].tolist() == [5, 17, 200] and (D[0, :3] == 0).all() and not np.signbit(D[0, :3]).any()
            assert I[1, 0] == 100 and D[1, 0] == 0 and not np.signbit(D[1, 0])
            assert (I[5] == -1).all() and (D[5] == FMAX).all()  # the NaN query finds nothing, the other seven everything
            valid = n - len(bad)
            others = [i for i in range(8) if i != 5]
            assert (I[others][:, :min(k, valid)] >= 0).all()
            assert (I[:, valid:] == -1).all() and (D[:, valid:] == FMAX).all()  # (k > n: padding)
    finally:
        ix.close()
    # k > n with n = 37, and a base
    small = np.ascontiguousarray(H.gauss(42, 37, d))
    ix = FlatL2Index.from_array(small, dtype=dtype, base=1000, l2_small_batch=True)
    try:
        good = np.ascontiguousarray(q[[0, 1, 2, 3, 4]])
        D, I = ix.search(good, 50)
        same((D, I), topk_l2(ref_dists(small, dtype, query_seen(good, False, dtype)), 50, base=1000), "n = 37")
        assert (I[:, :37] >= 1000).all() and (I[:, 37:] == -1).all() and (D[:, 37:] == FMAX).all()
    finally:
        ix.close()
    ix = FlatL2Index(d, dtype=dtype, l2_small_batch=True)  # n = 0
    D, I = ix.search(q, 4)
    assert (I == -1).all() and (D == FMAX).all() and ix.ntotal == 0
    ix.close()


def test_fp16_subnormals_and_values_that_round_on_a_tie():
    """fp16 rows and queries of subnormals (multiples of 2^-24 below 2^-14), of values halfway between two fp16 numbers
    (round to even on the way in) and of products q * inv that land on such a tie: a flushed subnormal, a second
    rounding or a mixed-precision subtraction would move a distance."""
    d, n = 100, 500
    rng = np.random.default_rng(77)
    sub = np.float32(2.0 ** -24)
    corpus = (rng.integers(-1023, 1024, size=(n, d)).astype(np.float32) * sub)  # every element an fp16 subnormal (or 0)
    ties = (rng.integers(1024, 2048, size=(n // 2, d)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -10)
    corpus[n // 2:] = ties  # 1 + (m + 1/2) 2^-10: halfway between two fp16 numbers of [1, 2)
    corpus[3] = corpus[2]
    q = np.empty((8, d), np.float32)
    q[:3] = rng.integers(-1023, 1024, size=(3, d)).astype(np.float32) * sub
    q[3] = corpus[2]
    q[4:7] = (rng.integers(1024, 2048, size=(3, d)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -10)
    q[7] = corpus[n - 1]
    assert (np.abs(corpus[:n // 2].astype(np.float16).astype(np.float32)) < 2.0 ** -14).all()
    assert (corpus[n // 2:].astype(np.float16).astype(np.float32) != corpus[n // 2:]).all()
    ix = FlatL2Index.from_array(corpus, dtype="f16", l2_small_batch=True)
    try:
        for normalize in (False, True):
            dist = ref_dists(corpus, "f16", query_seen(q, normalize, "f16"))
            if not normalize:
                assert dist[3, 2] == 0 and dist[3, 3] == 0 and dist[7, n - 1] == 0
                assert 0 < dist[0, :n // 2].min() < 2.0 ** -20  # (sums of squared differences of subnormals)
            for k in (1, 10, n):
                c38 = ix.debug_counter(38)
                got = ix.search(q, k, normalize=normalize)
                assert ix.debug_counter(38) > c38
                same(got, topk_l2(dist, k), f"k={k} normalize={normalize}")
                ix.set_l2_small_batch(False)
                same(got, ix.search(q, k, normalize=normalize), f"k={k} normalize={normalize} against the switch off")
                ix.set_l2_small_batch(True)
                for nq in (2, 5):
                    D, I = ix.search(q[:nq], k, normalize=normalize)
                    assert np.array_equal(D, got[0][:nq]) and np.array_equal(I, got[1][:nq])
    finally:
        ix.close()


# ---- 4: forced retries -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, d", [("f32", 384), ("f16", 383)])
def test_forced_retry_is_served_by_the_single_query_scan(dtype, d):
    """k = 2048 at n = 3001 with debug option 7 = 4: four workgroups emit at most 60 keys per query, the selection cannot
    prove 2048 results from them, and the host serves every query of the group again, alone (counter 25)."""
    corpus, q = H.gauss(400 + d, N, d), H.gauss(401 + d, 13, d)
    ix = FlatL2Index.from_array(corpus, dtype=dtype)
    try:
        k = 2048
        want = topk_l2(ref_dists(corpus, dtype, query_seen(q, True, dtype)), k)
        plain = ix.search(q, k, normalize=True)
        same(plain, want, "switch off")
        ix.set_l2_small_batch(True)
        for opt in (4, 256, 0):
            ix.debug_option(7, opt)
            c25, c38 = ix.debug_counter(25), ix.debug_counter(38)
            got = ix.search(q, k, normalize=True)
            assert ix.debug_counter(38) - c38 == 2  # 13 = 8 + 5 (the queries served again go out alone: not counted)
            if opt == 4:
                assert ix.debug_counter(25) - c25 == 13, "every query of the call is served again"
            same(got, plain, f"option 7 = {opt}")
            same(ix.search(q, 10, normalize=True), (want[0][:, :10], want[1][:, :10]), f"k = 10, option 7 = {opt}")
    finally:
        ix.debug_option(7, 0)
        ix.close()


# ---- 5: concurrent callers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_concurrent_callers(dtype):
    n, d, k = 5000, 384, 10
    corpus = H.gauss(70, n, d)
    q = H.gauss(71, 160, d)
    ix = FlatL2Index.from_array(corpus, dtype=dtype, l2_small_batch=True)
    try:
        serial = [ix.search(q[i:i + 1], k) for i in range(160)]
        assert ix.debug_counter(38) == 0
        same(ix.search(q[:16], k), topk_l2(ref_dists(corpus, dtype, query_seen(q[:16], False, dtype)), k), "a 16-query call")
        D40, I40 = ix.search(q[:40], k)  # (more than one combined call carries)
        for i in range(40):
            assert np.array_equal(D40[i], serial[i][0][0]) and np.array_equal(I40[i], serial[i][1][0])
        out, errors = [None] * 160, []
        c16, c38 = ix.debug_counter(16), ix.debug_counter(38)

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
        # (whether the callers overlapped is the scheduler's business; where they did, their batch went out as groups)
        batches, launches = ix.debug_counter(16) - c16, ix.debug_counter(38) - c38
        assert batches >= 0 and (launches > 0) == (batches > 0), (batches, launches)
        assert ix.debug_counter(23) == 0 and ix.debug_counter(34) == 0 and ix.debug_counter(36) == 0
    finally:
        ix.close()


# ---- 6: mutation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, d", [("f32", 384), ("f16", 385)])
def test_add_then_remove_then_an_11_query_search(dtype, d):
    rng = np.random.default_rng(60 + d)
    first, more = H.gauss(61 + d, N, d), H.gauss(62 + d, 200, d)
    q = H.gauss(64 + d, 11, d)
    ix = FlatL2Index.from_array(first, dtype=dtype, l2_small_batch=True)
    try:
        ix.search(q, 5)
        ix.add(more)
        everything = np.concatenate([first, more])
        gone = rng.random(everything.shape[0]) < 0.10
        assert ix.remove_ids(gone) == int(gone.sum()) and ix.l2_small_batch is True
        assert native.load().ls_l2_small_batch(ix._handle) == 1
        survivors = everything[~gone]
        fresh = FlatL2Index.from_array(survivors, dtype=dtype)
        try:
            for normalize in (False, True):
                dist = ref_dists(survivors, dtype, query_seen(q, normalize, dtype))
                for k in (10, 2048):
                    c38 = ix.debug_counter(38)
                    got = ix.search(q, k, normalize=normalize)
                    assert ix.debug_counter(38) - c38 >= 2  # 11 = 8 + 3
                    same(got, fresh.search(q, k, normalize=normalize), f"against a fresh index k={k}")
                    same(got, topk_l2(dist, k), f"against the reference k={k}")
            assert fresh.debug_counter(38) == 0
        finally:
            fresh.close()
    finally:
        ix.close()


# ---- 7: the handles beside it ------------------------------------------------------------------------------------------
def test_inner_product_and_ivf_l2_handles_beside_it_are_unchanged():
    d, k = 384, 10
    corpus, q = H.gauss(80, N, d), H.gauss(81, 13, d)
    ip = FlatIPIndex.from_array(corpus, dtype="f16")
    ivf = IVFFlatIndex(d, 16, metric="l2")
    ivf.set_centroids(corpus[:16])
    ivf.add(corpus)
    ivf.nprobe = 5
    l2 = FlatL2Index.from_array(corpus)
    try:
        before_ip, before_ivf = ip.search(q, k), ivf.search(q, k)
        before_l2 = l2.search(q, k)
        l2.set_l2_small_batch(True)
        same(l2.search(q, k), before_l2, "the L2 handle itself")
        assert l2.debug_counter(38) == 2
        same(ip.search(q, k), before_ip, "the inner-product handle")
        same(ivf.search(q, k), before_ivf, "the IVF L2 handle")
        lib = native.load()
        assert lib.ls_set_l2_small_batch(ip._handle, 1) == native.LS_ERR_INVALID_ARG and b"L2" in lib.ls_last_error()
        assert lib.ls_l2_small_batch(ip._handle) == 0 and ip.debug_counter(38) == 0
        with pytest.raises(ValueError):
            ip.set_l2_small_batch(True)
        with pytest.raises(ValueError):
            ivf.set_small_batch(True)  # (the IVF index keeps refusing its own small batches under L2)
        same(ip.search(q, k), before_ip, "the inner-product handle after the refusal")
        l2.set_l2_small_batch(False)
        same(l2.search(q, k), before_l2, "the L2 handle, switched off again")
        assert l2.debug_counter(38) == 2
    finally:
        ip.close()
        ivf.close()
        l2.close()


# ---- 8: faiss_compat ---------------------------------------------------------------------------------------------------
def test_faiss_compat_index_flat_l2_with_the_switch(tmp_path):
    d = 100
    corpus, q = H.gauss(90, 800, d, normalize=False), H.gauss(91, 13, d, normalize=False)
    ix = faiss_compat.IndexFlatL2(d, l2_small_batch=True)
    ix.add(corpus)
    want = topk_l2(ref_dists(corpus, "f32", q), 10)
    same(ix.search(q, 10), want, "a 13-query search")
    assert ix.debug_counter(38) == 2 and ix.l2_small_batch is True
    p = tmp_path / "l2.index"
    faiss_compat.write_index(ix, p)
    assert p.read_bytes()[:4] == b"IxF2"
    back = faiss_compat.read_index(p, l2_small_batch=True)
    assert isinstance(back, faiss_compat.IndexFlatL2) and back.ntotal == 800 and back.l2_small_batch is True
    same(back.search(q, 10), want, "after write_index / read_index")
    assert back.debug_counter(38) == 2
    plain = faiss_compat.read_index(p)
    same(plain.search(q, 10), want, "read without the keyword")
    assert plain.debug_counter(38) == 0 and plain.l2_small_batch is False
    flat = faiss_compat.IndexFlat(d, faiss_compat.METRIC_L2, l2_small_batch=True)
    flat.add(corpus)
    same(flat.search(q, 10), want, "IndexFlat(d, METRIC_L2, l2_small_batch=True)")
    assert flat.debug_counter(38) == 2
    for x in (ix, back, plain, flat):
        x.close()
