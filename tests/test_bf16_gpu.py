"""The bf16 storage dtype on the MI355X (include/leansearch_bf16.h). Every comparison is np.array_equal
on scores and indices against a host-only reference: tests/bf16_ref.c on lean_explore_amd/bf16.py's encoding of the rows
(int64 arithmetic for the integer-valued cases), ranked by the library's order on the host. The shapes are those of
tests/test_geometry_cpu.py: n = 3001 rows, where debug option 7 = 4 forces the non-SMALL variant of the scan and 256 the
SMALL one for every geometry."""

import ctypes

import numpy as np
import pytest

from lean_explore_amd import bf16, faiss_compat, loader, native
from lean_explore_amd import search as S
from lean_explore_amd.id_selectors import SearchParameters, SearchParametersIVF
from lean_explore_amd.index import FlatIPIndex
from lean_explore_amd.ivf import IVFFlatIndex
from oracle import oracle
from tests import helpers as H
from tests.test_bf16_cpu import ENCODE_TABLE, REF_DIMS, SWITCH_RULES, ref_of
from tests.test_geometry_cpu import (GEOMS, N, NQ, PLAIN_K, PLAIN_OPTS, SUBSET_K, SUBSET_RUNS, default_blocks, geom_of,
                                     is_small, ivf_dims, seen_queries, selections, uneven_assignment)
from tests.test_glue_cpu import FakeEmbed, _make_db, run
from tests.test_ivf_gpu import mixture
from tests.test_sq8_cpu import NEG, exact_topk

pytestmark = pytest.mark.gpu

NLIST = 37


def make_data(d, kind, n=N):
    """(corpus, [(queries, normalize)]), as tests/test_geometry_gpu.py makes them: integer-valued data (|values| <= 64:
    exact in bf16 and in any summation order) runs without normalisation only; Gaussian rows are unit norm, queries 0, 1
    are rescaled and run with normalize=True."""
    seed = 9000 + 3 * d
    if kind == "int":
        return H.int_corpus(seed, n, d, -64, 65), [(H.int_corpus(seed + 1, NQ, d, -64, 65), False)]
    q = H.gauss(seed + 1, NQ, d)
    q[:2] *= np.float32(2.5)
    return H.gauss(seed, n, d), [(np.ascontiguousarray(q[:2]), True), (np.ascontiguousarray(q[2:]), False)]


def scores_of(corpus, qn, kind):
    """The reference scores [nq, n] of the queries as the kernels see them."""
    if kind == "int":
        s = qn.astype(np.int64) @ corpus.astype(np.int64).T
        assert np.abs(s).max() < 2 ** 24
        return s.astype(np.float32)
    return ref_of(corpus, qn)


def topk_of(scores, rows, k):
    out = [exact_topk(s[rows], k, rows) for s in scores]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def assert_same(got, want, what):
    assert np.array_equal(got[1], want[1]), f"{what}: rows differ"
    assert np.array_equal(got[0], want[0]), f"{what}: scores differ"


def search_both_ways(search, q):
    """One call of all the queries, then query by query: the same bits."""
    D, I = search(q)
    for i in range(q.shape[0]):
        D1, I1 = search(q[i:i + 1])
        assert np.array_equal(I1[0], I[i]) and np.array_equal(D1[0], D[i]), f"query {i} alone differs from the call"
    return D, I


def test_the_cases_cover_every_geometry():
    assert {geom_of("f16", d) for d in REF_DIMS} == set(GEOMS["f16"])
    assert {geom_of("f16", d) for d in ivf_dims("f16")} == {g for g in GEOMS["f16"] if g[0] < 64}


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gauss", "int"])
@pytest.mark.parametrize("d", REF_DIMS)
def test_plain_and_subset_search(d, kind):
    L, V = geom_of("f16", d)
    corpus, groups = make_data(d, kind)
    ix = FlatIPIndex.from_array(corpus, dtype="bf16")
    sel = selections()
    subs = {name: ix.subset(rows) for name, rows in sel.items()}
    everything = sel["ones"]
    try:
        assert [s.rows for s in subs.values()] == [r.size for r in sel.values()]
        assert ix.bf16_inexact == bf16.inexact(corpus) and (kind != "int" or ix.bf16_inexact == 0)
        for q, normalize in groups:
            Sr = scores_of(corpus, seen_queries(q, normalize), kind)
            plain = {}
            for k in PLAIN_K:
                for opt in PLAIN_OPTS:
                    blocks = opt or default_blocks(N, L, V)
                    assert opt == 0 or is_small(N, blocks, L, V) == (opt == 256)
                    ix.debug_option(7, opt)
                    got = search_both_ways(lambda x: ix.search(x, k, normalize=normalize), q)
                    if opt == 0:
                        assert_same(got, topk_of(Sr, everything, k), f"plain k={k}")
                        plain[k] = got
                    else:  # the other variant: the same bits
                        assert_same(got, plain[k], f"plain k={k} option 7 = {opt}")
            for k in SUBSET_K:
                first = {}
                for name, opt in SUBSET_RUNS:
                    m = sel[name].size
                    small = is_small(m, opt or default_blocks(m, L, V), L, V)
                    assert {("mask10", 1): not small, ("mask10", 256): small, ("forty", 0): small,
                            ("ones", 4): not small}.get((name, opt), True)
                    ix.debug_option(7, opt)
                    got = ix.search(q, k, normalize=normalize, params=SearchParameters(sel=subs[name]))
                    if name not in first:
                        assert_same(got, topk_of(Sr, sel[name], k), f"subset {name} k={k}")
                        D, I = got
                        assert (I[:, m:] == -1).all() and (D[:, m:] == NEG).all() and (I[:, :min(k, m)] >= 0).all()
                        first[name] = got
                    else:
                        assert_same(got, first[name], f"subset {name} k={k} option 7 = {opt}")
                if k in plain:  # the all-ones mask is the plain search
                    assert_same(first["ones"], plain[k], f"all-ones subset k={k}")
            ix.debug_option(7, 0)
            assert_same(ix.search(q, 50, normalize=normalize, params=SearchParameters(sel=subs["ones"])),
                        ix.search(q, 50, normalize=normalize), "all-ones subset k=50")
    finally:
        ix.debug_option(7, 0)
        for s in subs.values():
            s.close()
        ix.close()


def test_a_call_of_many_queries_is_served_query_by_query():
    """40 queries over 40 000 rows: on an fp16 index this shape goes to the batched matrix-core path, on a bf16 index -
    as on an sq8 one - every query goes out alone on the scan kernel (launch counter), host and device calls alike."""
    n, d, nq, k = 40_000, 128, 40, 10
    corpus, q = H.gauss(41, n, d), H.gauss(42, nq, d)
    want = topk_of(ref_of(corpus, q), np.arange(n), k)
    ix = FlatIPIndex.from_array(corpus, dtype="bf16")
    try:
        before = ix.debug_counter(23)
        assert_same(ix.search(q, k), want, "host call")
        assert ix.debug_counter(23) == before, "a bf16 index must never launch a small-batch pass"
        import torch

        tq = torch.from_numpy(q).cuda()
        for kw in ({}, {"asynchronous": True}, {"pipeline": True}):
            Dt, It = ix.search_device(tq, k, **kw)
            ix.check()
            assert_same((Dt.cpu().numpy(), It.cpu().numpy()), want, f"device call {kw}")
    finally:
        ix.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------
def special_rows(d):
    u = np.array([a for a, _ in ENCODE_TABLE], np.uint32)
    rows = np.resize(u, (3, d)).view(np.float32).copy()  # the table's bit patterns, over and over
    return rows


@pytest.mark.parametrize("d", [250, 384])
def test_stored_bits_reconstruct_and_the_inexact_count(d, tmp_path):
    corpus = np.concatenate([special_rows(d), H.gauss(7, N - 3, d)])
    ix = FlatIPIndex.from_array(corpus, dtype="bf16")
    try:
        bits = ix.bf16_rows()
        assert bits.dtype == np.uint16 and np.array_equal(bits, bf16.encode(corpus))
        assert np.array_equal(ix.bf16_rows(1, 2), bits[1:3]) and ix.bf16_rows(N, 0).shape == (0, d)
        assert np.array_equal(ix.reconstruct_n(0, N).view(np.uint32), bf16.decode(bits).view(np.uint32))
        assert np.array_equal(ix.host_corpus().view(np.uint32), bf16.decode(bits).view(np.uint32))
        assert ix.bf16_inexact == bf16.inexact(corpus) > 0
        with pytest.raises(ValueError, match="allow_lossy"):
            faiss_compat.write_index(ix, tmp_path / "lossy.index")
    finally:
        ix.close()
    # a corpus that is already bf16-valued: nothing is lost, the file holds exactly what was added
    exact = bf16.decode(bf16.encode(H.gauss(8, N, d)))
    q = H.gauss(9, NQ, d)
    ix = FlatIPIndex.from_array(exact, dtype="bf16")
    try:
        assert ix.bf16_inexact == 0 and np.array_equal(ix.reconstruct_n(0, N), exact)
        faiss_compat.write_index(ix, tmp_path / "exact.index")
        assert np.array_equal(faiss_compat.read_index(tmp_path / "exact.index").host_corpus(), exact)
        back = faiss_compat.read_index(tmp_path / "exact.index", dtype="bf16")
        assert back.storage_dtype == "bf16"
        assert_same(back.search(q, 50, normalize=True), ix.search(q, 50, normalize=True), "read_index(dtype='bf16')")
        assert back.bf16_inexact == 0
        back.close()
    finally:
        ix.close()


def test_ivf_write_index_needs_allow_lossy_only_when_values_were_rounded(tmp_path):
    d, n = 100, 600
    rows = H.gauss(11, n, d)
    cent = H.gauss(12, NLIST, d)
    assign = uneven_assignment(n, NLIST)
    q = H.gauss(13, NQ, d)
    for corpus, lossless in ((rows, False), (bf16.decode(bf16.encode(rows)), True)):
        ivf = IVFFlatIndex(d, NLIST, dtype="bf16")
        ivf.set_centroids(cent)
        ivf.add(corpus, assign=assign)
        ivf.nprobe = 5
        try:
            assert ivf.bf16_inexact == bf16.inexact(corpus) and (ivf.bf16_inexact == 0) == lossless
            assert np.array_equal(ivf.reconstruct_n(0, n), bf16.decode(bf16.encode(corpus)))
            if not lossless:
                with pytest.raises(ValueError, match="allow_lossy"):
                    faiss_compat.write_index(ivf, tmp_path / "ivf.index")
                continue
            faiss_compat.write_index(ivf, tmp_path / "ivf.index")
            back = faiss_compat.read_index(tmp_path / "ivf.index", dtype="bf16", ivf=True)
            assert back.storage_dtype == "bf16" and back.nprobe == 5
            assert_same(back.search(q, 20), ivf.search(q, 20), "IwFl round trip")
            back.close()
        finally:
            ivf.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def probed_rows(cent, assign, qn, nprobe):
    """The rows of the lists every query probes: the top min(nprobe, nlist) centroids under the f32 scan order (the
    centroids are an f32 index whatever the rows' dtype), as tests/test_geometry_cpu.py::ivf_reference computes them."""
    _, P = oracle.c_search(cent, qn, min(nprobe, cent.shape[0]), order="scan")
    return [np.flatnonzero(np.isin(assign, P[i][P[i] >= 0])) for i in range(qn.shape[0])]


def ivf_want(Sr, rows_of, k):
    out = [exact_topk(Sr[i][rows], k, rows) if rows.size else (np.full(k, NEG, np.float32), np.full(k, -1, np.int64))
           for i, rows in enumerate(rows_of)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@pytest.mark.parametrize("d", ivf_dims("f16"))
def test_ivf_search_subset_and_second_launch(d):
    corpus, groups = make_data(d, "gauss")
    assign = uneven_assignment()
    sizes = np.bincount(assign, minlength=NLIST)
    cent = H.gauss(90 + d, NLIST, d)
    mask = selections()["mask10"]
    ivf = IVFFlatIndex(d, NLIST, dtype="bf16")
    ivf.set_centroids(cent)
    ivf.add(corpus, assign=assign)
    sub = ivf.subset(mask)
    try:
        assert np.array_equal(ivf.list_sizes(), sizes) and sub.rows == mask.size
        for q, normalize in groups:
            nq = q.shape[0]
            qn = seen_queries(q, normalize)
            Sr = ref_of(corpus, qn)
            for nprobe in (1, 5, NLIST):
                rows_of = probed_rows(cent, assign, qn, nprobe)
                for k in (10, 1500):
                    got = search_both_ways(
                        lambda x: ivf.search(x, k, normalize=normalize, params=SearchParametersIVF(nprobe=nprobe)), q)
                    assert_same(got, ivf_want(Sr, rows_of, k), f"nprobe {nprobe} k {k}")
                    if nprobe == NLIST and k == 1500:
                        # all 3001 rows probed: at most 47 workgroups emit at most 15 keys each, which cannot prove
                        # 1500 ranks - every query is served by the second launch
                        ivf.search(q, k, normalize=normalize, params=SearchParametersIVF(nprobe=nprobe))
                        assert ivf.last_kernel_ms()[2] == nq
                got = ivf.search(q, 50, normalize=normalize, params=SearchParametersIVF(sel=sub, nprobe=nprobe))
                assert_same(got, ivf_want(Sr, [np.intersect1d(r, mask) for r in rows_of], 50), f"IVFSubset nprobe {nprobe}")
    finally:
        sub.close()
        ivf.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def range_want(Sr, rows_of, radius):
    lims, D, I = [0], [], []
    for i, rows in enumerate(rows_of):
        hit = rows[Sr[i][rows] > radius]  # (ascending rows; NaN never passes)
        lims.append(lims[-1] + hit.size)
        D.append(Sr[i][hit])
        I.append(hit)
    return np.array(lims, np.uint64), np.concatenate(D).astype(np.float32), np.concatenate(I).astype(np.int64)


@pytest.mark.parametrize("d", [384, 1001])
def test_range_search_flat_and_ivf(d):
    corpus, _ = make_data(d, "gauss")
    q = H.gauss(55 + d, NQ, d) * np.float32(1.7)
    qn = seen_queries(q, True)
    Sr = ref_of(corpus, qn)
    radius = float(np.float32(1.0 / np.sqrt(d)))  # about one standard deviation of a score: a sixth of the rows
    mask = selections()["mask10"]
    ix = FlatIPIndex.from_array(corpus, dtype="bf16")
    try:
        for rows, params in ((np.arange(N), None), (mask, SearchParameters(sel=mask))):
            got = ix.range_search(q, radius, normalize=True, params=params)
            want = range_want(Sr, [rows] * NQ, radius)
            assert 0 < want[0][-1] < NQ * rows.size
            for g, w, what in zip(got, want, ("lims", "D", "I")):
                assert np.array_equal(g, w), what
    finally:
        ix.close()
    assign = uneven_assignment()
    cent = H.gauss(90 + d, NLIST, d)
    ivf = IVFFlatIndex(d, NLIST, dtype="bf16")
    ivf.set_centroids(cent)
    ivf.add(corpus, assign=assign)
    try:
        for nprobe in (5, NLIST):
            got = ivf.range_search(q, radius, normalize=True, params=SearchParametersIVF(nprobe=nprobe))
            want = range_want(Sr, probed_rows(cent, assign, qn, nprobe), radius)
            for g, w, what in zip(got, want, ("lims", "D", "I")):
                assert np.array_equal(g, w), (nprobe, what)
    finally:
        ivf.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def mutation_plan(d):
    corpus, _ = make_data(d, "gauss")
    rng = np.random.default_rng(5)
    first, second, third = corpus[:2000], corpus[2000:2600], corpus[2600:]
    gone = np.sort(rng.choice(2600, 700, replace=False))  # rows of the first two adds, of every tile and list
    keep = np.setdiff1d(np.arange(2600), gone)
    final = np.concatenate([corpus[:2600][keep], third])
    return corpus, first, second, third, gone, keep, final


@pytest.mark.parametrize("d", [250, 768])
def test_flat_add_remove_add(d):
    corpus, first, second, third, gone, keep, final = mutation_plan(d)
    q = H.gauss(61, NQ, d)
    ix = FlatIPIndex.from_array(first, dtype="bf16")
    fresh = None
    try:
        ix.search(q, 10)  # (the handle has served a search before it grows)
        sub = ix.subset(np.arange(0, 2000, 3))
        ix.add(second)
        assert ix.remove_ids(gone) == gone.size
        ix.add(third)
        assert ix.ntotal == final.shape[0]
        fresh = FlatIPIndex.from_array(final, dtype="bf16")
        assert np.array_equal(ix.bf16_rows(), fresh.bf16_rows()) and np.array_equal(ix.bf16_rows(), bf16.encode(final))
        assert np.array_equal(ix.reconstruct_n(), bf16.decode(bf16.encode(final)))
        for k in (10, 2048):
            assert_same(ix.search(q, k, normalize=True), fresh.search(q, k, normalize=True), f"k={k}")
        assert_same(ix.search(q, 50), topk_of(ref_of(final, q), np.arange(final.shape[0]), 50), "against bf16_ref.c")
        # the subset shrank to its survivors, under their new numbers
        survivors = np.flatnonzero(np.isin(keep, np.arange(0, 2000, 3)))
        assert sub.rows == survivors.size
        assert_same(ix.search(q, 50, params=SearchParameters(sel=sub)), topk_of(ref_of(final, q), survivors, 50), "subset")
        # every row ever handed in counts, removed or not
        assert ix.bf16_inexact == bf16.inexact(corpus) and fresh.bf16_inexact == bf16.inexact(final)
        sub.close()
    finally:
        ix.close()
        if fresh is not None:
            fresh.close()


@pytest.mark.parametrize("d", [250, 768])
def test_ivf_add_remove_add(d):
    corpus, first, second, third, gone, keep, final = mutation_plan(d)
    assign = uneven_assignment()
    final_assign = np.concatenate([assign[:2600][keep], assign[2600:]])
    cent = H.gauss(90 + d, NLIST, d)
    q = H.gauss(62, NQ, d)
    ivf = IVFFlatIndex(d, NLIST, dtype="bf16")
    ivf.set_centroids(cent)
    ivf.add(first, assign=assign[:2000])
    fresh = IVFFlatIndex(d, NLIST, dtype="bf16")
    fresh.set_centroids(cent)
    fresh.add(final, assign=final_assign)
    try:
        ivf.search(q, 10)
        sub = ivf.subset(np.arange(0, 2000, 3))
        ivf.add(second, assign=assign[2000:2600])
        assert ivf.remove_ids(gone) == gone.size
        ivf.add(third, assign=assign[2600:])
        assert ivf.ntotal == final.shape[0] and np.array_equal(ivf.assignment(), final_assign)
        assert np.array_equal(ivf.reconstruct_n(), bf16.decode(bf16.encode(final)))
        Sr = ref_of(final, q)
        for nprobe in (5, NLIST):
            p = SearchParametersIVF(nprobe=nprobe)
            rows_of = probed_rows(cent, final_assign, q, nprobe)
            for k in (10, 1500):
                got = ivf.search(q, k, params=p)
                assert_same(got, fresh.search(q, k, params=p), f"nprobe {nprobe} k={k}")
                assert_same(got, ivf_want(Sr, rows_of, k), f"nprobe {nprobe} k={k} against bf16_ref.c")
        survivors = np.flatnonzero(np.isin(keep, np.arange(0, 2000, 3)))
        assert sub.rows == survivors.size
        got = ivf.search(q, 50, params=SearchParametersIVF(sel=sub, nprobe=NLIST))
        assert_same(got, topk_of(Sr, survivors, 50), "IVFSubset")
        assert ivf.bf16_inexact == bf16.inexact(corpus) and fresh.bf16_inexact == bf16.inexact(final)
        sub.close()
    finally:
        ivf.close()
        fresh.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [384, 1024])
def test_against_the_f32_index_of_the_same_values(d):
    """The claim a user cares about: the bf16 index and the f32 index of the decoded rows differ in summation order only.
    Scores within 1e-5; an index may differ only where the float64 scores lie within 2e-6."""
    k = 50
    corpus, _ = make_data(d, "gauss")
    q = H.gauss(71 + d, 16, d)
    dec = bf16.decode(bf16.encode(corpus))
    b = FlatIPIndex.from_array(corpus, dtype="bf16")
    f = FlatIPIndex.from_array(dec, dtype="f32")
    try:
        Db, Ib = b.search(q, k)
        Df, If = f.search(q, k)
        S64 = q.astype(np.float64) @ dec.astype(np.float64).T
        print(f"d={d}: max |D_bf16 - D_f32| = {np.abs(Db - Df).max():.3e}, rows that differ: {(Ib != If).sum()}")
        assert np.abs(Db - Df).max() <= 1e-5
        assert np.abs(Db - np.take_along_axis(S64, Ib, axis=1)).max() <= 1e-5
        for i, j in zip(*np.nonzero(Ib != If)):
            assert abs(S64[i, Ib[i, j]] - S64[i, If[i, j]]) <= 2e-6, (i, j)
    finally:
        b.close()
        f.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_switches_refuse_on_a_live_handle():
    lib = native.load()
    x = H.gauss(1, 64, 8)
    ix = FlatIPIndex.from_array(x, dtype="bf16")
    ivf = IVFFlatIndex(8, 4, dtype="bf16")
    ivf.set_centroids(x[:4])
    ivf.add(x)
    ivf.search(x[:1], 3)
    setters = {"LS_SW_F16": (lib.ls_set_f16_small_batch, ix._handle), "LS_SW_SQ8": (lib.ls_set_sq8_small_batch, ix._handle),
               "LS_SW_SUBSET": (lib.ls_set_subset_small_batch, ix._handle), "LS_SW_L2": (lib.ls_set_l2_small_batch, ix._handle),
               "LS_SW_IVF": (lib.ls_ivf_set_small_batch, ivf._handle)}
    try:
        for sw, enable, words in SWITCH_RULES:
            fn, h = setters[sw]
            rc = fn(h, enable)
            if words is None:
                assert rc == native.LS_OK, (sw, enable, lib.ls_last_error())
            else:
                assert rc == native.LS_ERR_INVALID_ARG and lib.ls_last_error().decode().startswith(words), (sw, enable)
        out = np.empty(8, np.float32)
        assert lib.ls_sq8_step(ix._handle, out.ctypes.data) == native.LS_ERR_INVALID_ARG  # not an sq8 handle
        f32 = FlatIPIndex.from_array(x, dtype="f32")
        n = ctypes.c_int64()
        assert lib.ls_bf16_inexact(f32._handle, ctypes.byref(n)) == native.LS_ERR_INVALID_ARG  # not a bf16 handle
        assert b"bf16" in lib.ls_last_error()
        f32.close()
        ids = (ctypes.c_int32 * 2)(0, 0)
        h = ctypes.c_void_p()
        for fn in (lib.ls_create_sharded, lib.ls_create_replicated):
            assert fn(ctypes.byref(h), x.ctypes.data, 64, 8, native.LS_DTYPE_BF16, ids, 2) == native.LS_ERR_INVALID_ARG
        assert lib.ls_create_l2(ctypes.byref(h), x.ctypes.data, 64, 8, native.LS_DTYPE_BF16, 0) == native.LS_ERR_INVALID_ARG
    finally:
        ix.close()
        ivf.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semantic_index", ["flat", "ivf"])
def test_search_engine_storage_dtype_bf16(tmp_path, semantic_index):
    """The synthetic corpus of tests/test_sq8_gpu.py's engine test, made bf16-valued (what a bf16 embedder emits): the
    bf16 engine returns the ids the f32 engine returns."""
    n, d = 2_000, 96
    corpus, cent = mixture(71, n, d, 16)
    corpus = bf16.decode(bf16.encode(corpus))
    rows = [(5000 + i, f"Mathlib.decl{i}", "Mathlib.Mod", "doc", f"theorem t{i}", f"http://x/{i}", None,
             f"statement {i}", loader.embedding_to_blob(corpus[i].tolist())) for i in range(n)]
    db = tmp_path / "lean_explore.db"
    _make_db(db, rows)
    ids, loaded = loader.load_corpus_from_sqlite(db)
    assert np.array_equal(loaded, corpus)
    loader.save_ids_map(tmp_path / "informalization_faiss_ids_map.json", ids)
    if semantic_index == "ivf":
        src = IVFFlatIndex(d, 16)
        src.set_centroids(cent)
        src.add(loaded)
        src.nprobe = 16
    else:
        src = FlatIPIndex.from_array(loaded)
    faiss_compat.write_index(src, tmp_path / "informalization_faiss.index")
    src.close()
    qvec = corpus[123] * 3.0
    sems = {}
    for dtype in ("f32", "bf16"):
        eng = S.SearchEngine(base_path=tmp_path, embedding_client=FakeEmbed(qvec), lexical_retriever=False,
                             storage_dtype=dtype, semantic_index=semantic_index)
        sems[dtype] = run(eng._retrieve_semantic_candidates("q", 50))
        assert eng.faiss_informal_index.storage_dtype == dtype
    assert list(sems["bf16"]) == list(sems["f32"]) and list(sems["bf16"])[0] == 5123
    assert np.abs(np.array(list(sems["bf16"].values())) - np.array(list(sems["f32"].values()))).max() <= 1e-5
