"""Exact search over a row subset on the MI355X (ls_subset_create / ls_search_subset): the answer is the plain search
of an index that holds only the selected rows, with every score bit-identical to the unfiltered scan's."""

import threading
import time

import numpy as np
import pytest

from lean_explore_amd import faiss_compat as fc
from lean_explore_amd import native
from lean_explore_amd.index import FlatIPIndex
from oracle import oracle
from tests import helpers as H

pytestmark = pytest.mark.gpu


def sub_search(ix, q, k, sel, normalize=False):
    return ix.search(q, k, normalize=normalize, params=fc.SearchParameters(sel=sel))


def expect(corpus, rows, q, k, normalize=False, f16=False):
    """Oracle over corpus[rows] in the scan kernel's summation order, indices mapped through rows."""
    qq = oracle.c_normalize_l2(q) if normalize else q
    if f16:
        D, I = oracle.c_search(corpus[rows], qq, k, f16=True)
    else:
        D, I = oracle.c_search(corpus[rows], qq, k, order="scan")
    return D, np.where(I >= 0, rows[np.maximum(I, 0)], -1)


@pytest.mark.parametrize("n,d,k,dtype", [(200_000, 384, 50, "f32"), (200_000, 1024, 1000, "f32"),
                                         (200_000, 384, 100, "f16")])
def test_all_ones_subset_equals_plain_search(n, d, k, dtype):
    corpus = H.gauss(3, n, d)
    q = H.gauss(4, 3, d, normalize=False)
    ix = FlatIPIndex.from_array(corpus, dtype=dtype)
    sub = ix.subset(np.ones(n, bool))
    assert sub.rows == n
    for normalize in (False, True):
        for i in range(q.shape[0]):
            D0, I0 = ix.search(q[i:i + 1], k, normalize=normalize)
            D1, I1 = sub_search(ix, q[i:i + 1], k, sub, normalize)
            assert np.array_equal(D0, D1) and np.array_equal(I0, I1)
    sub.close()
    ix.close()


@pytest.mark.parametrize("d", [100, 384, 768, 1024])
def test_random_subsets_match_the_oracle_exactly(d):
    n = 30_000
    corpus = H.gauss(10 + d, n, d)
    q = H.gauss(20 + d, 2, d, normalize=False)
    ix = FlatIPIndex.from_array(corpus)
    rng = np.random.default_rng(d)
    for frac in (0.001, 0.01, 0.1, 0.5, 0.9):
        mask = rng.random(n) < frac
        rows = np.nonzero(mask)[0]
        sub = ix.subset(mask)
        assert sub.rows == rows.size
        for k in (1, 50, 1000, 2048):
            D, I = sub_search(ix, q, k, sub)
            Dr, Ir = expect(corpus, rows, q, k)
            assert np.array_equal(D, Dr) and np.array_equal(I, Ir), (frac, k)
        sub.close()
    ix.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_subset_is_the_full_ranking_restricted(dtype):
    n, d = 2048, 384
    corpus = H.gauss(5, n, d)
    q = H.gauss(6, 1, d, normalize=False)
    ix = FlatIPIndex.from_array(corpus, dtype=dtype)
    Df, If = ix.search(q, n)
    rng = np.random.default_rng(7)
    for frac in (0.02, 0.3, 0.8):
        mask = rng.random(n) < frac
        keep = mask[If[0]]
        for k in (1, 17, 300):
            D, I = sub_search(ix, q, k, mask)
            m = min(k, int(mask.sum()))
            assert np.array_equal(D[0, :m], Df[0][keep][:m]) and np.array_equal(I[0, :m], If[0][keep][:m])
            assert (I[0, m:] == -1).all() and (D[0, m:] == -np.finfo(np.float32).max).all()
    ix.close()


def test_f16_subsets_and_integer_ties():
    n, d = 20_000, 384
    corpus = H.gauss(8, n, d)
    q = H.gauss(9, 2, d)
    ix = FlatIPIndex.from_array(corpus, dtype="f16")
    rows = np.sort(np.random.default_rng(1).choice(n, 3000, replace=False))
    D, I = sub_search(ix, q, 100, rows)
    Dr, Ir = expect(corpus, rows, q, 100, f16=True)
    _, _, Sref = oracle.np_search(corpus[rows], q, 100, f16=True)
    rep = oracle.compare_topk(D, np.where(I >= 0, np.searchsorted(rows, I), -1), Dr,
                              np.where(Ir >= 0, np.searchsorted(rows, Ir), -1), Sref)
    assert rep["recall"] == 1.0, rep
    ix.close()
    ic = H.int_corpus(2, 5000, 128)
    ic[1000:2000] = ic[:1000]  # duplicate rows: ties everywhere, row-ascending
    qi = H.int_corpus(3, 1, 128)
    ix = FlatIPIndex.from_array(ic, dtype="f16")
    rows = np.arange(0, 5000, 3)
    D, I = sub_search(ix, qi, 500, rows)
    Dr, Ir = expect(ic, rows, qi, 500)
    assert np.array_equal(D, Dr) and np.array_equal(I, Ir)
    ix.close()


def test_edge_cases():
    n, d = 5000, 128
    corpus = H.gauss(12, n, d)
    corpus[100] = np.nan
    corpus[101] = -np.inf
    q = H.gauss(13, 5, d, normalize=False)
    ix = FlatIPIndex.from_array(corpus)
    # empty subset, m < k, single row
    D, I = sub_search(ix, q[:1], 10, np.zeros(n, bool))
    assert (I == -1).all() and (D == -np.finfo(np.float32).max).all()
    for rows in (np.array([4321]), np.array([3, 99, 100, 101, 102, 4999])):
        D, I = sub_search(ix, q[:1], 10, rows)
        Dr, Ir = expect(corpus, rows, q[:1], 10)
        assert np.array_equal(D, Dr) and np.array_equal(I, Ir)
        assert not np.isin(I, [100, 101]).any()
    # stray bits past ntotal, short bitmap
    bm = np.full((n + 64) // 8, 0xFF, np.uint8)
    s = ix.subset(fc.IDSelectorBitmap(bm))
    assert s.rows == n
    short = ix.subset(fc.IDSelectorBitmap(np.full(10, 0xFF, np.uint8)))
    assert short.rows == 80
    D, I = sub_search(ix, q[:1], 100, short)
    assert I[0].max() < 80
    # nq = 5: each query equals its lone call
    rows = np.arange(0, n, 7)
    sub = ix.subset(rows)
    D5, I5 = sub_search(ix, q, 64, sub)
    for i in range(5):
        D1, I1 = sub_search(ix, q[i:i + 1], 64, sub)
        assert np.array_equal(D5[i], D1[0]) and np.array_equal(I5[i], I1[0])
    # ls_set_base, then ls_add after creation: the subset keeps its rows
    ix2 = FlatIPIndex.from_array(corpus, base=1_000_000)
    sub2 = ix2.subset(rows)
    D, I = sub_search(ix2, q[:1], 20, sub2)
    Dr, Ir = expect(corpus, rows, q[:1], 20)
    assert np.array_equal(D, Dr) and np.array_equal(I, Ir + 1_000_000)
    ix2.add(H.gauss(14, 100, d))
    D, I = sub_search(ix2, q[:1], 20, sub2)
    assert np.array_equal(I, Ir + 1_000_000)
    # k rule and flags
    with pytest.raises(native.LeanSearchError) as e:
        sub_search(ix, q[:1], 4096, np.ones(n, bool))
    assert e.value.code == native.LS_ERR_K_TOO_LARGE
    D, I = sub_search(ix, q[:1], 4096, rows[:100])  # min(k, m) <= LS_MAX_K
    assert (I[0, 100:] == -1).all()
    ix2.close()
    assert not sub2.valid
    ix.close()


def test_forced_rescue_paths_stay_exact():
    n, d = 40_000, 384
    corpus = H.gauss(15, n, d)
    q = H.gauss(16, 2, d, normalize=False)
    rows = np.nonzero(np.random.default_rng(3).random(n) < 0.3)[0]
    Dr, Ir = expect(corpus, rows, q, 200)
    for opt in (0, 1):
        ix = FlatIPIndex.from_array(corpus)
        ix.debug_option(opt, 1)
        D, I = sub_search(ix, q, 200, rows)
        assert np.array_equal(D, Dr) and np.array_equal(I, Ir), opt
        ix.close()


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
def test_sharded_and_replicated_match_single_device(devices):
    n, d = 30_001, 384
    corpus = H.gauss(17, n, d)
    q = H.gauss(18, 3, d, normalize=False)
    single = FlatIPIndex.from_array(corpus)
    sh = FlatIPIndex.from_array(corpus, devices=devices)
    rep = FlatIPIndex.from_array(corpus, devices=devices, replicate=True)
    lo, rows_g = sh.shards()[1][1], sh.shards()[1][2]
    rng = np.random.default_rng(4)
    for rows in (np.nonzero(rng.random(n) < 0.2)[0], np.arange(lo + 3, lo + rows_g - 5, 2)):  # one inside a shard
        for k in (10, 1000):
            D0, I0 = sub_search(single, q, k, rows, normalize=True)
            for ix in (sh, rep):
                D, I = sub_search(ix, q, k, rows, normalize=True)
                assert np.array_equal(D, D0) and np.array_equal(I, I0)
    for ix in (single, sh, rep):
        ix.close()


def test_concurrent_plain_and_subset_callers():
    n, d = 50_000, 384
    corpus = H.gauss(19, n, d)
    qs = H.gauss(20, 16, d, normalize=False)
    ix = FlatIPIndex.from_array(corpus)
    subs = [ix.subset(np.arange(s, n, 3 + s)) for s in range(3)]
    want = {}
    for i in range(len(qs)):
        want[("p", i)] = ix.search(qs[i:i + 1], 50)
        for s, sub in enumerate(subs):
            want[(s, i)] = sub_search(ix, qs[i:i + 1], 50, sub)
    bad, done = [], [0]

    def worker(t):
        rng = np.random.default_rng(t)
        end = time.time() + 2.0
        while time.time() < end:
            i = int(rng.integers(len(qs)))
            kind = "p" if t % 2 == 0 else int(rng.integers(3))
            got = ix.search(qs[i:i + 1], 50) if kind == "p" else sub_search(ix, qs[i:i + 1], 50, subs[kind])
            w = want[(kind, i)]
            if not (np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1])):
                bad.append((t, kind, i))
            done[0] += 1

    th = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not bad and done[0] > 16
    ix.close()


def test_service_prefilter_on_the_gpu_index(tmp_path):
    """Service.search(packages=..., prefilter_packages=True) on a FlatIPIndex: the dense candidates are the oracle's
    top-faiss_k among the package's rows."""
    import asyncio

    from lean_explore_amd import loader
    from lean_explore_amd import search as S
    from tests.test_subset_cpu import FakeEmbed, _make_db

    n, d = 3000, 64
    corpus = H.gauss(21, n, d)
    rows = []
    for i in range(n):
        pkg = "Small" if i % 10 == 0 else "Big"
        rows.append((5000 + i, f"{pkg}.decl{i}", f"{pkg}.Mod", None, f"def d{i}", f"http://x/{i}", None,
                     f"informal {i}", loader.embedding_to_blob(corpus[i].tolist())))
    db = tmp_path / "lean_explore.db"
    _make_db(db, rows)
    ids, loaded = loader.load_corpus_from_sqlite(db)
    ix = FlatIPIndex.from_array(loaded)
    qvec = corpus[1] * 3.0
    eng = S.SearchEngine(db_path=db, embedding_client=FakeEmbed(qvec), index=ix, ids_map=ids, lexical_retriever=False)
    faiss_k = 40
    sem = asyncio.run(eng._retrieve_semantic_candidates("q", faiss_k, ["Small"]))
    sel = np.array([r for r, i in enumerate(ids) if (i - 5000) % 10 == 0])
    D, I = expect(loaded, sel, np.array([qvec], np.float32), faiss_k, normalize=True)
    want = [ids[r] for r in I[0] if r >= 0]
    assert list(sem) == want
    resp = asyncio.run(S.Service(engine=eng).search("q", limit=10, rerank_top=None, packages=["Small"],
                                                    prefilter_packages=True))
    assert resp.count == 10 and all(r.module.startswith("Small") for r in resp.results)
    ix.close()


@pytest.mark.parametrize("shards,k", [(8, 2048), (8, 1500), (5, 2048)])
def test_many_shards_merge_in_rounds(shards, k):
    """G * k past one merge launch's keys (8192): the sharded subset search merges in rounds, like ls_search."""
    n, d = 40_003, 128
    corpus = H.gauss(22, n, d)
    q = H.gauss(23, 2, d, normalize=False)
    single = FlatIPIndex.from_array(corpus)
    sh = FlatIPIndex.from_array(corpus, devices=[0] * shards)
    rows = np.nonzero(np.random.default_rng(shards).random(n) < 0.6)[0]
    D0, I0 = sub_search(single, q, k, rows)
    D, I = sub_search(sh, q, k, rows)
    assert np.array_equal(D, D0) and np.array_equal(I, I0)
    Dp, Ip = sh.search(q, k)  # the plain search of the same handle, for comparison: it takes this k too
    assert Ip.shape == (2, k)
    Dr, Ir = expect(corpus, rows, q, k)
    assert np.array_equal(D, Dr) and np.array_equal(I, Ir)
    single.close()
    sh.close()


def test_replicated_calls_round_robin_and_agree():
    n, d = 20_000, 256
    corpus = H.gauss(24, n, d)
    q = H.gauss(25, 1, d, normalize=False)
    rep = FlatIPIndex.from_array(corpus, devices=[0, 0, 0], replicate=True)
    sub = rep.subset(np.arange(5, n, 4))
    first = sub_search(rep, q, 100, sub)
    for _ in range(5):  # consecutive calls go to replicas 1, 2, 0, ...: all hold the subset and agree
        D, I = sub_search(rep, q, 100, sub)
        assert np.array_equal(D, first[0]) and np.array_equal(I, first[1])
    Dr, Ir = expect(corpus, np.arange(5, n, 4), q, 100)
    assert np.array_equal(first[0], Dr) and np.array_equal(first[1], Ir)
    rep.close()
