"""IVF-flat search on the MI355X (include/leansearch_ivf.h, lean_explore_amd.ivf.IVFFlatIndex).

The definition under test: the probed lists of a query are the top ``nprobe`` rows of the library's exact search over
the centroids, and the result is the library's exact SUBSET search (``ls_search_subset``) of a flat index of the same
rows over the rows of those lists - scores and indices, bit for bit. Every comparison below is ``array_equal`` over
every query and every slot unless it says otherwise; nothing asserts a time.

Corpora are seeded Gaussian mixtures around the centroids with Zipf-like component weights: clustered rows, uneven lists.
"""

import numpy as np
import pytest

from lean_explore_amd import faiss_compat, loader, native
from lean_explore_amd import search as S
from lean_explore_amd.id_selectors import IDSelectorBitmap, SearchParameters, SearchParametersIVF
from lean_explore_amd.index import FlatIPIndex
from lean_explore_amd.ivf import IVFFlatIndex
from oracle import oracle
from tests import helpers as H
from tests.test_glue_cpu import FakeEmbed, _make_db, run
from tests.test_ivf_cpu import write_iwfl

pytestmark = pytest.mark.gpu

NEG = np.float32(-np.finfo(np.float32).max)
NQ = 16

# name: (rows, d, dtype, nlist, k)
SHAPES = {
    "5k_64": (5_000, 64, "f32", 64, 10),
    "c2": (200_000, 384, "f32", 447, 50),
    "c2p": (200_000, 1024, "f32", 447, 1000),
    "c2_f16": (200_000, 384, "f16", 447, 100),
    "768_f16": (100_000, 768, "f16", 316, 50),
}


def mixture(seed, n, d, nlist, sigma=0.35):
    """(rows [n, d] unit norm, centroids [nlist, d] unit norm): component c has weight ~ 1 / (c + 3)."""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((nlist, d), dtype=np.float32)
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    w = 1.0 / (np.arange(nlist) + 3.0)
    comp = rng.choice(nlist, size=n, p=w / w.sum())
    x = rng.standard_normal((n, d), dtype=np.float32)
    x *= np.float32(sigma / np.sqrt(d))
    x += cent[comp]
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x, cent


def queries(seed, corpus, nq=NQ):
    """Rows of the corpus, perturbed and rescaled: not unit norm, so LS_FLAG_NORMALIZE has work to do."""
    rng = np.random.default_rng(seed)
    pick = rng.choice(corpus.shape[0], nq, replace=False)
    q = corpus[pick] + np.float32(0.05) * rng.standard_normal((nq, corpus.shape[1]), dtype=np.float32)
    return np.ascontiguousarray(q * np.float32(2.5), dtype=np.float32)


class Built:
    def __init__(self, name):
        n, d, dtype, nlist, k = SHAPES[name]
        self.n, self.d, self.dtype, self.nlist, self.k = n, d, dtype, nlist, k
        self.corpus, self.cent = mixture(1000 + n + d, n, d, nlist)
        self.q = queries(77 + d, self.corpus)
        self.flat = FlatIPIndex.from_array(self.corpus, dtype=dtype)
        self.ivf = IVFFlatIndex(d, nlist, dtype=dtype)
        self.ivf.set_centroids(self.cent)
        self.ivf.add(self.corpus)
        self.assign = self.ivf.assignment()  # (builds the device object)
        self.coarse = FlatIPIndex.from_array(self.cent)  # an independent handle of the centroids

    def close(self):
        for ix in (self.flat, self.ivf, self.coarse):
            ix.close()


@pytest.fixture(scope="module", params=list(SHAPES))
def built(request):
    b = Built(request.param)
    yield b
    b.close()


def probed_bitmap(assign, lists):
    lists = np.asarray(lists)
    mask = np.isin(assign, lists[lists >= 0])
    return np.packbits(mask, bitorder="little"), mask


def subset_reference(flat, coarse, assign, q, k, nprobe, normalize):
    """The definition, spelled with the flat index's public calls: probe lists from an independent exact search over
    the centroids, a bitmap of their rows, one subset search per query."""
    _, P = coarse.search(q, min(nprobe, coarse.ntotal), normalize=normalize)
    D = np.empty((q.shape[0], k), np.float32)
    I = np.empty((q.shape[0], k), np.int64)
    masks = []
    for i in range(q.shape[0]):
        bm, mask = probed_bitmap(assign, P[i])
        D[i], I[i] = (a[0] for a in flat.search(q[i:i + 1], k, normalize=normalize,
                                                params=SearchParameters(sel=IDSelectorBitmap(bm))))
        masks.append(mask)
    return D, I, masks


# ---- case 1 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [False, True])
def test_all_lists_probed_equals_flat_search(built, normalize):
    b = built
    D, I = b.ivf.search(b.q, b.k, normalize=normalize, params=SearchParametersIVF(nprobe=b.nlist))
    for i in range(NQ):  # query by query: the flat index's single-query scan
        Df, If = b.flat.search(b.q[i:i + 1], b.k, normalize=normalize)
        assert np.array_equal(I[i], If[0]), i
        assert np.array_equal(D[i], Df[0]), i
    assert (I >= 0).all()


# ---- case 2 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nprobe", [1, 7, 64])
def test_probed_lists_equal_subset_search(built, nprobe):
    b = built
    normalize = b.d != 64  # (the small shape runs on the raw queries)
    Dr, Ir, masks = subset_reference(b.flat, b.coarse, b.assign, b.q, b.k, nprobe, normalize)
    b.ivf.nprobe = nprobe
    D, I = b.ivf.search(b.q, b.k, normalize=normalize)  # one 16-query call ...
    assert np.array_equal(I, Ir)
    assert np.array_equal(D, Dr)
    for i in range(NQ):  # ... equals its 16 single-query calls
        D1, I1 = b.ivf.search(b.q[i:i + 1], b.k, normalize=normalize)
        assert np.array_equal(I1[0], I[i]) and np.array_equal(D1[0], D[i]), i
    probed = np.array([m.sum() for m in masks])
    print(f"\n[{b.n}x{b.d} {b.dtype} nlist {b.nlist} nprobe {nprobe}] rows probed mean {probed.mean():.0f} "
          f"max {probed.max()} of {b.n}")


# ---- case 3 ----------------------------------------------------------------------------------------------------------
def test_definition_against_the_cpu_oracle(built):
    """float64 twin over the probed rows of every query; the project's bars (scores within 1e-5, an index may differ
    only where the oracle's own scores are within 2e-6); recall within the probed set must be 1.0."""
    b = built
    nprobe = 7 if b.nlist == 64 else 64
    _, P = b.coarse.search(b.q, nprobe, normalize=True)
    D, I = b.ivf.search(b.q, b.k, normalize=True, params=SearchParametersIVF(nprobe=nprobe))
    qn = oracle.np_normalize_l2(b.q)
    for i in range(NQ):
        rows = np.flatnonzero(np.isin(b.assign, P[i]))
        Dr, Ir, Sr = oracle.np_search(b.corpus[rows], qn[i:i + 1], b.k, f16=(b.dtype == "f16"))
        got = I[i:i + 1].copy()
        ok = got >= 0
        assert np.isin(got[ok], rows).all(), "a returned row is not in a probed list"
        got[ok] = np.searchsorted(rows, got[ok])  # original rows -> positions in the probed set (rows ascend)
        rep = oracle.compare_topk(D[i:i + 1], got, Dr, Ir, Sr)
        assert rep["recall"] == 1.0, (i, rep)


# ---- case 4 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_integer_corpus_with_duplicates_across_lists(dtype):
    """Integer-valued rows: every score is exact, thousands of rows tie, and each query row has 240 copies spread over
    all lists, so that rank k falls INSIDE its tie group (about nprobe / nlist of the copies are probed)."""
    n, d, nlist, copies = 24_000, 64, 32, 240
    rng = np.random.default_rng(404)
    corpus = H.int_corpus(41, n, d)
    base_rows = rng.choice(n, 20, replace=False)
    for r in base_rows:
        where = rng.choice(n, copies, replace=False)
        corpus[where] = corpus[r]
    assign = rng.integers(0, nlist, n).astype(np.int32)  # the copies land in different lists
    cent = H.int_corpus(43, nlist, d)
    flat = FlatIPIndex.from_array(corpus, dtype=dtype)
    coarse = FlatIPIndex.from_array(cent)
    ivf = IVFFlatIndex(d, nlist, dtype=dtype)
    ivf.set_centroids(cent)
    ivf.add(corpus, assign=assign)
    q = np.ascontiguousarray(corpus[base_rows[:NQ]])
    for nprobe, k in ((8, 30), (8, 300), (3, 1000), (32, 100)):
        Dr, Ir, masks = subset_reference(flat, coarse, assign, q, k, nprobe, False)
        D, I = ivf.search(q, k, params=SearchParametersIVF(nprobe=nprobe))
        assert np.array_equal(I, Ir) and np.array_equal(D, Dr), (nprobe, k)
        if k == 30:  # rank k is inside the group of the query's own copies: the k-th and (k+1)-th probed rows tie
            for i in range(NQ):
                top = float(q[i] @ q[i])
                tied = int((corpus[masks[i]] @ q[i] == top).sum())
                assert tied > k and (D[i] == np.float32(top)).all(), (i, tied)
    assert np.array_equal(ivf.list_sizes(), np.bincount(assign, minlength=nlist))
    for ix in (flat, coarse, ivf):
        ix.close()


# ---- case 5 ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def forced():
    """Explicit assignment: lists 1 and 2 are empty, list 0 holds a third of the rows, list 11 holds 5 rows."""
    n, d, nlist = 3_000, 32, 12
    corpus, _ = mixture(9, n, d, nlist)
    rng = np.random.default_rng(10)
    assign = rng.integers(3, 11, n).astype(np.int32)
    five = np.array([5, 600, 1200, 1800, 2999])
    others = np.setdiff1d(np.arange(n), five)
    assign[rng.choice(others, n // 3, replace=False)] = 0  # (never one of list 11's five rows)
    assign[five] = 11
    cent = rng.standard_normal((nlist, d), dtype=np.float32)
    flat = FlatIPIndex.from_array(corpus)
    coarse = FlatIPIndex.from_array(cent)
    ivf = IVFFlatIndex(d, nlist)
    ivf.set_centroids(cent)
    ivf.add(corpus, assign=assign)
    yield corpus, assign, cent, flat, coarse, ivf
    for ix in (flat, coarse, ivf):
        ix.close()


def test_edges_padding_and_empty_lists(forced):
    corpus, assign, cent, flat, coarse, ivf = forced
    sizes = ivf.list_sizes()
    assert sizes[1] == 0 and sizes[2] == 0 and sizes[0] >= 1000 and sizes[11] == 5
    assert np.array_equal(sizes, np.bincount(assign, minlength=12)) and np.array_equal(ivf.assignment(), assign)
    # fewer probed rows than k: the query that probes list 11 alone gets 5 rows and padding
    q11 = np.ascontiguousarray(cent[11:12] * 4.0)
    D, I = ivf.search(q11, 40, params=SearchParametersIVF(nprobe=1))
    Dr, Ir, _ = subset_reference(flat, coarse, assign, q11, 40, 1, False)
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
    assert sorted(I[0, :5].tolist()) == [5, 600, 1200, 1800, 2999] and (I[0, 5:] == -1).all() and (D[0, 5:] == NEG).all()
    # every probed list empty: the query lies on the centroids of lists 1 and 2
    qe = np.ascontiguousarray((cent[1:2] + cent[2:3]) * 10.0)
    _, P = coarse.search(qe, 2)
    assert sorted(P[0].tolist()) == [1, 2]
    D, I = ivf.search(qe, 7, params=SearchParametersIVF(nprobe=2))
    assert (I == -1).all() and (D == NEG).all()
    # mixed: all sixteen queries, several nprobe, k past the probed rows of some
    q = queries(3, corpus)
    for nprobe in (1, 2, 5, 12):
        Dr, Ir, _ = subset_reference(flat, coarse, assign, q, 1500, nprobe, True)
        D, I = ivf.search(q, 1500, normalize=True, params=SearchParametersIVF(nprobe=nprobe))
        assert np.array_equal(I, Ir) and np.array_equal(D, Dr), nprobe
    # nprobe > nlist clamps
    Da, Ia = ivf.search(q, 20, params=SearchParametersIVF(nprobe=12))
    Db, Ib = ivf.search(q, 20, params=SearchParametersIVF(nprobe=100_000))
    Df, If = flat.search(q, 20)
    assert np.array_equal(Ia, Ib) and np.array_equal(Da, Db) and np.array_equal(Ia, If) and np.array_equal(Da, Df)
    # nq = 0
    D, I = ivf.search(np.zeros((0, 32), np.float32), 9)
    assert D.shape == (0, 9) and I.shape == (0, 9)
    lib = native.load()
    assert lib.ls_ivf_search(ivf._handle, None, 0, 9, 1, 0, None, None) == native.LS_OK
    assert lib.ls_ivf_search(ivf._handle, q.ctypes.data, 1, 9, 0, 0, D.ctypes.data, I.ctypes.data) == native.LS_ERR_INVALID_ARG
    assert lib.ls_ivf_ntotal(ivf._handle) == 3000 and lib.ls_ivf_dim(ivf._handle) == 32 and lib.ls_ivf_nlist(ivf._handle) == 12


def test_edges_nan_and_inf_rows():
    n, d, nlist = 4_000, 48, 16
    corpus, cent = mixture(21, n, d, nlist)
    corpus[7, 3] = np.nan
    corpus[100] = np.nan
    corpus[250, 0] = np.inf
    corpus[251, 0] = -np.inf
    corpus[1999, 5] = np.inf
    corpus[3000, 5] = -np.inf
    corpus[3001, 1], corpus[3001, 2] = np.inf, -np.inf
    assign = np.random.default_rng(22).integers(0, nlist, n).astype(np.int32)
    flat = FlatIPIndex.from_array(corpus)
    coarse = FlatIPIndex.from_array(cent)
    ivf = IVFFlatIndex(d, nlist)
    ivf.set_centroids(cent)
    ivf.add(corpus, assign=assign)
    q = queries(23, np.nan_to_num(corpus, nan=0.0, posinf=1.0, neginf=-1.0))
    for nprobe in (4, 16):
        Dr, Ir, _ = subset_reference(flat, coarse, assign, q, 600, nprobe, False)
        D, I = ivf.search(q, 600, params=SearchParametersIVF(nprobe=nprobe))
        assert np.array_equal(I, Ir) and np.array_equal(D, Dr, equal_nan=True), nprobe
        assert not np.isnan(D).any() and not np.isin(I, [7, 100]).any()  # (rows with a NaN component score NaN)
    # the default assignment sends a row no centroid scores (NaN) to list 0
    ivf2 = IVFFlatIndex(d, nlist)
    ivf2.set_centroids(cent)
    ivf2.add(corpus)
    a = ivf2.assignment()
    assert a[100] == 0 and a[7] == 0
    for ix in (flat, coarse, ivf, ivf2):
        ix.close()


def test_edges_empty_index_and_max_k():
    ivf = IVFFlatIndex(16, 4)
    ivf.set_centroids(H.gauss(1, 4, 16))
    D, I = ivf.search(H.gauss(2, 3, 16), 5)  # n = 0
    assert ivf.ntotal == 0 and (I == -1).all() and (D == NEG).all() and (ivf.list_sizes() == 0).all()
    ivf.close()

    n, d, nlist = 5_000, 64, 64
    corpus, cent = mixture(31, n, d, nlist)
    flat = FlatIPIndex.from_array(corpus)
    coarse = FlatIPIndex.from_array(cent)
    ivf = IVFFlatIndex(d, nlist)
    ivf.set_centroids(cent)
    ivf.add(corpus)
    assign = ivf.assignment()
    q = queries(32, corpus)
    k = native.LS_MAX_K
    D, I = ivf.search(q, k, params=SearchParametersIVF(nprobe=nlist))
    Df, If = flat.search(q, k)
    for i in range(NQ):
        D1, I1 = flat.search(q[i:i + 1], k)
        assert np.array_equal(I[i], I1[0]) and np.array_equal(D[i], D1[0]), i
    assert np.array_equal(I, If)
    for nprobe in (7, 40):
        Dr, Ir, _ = subset_reference(flat, coarse, assign, q, k, nprobe, False)
        D, I = ivf.search(q, k, params=SearchParametersIVF(nprobe=nprobe))
        assert np.array_equal(I, Ir) and np.array_equal(D, Dr), nprobe
    with pytest.raises(native.LeanSearchError) as e:
        ivf.search(q, k + 1)
    assert e.value.code == native.LS_ERR_K_TOO_LARGE and "rows of the index" in str(e.value)
    for ix in (flat, coarse, ivf):
        ix.close()


def test_default_assignment_is_the_library_argmax_with_ties_to_the_lowest_list():
    n, d, nlist = 6_000, 32, 20
    corpus = H.int_corpus(51, n, d)
    cent = H.int_corpus(52, nlist, d)
    cent[9] = cent[4]   # a duplicated centroid: every tie between them goes to list 4
    cent[15] = cent[4]
    ivf = IVFFlatIndex(d, nlist)
    ivf.set_centroids(cent)
    ivf.add(corpus)
    a = ivf.assignment()
    _, nearest = ivf.quantizer.search(corpus, 1)
    assert np.array_equal(a, nearest[:, 0].astype(np.int32))
    scores = corpus @ cent.T  # small integers: exact in float32
    assert np.array_equal(a, np.argmax(scores, axis=1))  # (argmax takes the first maximum: the lowest list)
    sizes = ivf.list_sizes()
    assert sizes[9] == 0 and sizes[15] == 0 and sizes[4] > 0 and sizes.sum() == n
    assert (scores.max(axis=1)[:, None] == scores).sum(axis=1).max() > 1  # ties did occur
    ivf.close()


# ---- case 6 ----------------------------------------------------------------------------------------------------------
def test_index_file_with_real_centroids(tmp_path):
    n, d, nlist = 30_000, 128, 100
    corpus, cent = mixture(61, n, d, nlist)
    coarse = FlatIPIndex.from_array(cent)
    _, a = coarse.search(corpus, 1)
    assign = a[:, 0].astype(np.int32)
    p = tmp_path / "ivf.index"
    write_iwfl(p, corpus, assign, cent, nprobe=9)
    ivf = faiss_compat.read_index(p, ivf=True)
    assert isinstance(ivf, IVFFlatIndex) and ivf.nprobe == 9 and ivf.ntotal == n
    flat = faiss_compat.read_index(p)
    q = queries(62, corpus)
    Dr, Ir, _ = subset_reference(flat, coarse, assign, q, 50, 9, True)
    D, I = ivf.search(q, 50, normalize=True)
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
    assert np.array_equal(ivf.assignment(), assign)
    Dr, Ir, _ = subset_reference(flat, coarse, assign, q, 50, 33, True)
    D, I = ivf.search(q, 50, normalize=True, params=SearchParametersIVF(nprobe=33))
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
    for ix in (flat, coarse, ivf):
        ix.close()


@pytest.mark.parametrize("nlist", [48, 160])
def test_engine_semantic_index_ivf(tmp_path, nlist):
    """The engine sets nprobe = 64 as the reference does: with 48 lists that probes everything (identical to the flat
    engine), with 160 lists the candidates are a subset of the flat engine's exact candidates over the probed rows."""
    n, d = 2_000, 96
    corpus, cent = mixture(71, n, d, nlist)
    rows = [(5000 + i, f"Mathlib.decl{i}", "Mathlib.Mod", "doc", f"theorem t{i}", f"http://x/{i}", None,
             f"statement {i}", loader.embedding_to_blob(corpus[i].tolist())) for i in range(n)]
    db = tmp_path / "lean_explore.db"
    _make_db(db, rows)
    ids, loaded = loader.load_corpus_from_sqlite(db)
    assert np.array_equal(loaded, corpus)
    loader.save_ids_map(tmp_path / "informalization_faiss_ids_map.json", ids)
    coarse = FlatIPIndex.from_array(cent)
    _, a = coarse.search(loaded, 1)
    assign = a[:, 0].astype(np.int32)
    write_iwfl(tmp_path / "informalization_faiss.index", loaded, assign, cent, nprobe=1)
    qvec = corpus[123] * 3.0 + 0.01 * H.gauss(5, 1, d)[0]
    flat_eng = S.SearchEngine(base_path=tmp_path, embedding_client=FakeEmbed(qvec), lexical_retriever=False)
    ivf_eng = S.SearchEngine(base_path=tmp_path, embedding_client=FakeEmbed(qvec), lexical_retriever=False,
                             semantic_index="ivf")
    k = 200
    sem_flat = run(flat_eng._retrieve_semantic_candidates("q", n))  # every row, exact
    sem_ivf = run(ivf_eng._retrieve_semantic_candidates("q", k))
    assert isinstance(ivf_eng.faiss_informal_index, IVFFlatIndex) and ivf_eng.faiss_informal_index.nprobe == 64
    assert type(flat_eng.faiss_informal_index) is FlatIPIndex
    assert list(sem_ivf)[0] == 5123 and len(sem_ivf) == k
    assert set(sem_ivf) <= set(sem_flat)
    for i, s in sem_ivf.items():
        assert sem_flat[i] == s  # the same score bits
    # the flat engine's exact candidates restricted to the probed rows, in its order
    x = np.ascontiguousarray(qvec[None, :], dtype=np.float32)
    _, P = coarse.search(x, min(64, nlist), normalize=True)
    probed_ids = {ids[r] for r in np.flatnonzero(np.isin(assign, P[0]))}
    want = [i for i in sem_flat if i in probed_ids][:k]
    assert list(sem_ivf) == want
    if nlist <= 64:
        assert list(sem_ivf) == list(sem_flat)[:k]
        assert list(sem_ivf) == list(run(flat_eng._retrieve_semantic_candidates("q", k)))
    r = run(S.Service(engine=ivf_eng).search("q", limit=20, rerank_top=0))
    assert r.count == len(r.results) > 0 and r.results[0].id == 5123
    with pytest.raises(ValueError):
        run(ivf_eng.search_prefiltered("q", ["Mathlib"]))
    coarse.close()


# ---- case 7 ----------------------------------------------------------------------------------------------------------
def test_train_is_deterministic_and_fills_every_list():
    n, d, nlist = 40_000, 64, 100
    corpus, _ = mixture(81, n, d, nlist, sigma=0.5)
    a = IVFFlatIndex(d, nlist)
    a.train(corpus, niter=8, seed=7)
    b = IVFFlatIndex(d, nlist)
    b.train(corpus, niter=8, seed=7)
    c = IVFFlatIndex(d, nlist)
    c.train(corpus, niter=8, seed=8)
    assert a.is_trained and np.array_equal(a.centroids, b.centroids)
    assert not np.array_equal(a.centroids, c.centroids)
    assert a.centroids.shape == (nlist, d) and np.isfinite(a.centroids).all()
    assert np.array_equal(a.quantizer.host_corpus(), a.centroids)
    a.add(corpus)
    sizes = a.list_sizes()
    assert sizes.sum() == n and (sizes > 0).all(), sizes
    flat = FlatIPIndex.from_array(corpus)
    q = queries(82, corpus, 64)
    a.nprobe = 64
    _, I = a.search(q, 50, normalize=True)
    _, If = flat.search(q, 50, normalize=True)
    recall = np.mean([len(set(I[i]) & set(If[i])) / 50.0 for i in range(q.shape[0])])
    print(f"\n[train] nlist {nlist} sizes min {sizes.min()} max {sizes.max()}  recall@50 of nprobe 64 vs exact: {recall:.4f}")
    for ix in (a, b, c, flat):
        ix.close()
