"""IVF search over a row subset on the MI355X (include/leansearch_ivf_subset.h, IVFFlatIndex.subset / IVFSubset).

The definition under test: per query, what the flat index's subset search returns for the bitmap (rows of the probed
lists) AND (selected rows) - scores and rows, bit for bit; the probed lists are those of the unfiltered IVF search.
Section (e) compares with host-only references (tests/test_geometry_cpu.py) at every row geometry an IVF index can
have; section (f) with the library's own flat subset search at larger shapes. Every comparison is ``array_equal`` except
the Gaussian f16 cases of (e), which go through the project's bars (Checker). Nothing asserts a time."""

import numpy as np
import pytest

from lean_explore_amd import loader, native
from lean_explore_amd import search as S
from lean_explore_amd.id_selectors import IDSelectorBitmap, SearchParameters, SearchParametersIVF
from lean_explore_amd.index import FlatIPIndex
from lean_explore_amd.ivf import IVFFlatIndex, IVFSubset
from tests import helpers as H
from tests.test_geometry_cpu import N, ivf_reference, seen_queries, selections, uneven_assignment
from tests.test_geometry_gpu import IVF_CASES, NLIST, Checker, make_data
from tests.test_glue_cpu import FakeEmbed, _make_db, run
from tests.test_ivf_cpu import write_iwfl
from tests.test_ivf_gpu import NQ, mixture, probed_bitmap, queries

pytestmark = pytest.mark.gpu

NEG = np.float32(-np.finfo(np.float32).max)


# ---- (e) ----------------------------------------------------------------------------------------------------------------
def subset_selections(assign):
    sel = dict(selections())  # mask10, forty, one, ones
    sel["list7"] = np.flatnonzero(assign == 7)
    sel["empty"] = np.zeros(0, np.int64)
    sel["half"] = np.flatnonzero(np.random.default_rng(32).random(N) < 0.5)
    return sel


@pytest.mark.parametrize("dtype, d, kind", IVF_CASES)
def test_every_geometry_against_the_host_reference(dtype, d, kind):
    corpus, groups = make_data(dtype, d, kind)
    assign = uneven_assignment()
    cent = H.gauss(90 + d, NLIST, d)
    check = Checker(corpus, dtype, kind)
    ivf = IVFFlatIndex(d, NLIST, dtype=dtype)
    ivf.set_centroids(cent)
    ivf.add(corpus, assign=assign)
    sel = subset_selections(assign)
    subs = {name: ivf.subset(rows) for name, rows in sel.items()}
    try:
        sizes = np.bincount(assign, minlength=NLIST)
        for name, rows in sel.items():  # the compaction, through the getter
            assert subs[name].rows == rows.size and subs[name].valid
            assert np.array_equal(subs[name].list_sizes(), np.bincount(assign[rows], minlength=NLIST)), name
        assert np.array_equal(subs["ones"].list_sizes(), sizes) and subs["list7"].rows == sizes[7] == N // 3
        for q, normalize in groups:
            nq = q.shape[0]
            qn = seen_queries(q, normalize)
            for nprobe in (1, 5, NLIST):
                # (k = 1: only the probed rows of every query are wanted from the reference)
                _, _, probed = ivf_reference(corpus, cent, assign, q, 1, nprobe, normalize, dtype, flat=check.flat)
                for name, rows in sel.items():
                    want_rows = [np.intersect1d(p, rows) for p in probed]
                    params = SearchParametersIVF(sel=subs[name], nprobe=nprobe)
                    for k in (1, 50, 1500):
                        D, I = ivf.search(q, k, normalize=normalize, params=params)
                        second = ivf.last_kernel_ms()[2]
                        for i in range(nq):
                            what = f"{name} nprobe={nprobe} k={k} query {i}"
                            m = want_rows[i].size
                            check(D[i:i + 1], I[i:i + 1], want_rows[i], qn[i:i + 1], k, what)
                            assert (I[i, m:] == -1).all() and (D[i, m:] == NEG).all() and (I[i, :min(k, m)] >= 0).all(), what
                            D1, I1 = ivf.search(q[i:i + 1], k, normalize=normalize, params=params)
                            assert np.array_equal(I1[0], I[i]) and np.array_equal(D1[0], D[i]), what + " alone"
                        if nprobe == NLIST and k == 1500 and name in ("ones", "half"):
                            # 3001 (about 1500) rows probed and selected: the workgroups' 15 keys each cannot prove
                            # 1500 (every) rank(s) - each query is served by the second launch, over the row list
                            assert second == nq, (name, second, nq)
                            assert ivf.last_kernel_ms()[2] == 1  # (the single-query call just made)
                    if name == "ones":  # the all-ones subset is the unfiltered search
                        for k in (50, 1500):
                            D, I = ivf.search(q, k, normalize=normalize, params=params)
                            Du, Iu = ivf.search(q, k, normalize=normalize, params=SearchParametersIVF(nprobe=nprobe))
                            assert np.array_equal(I, Iu) and np.array_equal(D, Du), (nprobe, k)
    finally:
        for s in subs.values():
            s.close()
        ivf.close()


# ---- (f) ----------------------------------------------------------------------------------------------------------------
SHAPES = {"5k_64_f32": (5_000, 64, "f32", 64, 10), "20k_384_f32": (20_000, 384, "f32", 141, 50),
          "20k_384_f16": (20_000, 384, "f16", 141, 100), "20k_384_sq8": (20_000, 384, "sq8", 141, 50)}


class Built:
    def __init__(self, name):
        n, d, dtype, nlist, k = SHAPES[name]
        self.n, self.d, self.dtype, self.nlist, self.k = n, d, dtype, nlist, k
        self.corpus, self.cent = mixture(3000 + n + d, n, d, nlist)
        self.q = queries(55 + d, self.corpus)
        self.flat = FlatIPIndex.from_array(self.corpus, dtype=dtype)
        self.ivf = IVFFlatIndex(d, nlist, dtype=dtype)
        self.ivf.set_centroids(self.cent)
        self.ivf.add(self.corpus)
        self.assign = self.ivf.assignment()
        self.coarse = FlatIPIndex.from_array(self.cent)  # an independent handle of the centroids
        self.mask = np.random.default_rng(n + d).random(n) < 0.3
        self.sub = self.ivf.subset(self.mask)
        self.ones = self.ivf.subset(np.ones(n, bool))

    def close(self):
        for ix in (self.flat, self.ivf, self.coarse):
            ix.close()


@pytest.fixture(scope="module", params=list(SHAPES))
def built(request):
    b = Built(request.param)
    yield b
    b.close()


@pytest.mark.parametrize("nprobe", [1, 7, 64])
def test_equals_the_flat_subset_search_of_probed_and_selected(built, nprobe):
    b = built
    normalize = b.d != 64
    assert b.sub.rows == int(b.mask.sum()) and b.ones.rows == b.n
    _, P = b.coarse.search(b.q, min(nprobe, b.nlist), normalize=normalize)
    D, I = b.ivf.search(b.q, b.k, normalize=normalize, params=SearchParametersIVF(sel=b.sub, nprobe=nprobe))
    b.ivf.nprobe = nprobe
    Da, Ia = b.ivf.search(b.q, b.k, normalize=normalize, params=b.sub)  # the subset as `params`: nprobe of the attribute
    assert np.array_equal(Ia, I) and np.array_equal(Da, D)
    kept = []
    for i in range(NQ):
        _, probed = probed_bitmap(b.assign, P[i])
        both = probed & b.mask
        bm = np.packbits(both, bitorder="little")
        Df, If = b.flat.search(b.q[i:i + 1], b.k, normalize=normalize, params=SearchParameters(sel=IDSelectorBitmap(bm)))
        assert np.array_equal(I[i], If[0]), i
        assert np.array_equal(D[i], Df[0]), i
        D1, I1 = b.ivf.search(b.q[i:i + 1], b.k, normalize=normalize, params=b.sub)
        assert np.array_equal(I1[0], I[i]) and np.array_equal(D1[0], D[i]), i
        kept.append(int(both.sum()))
    # the one-shot form: create, search, close
    Do, Io = b.ivf.search_subset(b.q, b.k, b.mask, nprobe=nprobe, normalize=normalize)
    assert np.array_equal(Io, I) and np.array_equal(Do, D)
    # the all-ones subset is the unfiltered IVF search
    Du, Iu = b.ivf.search(b.q, b.k, normalize=normalize)
    D1, I1 = b.ivf.search(b.q, b.k, normalize=normalize, params=b.ones)
    assert np.array_equal(I1, Iu) and np.array_equal(D1, Du)
    print(f"\n[{b.n}x{b.d} {b.dtype} nlist {b.nlist} nprobe {nprobe}] rows probed and selected: mean {np.mean(kept):.0f} "
          f"max {max(kept)} of {b.sub.rows} selected")


@pytest.mark.parametrize("normalize", [False, True])
def test_all_lists_probed_equals_the_flat_subset_search(built, normalize):
    b = built
    D, I = b.ivf.search(b.q, b.k, normalize=normalize, params=SearchParametersIVF(sel=b.sub, nprobe=b.nlist))
    fsub = b.flat.subset(b.mask)
    for i in range(NQ):
        Df, If = b.flat.search(b.q[i:i + 1], b.k, normalize=normalize, params=SearchParameters(sel=fsub))
        assert np.array_equal(I[i], If[0]) and np.array_equal(D[i], Df[0]), i
    fsub.close()
    assert b.mask[I].all()


# ---- (g) ----------------------------------------------------------------------------------------------------------------
def small_pair(n=5_000, d=64, nlist=64, seed=31):
    corpus, cent = mixture(seed, n, d, nlist)
    flat = FlatIPIndex.from_array(corpus)
    ivf = IVFFlatIndex(d, nlist)
    ivf.set_centroids(cent)
    ivf.add(corpus)
    return corpus, flat, ivf


def test_lifetime_of_subsets():
    corpus, flat, ivf = small_pair()
    _, _, other = small_pair(seed=33)
    n, nlist = corpus.shape[0], ivf.nlist
    q = queries(34, corpus)
    a_rows, b_rows = np.arange(0, n, 3), np.arange(1000, 3000)
    a, b = ivf.subset(a_rows), ivf.subset(b_rows)  # two subsets alive at once
    assert isinstance(a, IVFSubset) and a.id != b.id and a.rows == a_rows.size and b.rows == b_rows.size
    assert ivf.subset(a) is a and a.sel is a
    want = {}
    for name, rows in (("a", a_rows), ("b", b_rows)):
        want[name] = [flat.search(q[i:i + 1], 20, params=SearchParameters(sel=rows)) for i in range(NQ)]
    for name, sub in (("a", a), ("b", b), ("a", a)):
        D, I = ivf.search(q, 20, params=SearchParametersIVF(sel=sub, nprobe=nlist))
        for i in range(NQ):
            assert np.array_equal(I[i], want[name][i][1][0]) and np.array_equal(D[i], want[name][i][0][0]), (name, i)
    a.close()  # destroy one and search the other
    assert not a.valid and b.valid
    with pytest.raises(ValueError, match="closed"):
        ivf.search(q, 20, params=a)
    a.close()  # twice is fine
    D, I = ivf.search(q, 20, params=SearchParametersIVF(sel=b, nprobe=nlist))
    assert all(np.array_equal(I[i], want["b"][i][1][0]) for i in range(NQ))
    lib = native.load()
    D1, I1 = np.empty((1, 20), np.float32), np.empty((1, 20), np.int64)
    for bad in (0, -1, 1, 12345):  # 1 was a's id: ids are not reused
        assert bad != b.id
        assert lib.ls_ivf_search_subset(ivf._handle, bad, q.ctypes.data, 1, 20, 4, 0, D1.ctypes.data,
                                        I1.ctypes.data) == native.LS_ERR_INVALID_ARG
        assert lib.ls_ivf_subset_destroy(ivf._handle, bad) == native.LS_ERR_INVALID_ARG
    assert lib.ls_ivf_search_subset(ivf._handle, b.id, q.ctypes.data, 1, 20, 0, 0, D1.ctypes.data,
                                    I1.ctypes.data) == native.LS_ERR_INVALID_ARG  # nprobe = 0
    assert lib.ls_ivf_search_subset(ivf._handle, b.id, q.ctypes.data, 1, 20, 4, 2, D1.ctypes.data,
                                    I1.ctypes.data) == native.LS_ERR_INVALID_ARG  # a flag other than NORMALIZE
    assert lib.ls_ivf_search_subset(ivf._handle, b.id, None, 0, 20, 4, 0, None, None) == native.LS_OK  # nq = 0
    with pytest.raises(ValueError, match="another index"):
        other.search(q, 20, params=b)
    # a subset with no row in the probed lists, and the empty subset: all padding
    lone = ivf.subset(np.array([17]))
    _, P = ivf.quantizer.search(q, 1)
    away = np.flatnonzero(P[:, 0] != ivf.assignment()[17])
    assert away.size
    D, I = ivf.search(q[away], 5, params=SearchParametersIVF(sel=lone, nprobe=1))
    assert (I == -1).all() and (D == NEG).all()
    D, I = ivf.search(q, 5, params=SearchParametersIVF(sel=lone, nprobe=nlist))
    assert (I[:, 0] == 17).all() and (I[:, 1:] == -1).all() and (D[:, 1:] == NEG).all()
    none = ivf.subset(np.zeros(n, bool))
    D, I = ivf.search(q, 5, params=SearchParametersIVF(sel=none, nprobe=nlist))
    assert none.rows == 0 and (I == -1).all() and (D == NEG).all()
    # a short bitmap, and bits past ntotal
    short = ivf.subset(IDSelectorBitmap(np.full(100, 0xFF, np.uint8)))
    long_ = ivf.subset(IDSelectorBitmap(np.full((n + 7) // 8 + 3, 0xFF, np.uint8)))
    assert short.rows == 800 and long_.rows == n
    D, I = ivf.search(q, 900, params=SearchParametersIVF(sel=short, nprobe=nlist))
    assert all(sorted(I[i, :800].tolist()) == list(range(800)) for i in range(NQ)) and (I[:, 800:] == -1).all()
    ivf.close()  # frees the subsets with the handle
    assert not b.valid and not lone.valid
    with pytest.raises(ValueError, match="closed"):
        ivf.search(q, 20, params=b)
    b.close()
    for ix in (flat, other):
        ix.close()


# ---- (h) ----------------------------------------------------------------------------------------------------------------
def test_k_too_large_follows_the_selected_rows():
    corpus, flat, ivf = small_pair()
    n, nlist = corpus.shape[0], ivf.nlist
    q = queries(35, corpus)
    K = native.LS_MAX_K
    with pytest.raises(native.LeanSearchError) as e:  # the unfiltered search: min(k, ntotal)
        ivf.search(q, K + 1)
    assert e.value.code == native.LS_ERR_K_TOO_LARGE
    big, ones = ivf.subset(np.arange(K + 1)), ivf.subset(np.ones(n, bool))
    for sub in (big, ones):
        with pytest.raises(native.LeanSearchError) as e:
            ivf.search(q, K + 1, params=sub)
        assert e.value.code == native.LS_ERR_K_TOO_LARGE and "selected rows" in str(e.value)
        D, I = ivf.search(q, K, params=SearchParametersIVF(sel=sub, nprobe=nlist))  # k = LS_MAX_K is served
        assert (I >= 0).all()
    for m, k in ((K, 3000), (100, 5000), (1, K + 1)):  # m <= LS_MAX_K: any k is served, padded past m
        rows = np.sort(np.random.default_rng(m).choice(n, m, replace=False))
        sub = ivf.subset(rows)
        D, I = ivf.search(q, k, params=SearchParametersIVF(sel=sub, nprobe=nlist))
        for i in range(NQ):
            Df, If = flat.search(q[i:i + 1], k, params=SearchParameters(sel=rows))
            assert np.array_equal(I[i], If[0]) and np.array_equal(D[i], Df[0]), (m, k, i)
        assert (I[:, :m] >= 0).all() and (I[:, m:] == -1).all() and (D[:, m:] == NEG).all()
        sub.close()
    for ix in (flat, ivf):
        ix.close()


# ---- (i) ----------------------------------------------------------------------------------------------------------------
def test_engine_ivf_prefilter(tmp_path):
    """The small database of tests/test_ivf_gpu.py's engine test, every third declaration in a second package."""
    n, d, nlist = 2_000, 96, 160
    corpus, cent = mixture(71, n, d, nlist)
    pkg = np.where(np.arange(n) % 3 == 0, "Std", "Mathlib")
    rows = [(5000 + i, f"{pkg[i]}.decl{i}", f"{pkg[i]}.Mod", "doc", f"theorem t{i}", f"http://x/{i}", None,
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
    qvec = corpus[123] * 3.0 + 0.01 * H.gauss(5, 1, d)[0]  # row 123 is a Std declaration
    kw = dict(base_path=tmp_path, embedding_client=FakeEmbed(qvec), lexical_retriever=False, semantic_index="ivf")
    eng = S.SearchEngine(**kw, ivf_prefilter=True)
    off = S.SearchEngine(**kw)
    k = 200
    sem = run(eng._retrieve_semantic_candidates("q", k, ["Mathlib"]))
    index = eng.faiss_informal_index
    assert isinstance(index, IVFFlatIndex) and index.nprobe == 64
    cached = eng._package_subset(["Mathlib"])
    assert isinstance(cached, IVFSubset) and cached.index is index and eng._package_subset(["Mathlib"]) is cached
    mask = pkg == "Mathlib"
    assert cached.rows == int(mask.sum())
    # the candidates are the IVF subset search of the package mask ...
    x = np.ascontiguousarray(qvec[None, :], dtype=np.float32)
    D, I = index.search_subset(x, k, mask, nprobe=64, normalize=True)
    assert (I[0] >= 0).all() and mask[I[0]].all()
    assert list(sem.items()) == [(ids[r], max(0.0, float(s))) for r, s in zip(I[0].tolist(), D[0].tolist())]
    # ... which is the flat subset search of (probed AND package)
    _, P = coarse.search(x, 64, normalize=True)
    bm = np.packbits(np.isin(assign, P[0]) & mask, bitorder="little")
    flat = FlatIPIndex.from_array(loaded)
    Df, If = flat.search(x, k, normalize=True, params=SearchParameters(sel=IDSelectorBitmap(bm)))
    assert np.array_equal(I, If) and np.array_equal(D, Df)
    res = run(eng.search_prefiltered("q", ["Mathlib"], limit=20, rerank_top=None))
    assert len(res) == 20 and all(r.module.startswith("Mathlib") for r in res)
    resp = run(S.Service(engine=eng).search("q", limit=20, rerank_top=0, packages=["Std"], prefilter_packages=True,
                                            prefilter_lexical=True))  # (no lexical signal: the flag is accepted)
    assert resp.count == 20 and all(r.module.startswith("Std") for r in resp.results) and resp.results[0].id == 5123
    assert len(eng._package_subsets) == 2
    with pytest.raises(ValueError, match="ivf_prefilter"):  # the same engine without the switch still refuses
        run(off.search_prefiltered("q", ["Mathlib"]))
    assert list(run(off._retrieve_semantic_candidates("q", k))) == \
        list(run(eng._retrieve_semantic_candidates("q", k)))  # the unfiltered path is the same with the switch on
    for ix in (coarse, flat):
        ix.close()
