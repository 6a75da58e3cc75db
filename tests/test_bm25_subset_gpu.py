"""BM25 over a document subset on the GPU (csrc/ls_bm25.hip `bm25_score_list_kernel`): every
result - scores AND documents - equals the host reference built from oracle.bm25_ref bit for bit; no tolerance anywhere."""

import asyncio
import ctypes

import numpy as np
import pytest

from lean_explore_amd import native
from lean_explore_amd.bm25 import BM25Index, NameRetriever
from lean_explore_amd.search.tokenization import tokenize_raw, tokenize_spaced
from oracle import bm25_ref as R
from tests.test_bm25 import WORDS, synth_names
from tests.test_bm25_subset_cpu import ref_subset

pytestmark = pytest.mark.gpu

N = 20_000
LONG_Q = (["nat", "add", "comm", "list", "map", "measure", "theory", "ker"] * 9)[:70]  # chained launches: F[pos]
QUERIES = (["nat", "add", "comm"], ["list", "list", "map"], ["nope"], [], LONG_Q)
KS = (1, 50, 1000, 2048)
MS = (0, 1, 3, 5, 255, 257, 2047, 2305, 4097, 20_000)


def _selections():
    rng = np.random.default_rng(17)
    sel = {}
    for dens in (0.5, 0.1, 0.01):
        sel[f"random{dens}"] = np.nonzero(rng.random(N) < dens)[0]
    sel["every7th"] = np.arange(0, N, 7)
    for m in MS:
        sel[f"first{m}"] = np.arange(m)
        sel[f"last{m}"] = np.arange(N - m, N)
        sel[f"middle{m}"] = np.arange((N - m) // 2, (N - m) // 2 + m)
    return sel


SELECTIONS = _selections()


class Corpus:
    def __init__(self):
        self.corpus = [list(dict.fromkeys(tokenize_spaced(n))) for n in synth_names(N, 3)]
        self.ref = R.build(self.corpus)
        self.ix = BM25Index().index(self.corpus)
        self.scores = [R.scores(self.ref, R.token_ids(self.ref, q)) for q in QUERIES]  # computed once, never written
        for s in self.scores:
            s.setflags(write=False)

    def want(self, qi, rows, k):
        s = self.scores[qi]
        order = np.lexsort((rows, -s[rows].astype(np.float64)))[:k]
        docs = np.full(k, -1, dtype=np.int64)
        out = np.full(k, np.float32(-3.4028234663852886e38), dtype=np.float32)
        docs[: order.size] = rows[order]
        out[: order.size] = s[rows[order]]
        return docs, out


@pytest.fixture(scope="module")
def C():
    c = Corpus()
    yield c
    c.ix.close()


def test_reference_helper_is_the_issues_definition(C):
    rows = SELECTIONS["random0.1"]
    for qi, q in enumerate(QUERIES[:2]):
        d0, s0 = ref_subset(C.ref, q, rows, 100)
        d1, s1 = C.want(qi, rows, 100)
        assert np.array_equal(d0, d1) and np.array_equal(s0, s1)


@pytest.mark.parametrize("name", sorted(SELECTIONS))
def test_subset_retrieve_bit_exact_vs_host_reference(C, name):
    rows = SELECTIONS[name]
    mask = np.zeros(N, dtype=bool)
    mask[rows] = True
    sub = C.ix.subset(mask)
    assert sub.docs == rows.size and sub.valid
    for qi, q in enumerate(QUERIES):
        for k in KS:
            docs, sc = C.ix.retrieve(q, k, subset=sub)
            dref, sref = C.want(qi, rows, k)
            assert np.array_equal(sc, sref), (name, qi, k)
            assert np.array_equal(docs, dref), (name, qi, k)
    # k past LS_MAX_K: an error only when the subset has more than LS_MAX_K documents, else padding
    if rows.size > native.LS_MAX_K:
        with pytest.raises(native.LeanSearchError) as e:
            C.ix.retrieve(QUERIES[0], 3000, subset=sub)
        assert e.value.code == native.LS_ERR_K_TOO_LARGE
        with pytest.raises(native.LeanSearchError) as e:
            C.ix.retrieve(["nope"], 3000, subset=sub)  # (the k rule comes before the no-posting shortcut)
        assert e.value.code == native.LS_ERR_K_TOO_LARGE
    else:
        for qi in (0, 2):
            docs, sc = C.ix.retrieve(QUERIES[qi], 3000, subset=sub)
            dref, sref = C.want(qi, rows, 3000)
            assert np.array_equal(sc, sref) and np.array_equal(docs, dref), (name, qi)
    sub.close()
    assert not sub.valid


def test_selection_forms_agree(C):
    """A bool mask, an int array (unsorted, duplicated, out of range), a selector and a long / short bitmap."""
    from lean_explore_amd.id_selectors import IDSelectorBitmap, IDSelectorRange

    rows = SELECTIONS["random0.01"]
    want = C.want(0, rows, 50)
    shuffled = np.concatenate([rows[::-1], rows[:5], [-3, N, N + 9]])
    for sel in (shuffled, IDSelectorBitmap(np.packbits(np.isin(np.arange(N + 64), rows), bitorder="little"))):
        sub = C.ix.subset(sel)
        assert sub.docs == rows.size
        docs, sc = C.ix.retrieve(QUERIES[0], 50, subset=sub)
        assert np.array_equal(docs, want[0]) and np.array_equal(sc, want[1])
    sub = C.ix.subset(IDSelectorRange(100, 357))
    assert sub.docs == 257
    docs, sc = C.ix.retrieve(QUERIES[0], 300, subset=sub)
    dref, sref = C.want(0, np.arange(100, 357), 300)
    assert np.array_equal(docs, dref) and np.array_equal(sc, sref)
    # bits past n_docs are ignored; documents past a short bitmap are not selected
    sub = C.ix.subset(IDSelectorBitmap(np.full(N // 8 + 40, 0xFF, np.uint8)))
    assert sub.docs == N
    sub = C.ix.subset(IDSelectorBitmap(np.full(13, 0xFF, np.uint8)))
    assert sub.docs == 104
    docs, sc = C.ix.retrieve(QUERIES[1], 200, subset=sub)
    dref, sref = C.want(1, np.arange(104), 200)
    assert np.array_equal(docs, dref) and np.array_equal(sc, sref)


def test_all_ones_subset_equals_plain_retrieve(C):
    sub = C.ix.subset(np.ones(N, dtype=bool))
    for q in QUERIES:
        for k in KS:
            d0, s0 = C.ix.retrieve(q, k)
            d1, s1 = C.ix.retrieve(q, k, subset=sub)
            assert np.array_equal(d0, d1) and np.array_equal(s0, s1), (q[:3], k)


def test_plain_retrieve_between_subset_calls(C):
    """The subset path shares F and the candidate buffers with the plain one."""
    rows = SELECTIONS["random0.1"]
    sub = C.ix.subset(rows)
    for qi, k in ((0, 1000), (4, 300)):
        d1, s1 = C.ix.retrieve(QUERIES[qi], k, subset=sub)
        d0, s0 = C.ix.retrieve(QUERIES[qi], k)
        d2, s2 = C.ix.retrieve(QUERIES[qi], k, subset=sub)
        dref, sref = R.retrieve(C.ref, QUERIES[qi], k)
        assert np.array_equal(d0, dref) and np.array_equal(s0, sref)
        want = C.want(qi, rows, k)
        for d, s in ((d1, s1), (d2, s2)):
            assert np.array_equal(d, want[0]) and np.array_equal(s, want[1])


def test_fat_documents_subset():
    """Documents with more tokens than the 8 entries a lane keeps in registers (the tail loop), a random half."""
    rng = np.random.default_rng(5)
    fat = [list(dict.fromkeys(WORDS[j] for j in rng.integers(0, len(WORDS), size=rng.integers(1, 40))))
           for _ in range(5000)]
    fx, fref = BM25Index().index(fat), R.build(fat)
    rows = np.nonzero(rng.random(5000) < 0.5)[0]
    sub = fx.subset(rows)
    for q in (WORDS[:5], [WORDS[3]] * 3 + WORDS[10:14]):
        docs, sc = fx.retrieve(q, 500, subset=sub)
        dref, sref = ref_subset(fref, q, rows, 500)
        assert np.array_equal(sc, sref) and np.array_equal(docs, dref), q
    fx.close()


def test_subset_lifecycle(C):
    lib = native.load()
    sub = C.ix.subset(np.arange(10))
    other = BM25Index().index(C.corpus[:100])
    osub = other.subset(np.arange(10))
    with pytest.raises(ValueError):
        C.ix.retrieve(["nat"], 5, subset=osub)  # a subset of another index
    with pytest.raises(ValueError):
        other.retrieve(["nat"], 5, subset=sub)
    docs, _ = other.retrieve(["nat"], 5, subset=osub)
    assert (docs >= 0).all() and (docs < 10).all()
    sid = sub.id
    sub.close()
    with pytest.raises(ValueError):
        C.ix.retrieve(["nat"], 5, subset=sub)  # closed
    sub.close()  # closing twice is fine
    assert lib.ls_bm25_subset_destroy(C.ix._ensure(), sid) == native.LS_ERR_INVALID_ARG  # already gone
    assert lib.ls_bm25_subset_destroy(C.ix._ensure(), 123456) == native.LS_ERR_INVALID_ARG
    assert b"no subset" in lib.ls_last_error()
    out_s, out_d = np.empty(5, np.float32), np.empty(5, np.int64)
    tok = np.zeros(1, np.int32)
    assert lib.ls_bm25_search_subset(C.ix._ensure(), 123456, native.addr(tok), 1, 5, native.addr(out_s),
                                     native.addr(out_d)) == native.LS_ERR_INVALID_ARG
    live = C.ix.subset(np.arange(10))
    bad = np.array([len(C.ix.vocab)], np.int32)
    assert lib.ls_bm25_search_subset(C.ix._ensure(), live.id, native.addr(bad), 1, 5, native.addr(out_s),
                                     native.addr(out_d)) == native.LS_ERR_INVALID_ARG
    assert lib.ls_bm25_search_subset(C.ix._ensure(), live.id, native.addr(tok), 1, 0, native.addr(out_s),
                                     native.addr(out_d)) == native.LS_ERR_INVALID_ARG
    # a subset does not survive its handle: index() rebuilds it, close() drops it
    other.index(C.corpus[:100])
    assert not osub.valid
    with pytest.raises(ValueError):
        other.retrieve(["nat"], 5, subset=osub)
    osub2 = other.subset(np.arange(10))
    other.close()
    assert not osub2.valid
    with pytest.raises(ValueError):
        other.retrieve(["nat"], 5, subset=osub2)
    osub2.close()


def _merge_reference(names, ids, query, rows, k):
    want = {}
    for tok in (tokenize_spaced, tokenize_raw):
        ref = R.build([list(dict.fromkeys(tok(n))) for n in names])
        docs, sc = ref_subset(ref, tok(query), rows, min(k, max(1, rows.size)))
        for d, s in zip(docs.tolist(), sc.tolist()):
            if d >= 0:
                want[ids[d]] = max(want.get(ids[d], 0.0), float(s))
    return want


def test_name_retriever_subset_max_merge():
    n = 3000
    names = [f"{'Small' if i % 10 == 0 else 'Big'}.{name}" for i, name in enumerate(synth_names(n, 4))]
    ids = [10_000 + i for i in range(n)]
    nr = NameRetriever.from_names(ids, names)
    mask = np.arange(n) % 10 == 0
    sub = nr.subset(mask)
    assert sub.docs == 300 and sub.valid
    for q in (names[1230], "nat add comm", names[7]):  # (names[7] is a Big name: the raw index finds nothing selected)
        got = nr(q, 1000, subset=sub)
        assert got == _merge_reference(names, ids, q, np.nonzero(mask)[0], 1000), q
        assert set(got) <= {ids[i] for i in range(0, n, 10)}
    assert nr("nat add comm", 1000) == _merge_reference(names, ids, "nat add comm", np.arange(n), 1000)
    other = NameRetriever.from_names(ids[:50], names[:50])
    with pytest.raises(ValueError):
        other("nat", 10, subset=sub)
    sub.close()
    assert not sub.valid


def test_service_prefilters_both_stages_on_the_gpu(tmp_path):
    """Service.search(packages=["Small"], prefilter_packages=True, prefilter_lexical=True) on a FlatIPIndex and a
    NameRetriever: `limit` results, all in Small; the lexical candidates are the package's names."""
    from lean_explore_amd import loader
    from lean_explore_amd import search as S
    from lean_explore_amd.index import FlatIPIndex
    from tests import helpers as H
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
    names = [r[1] for r in rows]
    nr = NameRetriever.from_names([r[0] for r in rows], names)
    eng = S.SearchEngine(db_path=db, embedding_client=FakeEmbed(corpus[1] * 3.0), index=ix, ids_map=ids,
                         lexical_retriever=nr)
    query = "Small decl120"
    small = np.arange(0, n, 10)
    got = eng._retrieve_bm25_candidates(query, 1000, ["Small"])
    assert got == _merge_reference(names, [r[0] for r in rows], query, small, 1000)
    assert len(got) == 300
    resp = asyncio.run(S.Service(engine=eng).search(query, limit=10, rerank_top=None, packages=["Small"],
                                                    prefilter_packages=True, prefilter_lexical=True))
    assert resp.count == 10 and all(r.module.startswith("Small") for r in resp.results)
    assert len(eng._lexical_subsets) == 1  # the second call reused the cached subset
    ix.close()
