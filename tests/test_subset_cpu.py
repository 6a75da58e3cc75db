"""Row-subset search without a GPU: faiss selector semantics -> bitmap bytes, argument checks, the C ABI's refusal
on a CPU-only host, and the engine's package prefilter on an oracle-backed index that takes ``params``."""

import asyncio
import ctypes
import json
import sqlite3
from types import SimpleNamespace

import numpy as np
import pytest

from lean_explore_amd import faiss_compat as fc
from lean_explore_amd import loader, native
from lean_explore_amd import search as S
from lean_explore_amd.id_selectors import to_bitmap
from lean_explore_amd.index import FlatIPIndex
from oracle import oracle
from tests import helpers as H


def bits(bm, n):
    bm = np.asarray(bm, dtype=np.uint8)
    return [r for r in range(n) if (r >> 3) < bm.size and (bm[r >> 3] >> (r & 7)) & 1]


def test_range_selector_bitmap():
    assert bits(fc.IDSelectorRange(3, 11).bitmap(20), 20) == list(range(3, 11))
    assert bits(fc.IDSelectorRange(-5, 2).bitmap(20), 20) == [0, 1]
    assert bits(fc.IDSelectorRange(15, 99).bitmap(20), 20) == list(range(15, 20))
    assert bits(fc.IDSelectorRange(7, 7).bitmap(20), 20) == []
    bm = fc.IDSelectorRange(0, 9).bitmap(9)
    assert bm.tolist() == [0xFF, 0x01]


def test_batch_selector_bitmap():
    ids = np.array([9, 2, 2, 17, -1, 30, 0], np.int64)  # unsorted, duplicate, negative, out of range
    assert bits(fc.IDSelectorBatch(ids).bitmap(18), 18) == [0, 2, 9, 17]
    assert bits(fc.IDSelectorBatch(3, ids).bitmap(18), 18) == [2, 9]  # swig-style (n, array)
    assert bits(fc.IDSelectorBatch(np.array([], np.int64)).bitmap(5), 5) == []
    assert to_bitmap(fc.IDSelectorBatch([1, 8]), 9).tolist() == [0x02, 0x01]


def test_bitmap_selector_faiss_bit_order():
    raw = np.array([0b10000001, 0b00000100], np.uint8)
    sel = fc.IDSelectorBitmap(raw)
    assert bits(sel.bitmap(16), 16) == [0, 7, 10]
    assert bits(fc.IDSelectorBitmap(1, raw).bitmap(16), 16) == [0, 7]  # (n bytes, array): short bitmap
    long = np.full(8, 0xFF, np.uint8)  # bits past ntotal are left for the library to ignore
    assert to_bitmap(fc.IDSelectorBitmap(long), 5).tolist() == [0xFF] * 8


def test_masks_and_id_arrays():
    m = np.zeros(11, bool)
    m[[0, 5, 10]] = True
    assert bits(to_bitmap(m, 11), 11) == [0, 5, 10]
    assert bits(to_bitmap(np.array([10, 0, 5, 5]), 11), 11) == [0, 5, 10]
    p = fc.SearchParametersIVF(sel=fc.IDSelectorRange(1, 2), nprobe=64)
    assert p.nprobe == 64 and isinstance(p.sel, fc.IDSelectorRange)
    assert fc.SearchParameters().sel is None


def test_bad_selector_arguments():
    with pytest.raises(ValueError):
        to_bitmap(np.zeros(4, bool), 5)  # mask of the wrong length
    with pytest.raises(ValueError):
        to_bitmap(np.array([0.5, 1.0]), 5)
    with pytest.raises(ValueError):
        fc.IDSelectorBitmap(np.array([1, 2], np.int32))
    with pytest.raises(ValueError):
        fc.IDSelectorBatch(np.array([0.5]))
    with pytest.raises(ValueError):
        fc.IDSelectorBatch(5, np.array([1, 2]))
    with pytest.raises(ValueError):
        fc.IDSelectorBitmap(1, 2, 3)


def test_subset_abi_refuses_without_device(gpu_available):
    if gpu_available:
        pytest.skip("a GPU is visible; the refusal path is for CPU-only hosts")
    lib = native.load()
    sid, rows = ctypes.c_int32(), ctypes.c_int64()
    bm = (ctypes.c_uint8 * 1)(0xFF)
    h = ctypes.c_void_p()
    rc = lib.ls_create(ctypes.byref(h), None, 0, 8, 0, 0)
    assert rc == native.LS_ERR_NO_DEVICE
    ix = FlatIPIndex(8)
    ix.add(np.ones((3, 8), np.float32))
    with pytest.raises(native.LeanSearchError) as e:
        ix.subset(np.array([0, 2]))
    assert e.value.code == native.LS_ERR_NO_DEVICE
    with pytest.raises(native.LeanSearchError):
        ix.search(np.ones((1, 8), np.float32), 2, params=fc.SearchParameters(sel=fc.IDSelectorRange(0, 2)))
    assert lib.ls_subset_create(None, bm, 1, ctypes.byref(sid), ctypes.byref(rows)) == native.LS_ERR_INVALID_ARG
    assert lib.ls_subset_destroy(None, 1) == native.LS_ERR_INVALID_ARG


# ------------------------------------------------------------------ engine glue
class ParamsOracleIndex:
    """CPU stand-in that takes faiss's params=: the selection is a bool mask (no `subset` method)."""

    supports_fused_normalize = True

    def __init__(self, corpus):
        self.corpus, self.ntotal, self.d = corpus, corpus.shape[0], corpus.shape[1]
        self.calls = []

    def search(self, x, k, normalize=False, params=None):
        self.calls.append((k, normalize, params))
        q = oracle.c_normalize_l2(x) if normalize else x
        if params is None or params.sel is None:
            return oracle.c_search(self.corpus, q, k)
        rows = np.nonzero(np.asarray(params.sel))[0]
        D, I = oracle.c_search(self.corpus[rows], q, k)
        return D, np.where(I >= 0, rows[np.maximum(I, 0)], -1)


class SpyIndex(ParamsOracleIndex):
    def search(self, *args, **kwargs):
        self.calls.append(("raw", args[1:], dict(kwargs)))
        return super().search(*args, **kwargs)


class FakeEmbed:
    def __init__(self, vec):
        self.vec = vec

    async def embed(self, texts, is_query=False):
        return SimpleNamespace(embeddings=[list(map(float, self.vec))])


def _make_db(path, rows):
    con = sqlite3.connect(path)
    con.execute("CREATE TABLE declarations (id INTEGER PRIMARY KEY, name TEXT, module TEXT, "
                "docstring TEXT, source_text TEXT, source_link TEXT, dependencies TEXT, "
                "informalization TEXT, informalization_embedding BLOB)")
    con.executemany("INSERT INTO declarations VALUES (?,?,?,?,?,?,?,?,?)", rows)
    con.commit()
    con.close()


def _engine(tmp_path, index_cls, n=60, d=32, small_every=6):
    """Package "Small" owns every `small_every`-th row, "Big" the rest; the query sits near a Big row."""
    corpus = H.gauss(11, n, d)
    rows = []
    for i in range(n):
        pkg = "Small" if i % small_every == 0 else "Big"
        rows.append((2000 + i, f"{pkg}.decl{i}", f"{pkg}.Mod", None, f"def d{i}", f"http://x/{i}", None,
                     f"informal {i}", loader.embedding_to_blob(corpus[i].tolist())))
    db = tmp_path / "lean_explore.db"
    _make_db(db, rows)
    ids, loaded = loader.load_corpus_from_sqlite(db)
    ids = list(ids) + [999999]  # a row whose id is not in the database: never selected
    loaded = np.concatenate([loaded, corpus[1:2]], axis=0)
    index = index_cls(loaded)
    eng = S.SearchEngine(db_path=db, embedding_client=FakeEmbed(corpus[1] * 2.0), index=index, ids_map=ids,
                         lexical_retriever=False)
    return eng, index, loaded, ids


def test_prefilter_dense_candidates_are_the_package_top_k(tmp_path):
    eng, index, corpus, ids = _engine(tmp_path, ParamsOracleIndex)
    faiss_k = 4
    sem = asyncio.run(eng._retrieve_semantic_candidates("q", faiss_k, ["Small"]))
    rows = np.array([r for r, i in enumerate(ids) if i != 999999 and (i - 2000) % 6 == 0])
    q = oracle.c_normalize_l2(np.array([eng.embedding_client.vec], np.float32))
    D, I = oracle.c_search(corpus[rows], q, faiss_k)
    want = [ids[rows[j]] for j in I[0] if j >= 0]
    assert list(sem) == want
    assert np.allclose([sem[w] for w in want], np.maximum(D[0][: len(want)], 0.0))


def test_prefilter_returns_limit_where_the_post_filter_does_not(tmp_path):
    eng, _, _, _ = _engine(tmp_path, ParamsOracleIndex)
    post = asyncio.run(eng.search("q", limit=5, faiss_k=5, rerank_top=None, packages=["Small"]))
    pre = asyncio.run(eng.search_prefiltered("q", ["Small"], limit=5, faiss_k=5, rerank_top=None))
    assert len(post) < 5 and len(pre) == 5
    assert all(r.module.startswith("Small") for r in pre)
    svc = S.Service(engine=eng)
    resp = asyncio.run(svc.search("q", limit=5, rerank_top=None, packages=["Small"], prefilter_packages=True))
    assert resp.count == 5


def test_flag_off_calls_the_index_exactly_as_before(tmp_path):
    eng, index, _, _ = _engine(tmp_path, SpyIndex)
    asyncio.run(eng.search("q", limit=5, faiss_k=7, rerank_top=None, packages=["Small"]))
    asyncio.run(eng.search("q", limit=5, faiss_k=7, rerank_top=None))
    raw = [c for c in index.calls if c[0] == "raw"]
    assert raw and all(c[2] == {"normalize": True} and c[1] == (7,) for c in raw)
    svc = S.Service(engine=eng)
    asyncio.run(svc.search("q", limit=5, rerank_top=None, packages=["Small"]))
    raw = [c for c in index.calls if c[0] == "raw"]
    assert raw[-1][2] == {"normalize": True} and raw[-1][1] == (1000,)
    asyncio.run(eng.search_prefiltered("q", ["Small"], limit=5, faiss_k=7, rerank_top=None))
    last = [c for c in index.calls if c[0] == "raw"][-1]
    assert set(last[2]) == {"normalize", "params"}


def test_prefilter_needs_an_index_that_takes_params(tmp_path):
    class NoParams(ParamsOracleIndex):
        def search(self, x, k, normalize=False):
            return super().search(x, k, normalize)

    eng, _, _, _ = _engine(tmp_path, NoParams)
    with pytest.raises(TypeError):
        asyncio.run(eng.search_prefiltered("q", ["Small"], limit=5, faiss_k=5, rerank_top=None))
