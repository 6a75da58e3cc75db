"""The sq8 storage dtype on the GPU (include/leansearch_sq8.h). Everything is pinned bit for bit
(np.array_equal) against the host restatements: lean_explore_amd/sq8.py for the codes, tests/sq8_ref.c for the scores."""

import ctypes
import threading

import numpy as np
import pytest

from lean_explore_amd import faiss_compat, loader, native, sq8
from lean_explore_amd import search as S
from lean_explore_amd.id_selectors import IDSelectorBitmap, SearchParameters
from lean_explore_amd.index import FlatIPIndex, normalize_L2
from lean_explore_amd.ivf import IVFFlatIndex
from tests.test_glue_cpu import FakeEmbed, _make_db, run
from tests.test_ivf_gpu import mixture, queries, subset_reference
from tests.test_sq8_cpu import (NEG, QUALITY, exact_topk, geom, padded_codes, quality_data, recall_at, ref_scores)

pytestmark = pytest.mark.gpu


class Case:
    """A corpus, its sq8 index and the restatement's scores of 16 queries, computed once per shape."""

    def __init__(self, n, d, nlist=64):
        self.n, self.d = n, d
        self.corpus, self.cent = mixture(1000 + n + d, n, d, nlist)
        self.q = queries(77 + d, self.corpus)
        self.step = sq8.train_step(self.corpus)
        self.codes = sq8.encode(self.corpus, self.step)
        rc, self.g = geom(d)
        assert rc == 0
        self.cp = padded_codes(self.codes, self.g[0])
        self.ix = FlatIPIndex.from_array(self.corpus, dtype="sq8")
        self._ref = {}

    def qprime(self, normalize):
        q = self.q.copy()
        if normalize:
            normalize_L2(q)
        return q * self.step  # float32: the second of the two rounded multiplies

    def ref(self, normalize):
        if normalize not in self._ref:
            self._ref[normalize] = ref_scores(self.cp, self.g, self.qprime(normalize))
        return self._ref[normalize]


_cases = {}


def case(n, d, nlist=64):
    if (n, d) not in _cases:
        _cases[(n, d)] = Case(n, d, nlist)
    return _cases[(n, d)]


def assert_topk(D, I, scores, k, rows=None):
    for i in range(scores.shape[0]):
        Dr, Ir = exact_topk(scores[i], k, rows)
        assert np.array_equal(I[i], Ir), f"query {i}: rows differ"
        assert np.array_equal(D[i], Dr), f"query {i}: scores differ"


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, d, dirty", [(5_000, 100, True), (3_000, 384, False)])
def test_codes_step_and_reconstruct(n, d, dirty):
    x, _ = mixture(3 + d, n, d, 16)
    if dirty:
        x[:, 7] = 0.0
        x[11, 3], x[12, 4], x[13, 5], x[14, 99] = np.nan, np.inf, -np.inf, np.nan
    ix = FlatIPIndex.from_array(x, dtype="sq8")
    step = sq8.train_step(x)
    assert np.array_equal(ix.sq8_step, step)
    codes = sq8.encode(x, step)
    assert np.array_equal(ix.codes(), codes)
    assert np.array_equal(ix.codes(100, 17), codes[100:117])
    assert np.array_equal(ix.host_corpus(), sq8.decode(codes, step))
    assert ix.storage_dtype == "sq8" and native.load().ls_dtype(ix._handle) == native.LS_DTYPE_SQ8
    ix.close()
    import torch

    dev = FlatIPIndex.from_device_tensor(torch.from_numpy(x).cuda(), dtype="sq8")
    assert np.array_equal(dev.sq8_step, step) and np.array_equal(dev.codes(), codes)
    dev.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------
ZERO_EXCUSE = [(5_000, 64, 10), (5_000, 100, 10), (20_000, 384, 50), (6_000, 768, 50), (4_000, 1024, 1000),
               (3_000, 2048, 10), (200_000, 384, 50)]
# (by the launch rule of ls_scan_launch the d = 64 / 100 / 384 rows run the kernel that is not SMALL - their tiles hold
# 32 or 64 rows, so four tiles per wave pass 64 rows - and d = 768 / 1024 / 2048 run the SMALL one; both variants of
# every geometry: tests/test_geometry_gpu.py)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("n, d, k", ZERO_EXCUSE)
def test_zero_excuse(n, d, k, normalize):
    c = case(n, d)
    D, I = c.ix.search(c.q, k, normalize=normalize)
    assert c.ix.debug_counter(23) == 0 and c.ix.debug_counter(34) == 0  # never ls_mq / ls_mq16
    assert_topk(D, I, c.ref(normalize), k)
    for i in (0, 7, 15):  # a query's bits do not depend on its company
        D1, I1 = c.ix.search(c.q[i:i + 1], k, normalize=normalize)
        assert np.array_equal(D1[0], D[i]) and np.array_equal(I1[0], I[i])


def test_zero_excuse_alone_and_padding():
    c = case(5_000, 100)
    D, I = c.ix.search(c.q, 10, normalize=True)
    for i in range(16):
        D1, I1 = c.ix.search(c.q[i:i + 1], 10, normalize=True)
        assert np.array_equal(D1[0], D[i]) and np.array_equal(I1[0], I[i])
    small = FlatIPIndex.from_array(c.corpus[:37], dtype="sq8", sq8_step=c.step)
    Dp, Ip = small.search(c.q, 50, normalize=True)
    assert_topk(Dp, Ip, c.ref(True)[:, :37], 50)
    assert (Ip[:, 37:] == -1).all() and (Dp[:, 37:] == NEG).all() and (Ip[:, :37] >= 0).all()
    small.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def test_integer_identity_with_the_fp32_index():
    n, d, k = 20_000, 384, 50
    rng = np.random.default_rng(42)
    base = rng.integers(-127, 128, size=(400, d)).astype(np.float32)
    corpus = base[rng.integers(0, 400, size=n)]  # thousands of exact ties
    q = rng.integers(-8, 9, size=(16, d)).astype(np.float32)
    s8 = FlatIPIndex.from_array(corpus, dtype="sq8", sq8_step=np.ones(d, np.float32))
    f32 = FlatIPIndex.from_array(corpus, dtype="f32")
    assert np.array_equal(s8.codes().astype(np.float32), corpus)
    D8, I8 = s8.search(q, k)
    D32, I32 = f32.search(q, k)
    assert np.array_equal(I8, I32) and np.array_equal(D8, D32)
    assert (np.diff(D8, axis=1) == 0).sum() > 100  # the ties are really there
    s8.close()
    f32.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def test_entry_points_agree():
    import torch

    c = case(20_000, 384)
    k = 50
    D, I = c.ix.search(c.q, k, normalize=True)
    tq = torch.from_numpy(c.q).cuda()
    for kw in ({}, {"asynchronous": True}):
        s, i = c.ix.search_device(tq, k, normalize=True, **kw)
        torch.cuda.synchronize()
        assert np.array_equal(s.cpu().numpy(), D) and np.array_equal(i.cpu().numpy(), I), kw
    c.ix.debug_option(24, 2)  # the scan lanes whatever the corpus size
    outs = []
    for step in range(20):
        j = step % 16
        outs.append((j, c.ix.search_device(tq[j:j + 1], k, normalize=True, pipeline=True)))
    c.ix.check()
    for j, (s, i) in outs:
        assert np.array_equal(s.cpu().numpy()[0], D[j]) and np.array_equal(i.cpu().numpy()[0], I[j]), j
    c.ix.debug_option(24, 1)
    s, i = c.ix.search_device(tq, k, normalize=True, pipeline=True)  # 16 queries in one pipelined call
    c.ix.check()
    assert np.array_equal(s.cpu().numpy(), D) and np.array_equal(i.cpu().numpy(), I)
    # 8 concurrent callers: the combining queue serves them together, every one as alone
    got = [None] * 8
    gate = threading.Barrier(8)

    def caller(t):
        gate.wait()
        got[t] = [c.ix.search(c.q[j:j + 1], k, normalize=True) for j in (t, t + 8, t)]

    th = [threading.Thread(target=caller, args=(t,)) for t in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for t in range(8):
        for (Dt, It), j in zip(got[t], (t, t + 8, t)):
            assert np.array_equal(Dt[0], D[j]) and np.array_equal(It[0], I[j])
    assert c.ix.debug_counter(23) == 0 and c.ix.debug_counter(34) == 0
    D40, I40 = c.ix.search(np.concatenate([c.q, c.q, c.q[:8]]), k, normalize=True)  # past one combining pass
    assert np.array_equal(D40[:16], D) and np.array_equal(I40[32:], I[:8]) and np.array_equal(D40[16:32], D)


# ---- 5 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, d, k", [(5_000, 64, 10), (20_000, 384, 50), (4_000, 1024, 100)])
def test_subset(n, d, k):
    c = case(n, d)
    D, I = c.ix.search(c.q, k, normalize=True)
    ones = np.ones(n, bool)
    Ds, Is = c.ix.search(c.q, k, normalize=True, params=SearchParameters(sel=ones))
    assert np.array_equal(Ds, D) and np.array_equal(Is, I)
    mask = np.random.default_rng(9).random(n) < 0.10
    Dm, Im = c.ix.search(c.q, k, normalize=True, params=SearchParameters(sel=mask))
    rows = np.flatnonzero(mask)
    assert_topk(Dm, Im, c.ref(True)[:, rows], k, rows)


# ---- 6 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, d, nlist, k", [(5_000, 64, 64, 10), (20_000, 384, 141, 50)])
def test_ivf(n, d, nlist, k):
    corpus, cent = mixture(1000 + n + d, n, d, nlist)
    q = queries(77 + d, corpus)
    flat = FlatIPIndex.from_array(corpus, dtype="sq8")
    ivf = IVFFlatIndex(d, nlist, dtype="sq8")
    ivf.set_centroids(cent)
    ivf.add(corpus)
    assign = ivf.assignment()
    coarse = FlatIPIndex.from_array(cent)
    for normalize in (False, True):
        ivf.nprobe = nlist
        D, I = ivf.search(q, k, normalize=normalize)
        Df, If = flat.search(q, k, normalize=normalize)
        assert np.array_equal(I, If) and np.array_equal(D, Df)
    ivf.nprobe = 7
    D, I = ivf.search(q, k, normalize=True)
    Dr, Ir, masks = subset_reference(flat, coarse, assign, q, k, 7, True)
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
    assert all(m.sum() < n for m in masks)
    for ix in (flat, ivf, coarse):
        ix.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_add_encodes_with_the_handles_step():
    c = case(5_000, 100)
    x = c.corpus.copy()
    x[4_000:4_010] *= 40.0  # beyond +-127 * step: clamped
    x[4_020, 5] = np.nan
    whole = FlatIPIndex.from_array(x, dtype="sq8", sq8_step=c.step)
    grown = FlatIPIndex.from_array(x[:2_500], dtype="sq8", sq8_step=c.step)
    grown.add(x[2_500:])
    assert grown.ntotal == whole.ntotal == 5_000
    assert np.array_equal(grown.sq8_step, c.step)
    codes = sq8.encode(x, c.step)
    assert (np.abs(codes[4_000:4_010]) == 127).any()
    assert np.array_equal(grown.codes(), codes) and np.array_equal(whole.codes(), codes)
    for normalize in (False, True):
        Dg, Ig = grown.search(c.q, 20, normalize=normalize)
        Dw, Iw = whole.search(c.q, 20, normalize=normalize)
        assert np.array_equal(Dg, Dw) and np.array_equal(Ig, Iw)
    trained = FlatIPIndex.from_array(x[:2_500], dtype="sq8")  # the step stays the one trained at creation
    s0 = trained.sq8_step
    trained.add(x[2_500:])
    assert np.array_equal(trained.sq8_step, s0) and np.array_equal(s0, sq8.train_step(x[:2_500]))
    for ix in (whole, grown, trained):
        ix.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, d, nlist, k, floor", QUALITY)
def test_quality_against_the_fp32_index(n, d, nlist, k, floor):
    corpus, _, q = quality_data(n, d, nlist)
    s8 = FlatIPIndex.from_array(corpus, dtype="sq8")
    f32 = FlatIPIndex.from_array(corpus, dtype="f32")
    D8, I8 = s8.search(q, k)
    D32, I32 = f32.search(q, k)
    rec = recall_at(I8, I32)
    both = I8[:, :1] == I32[:, :1]
    dmax = float(np.abs(D8[:, 0] - D32[:, 0]).max())
    print(f"sq8 vs f32 on the GPU n={n} d={d}: recall@{k} {rec:.4f}  top-1 equal {int(both.sum())}/64  max |dscore| {dmax:.2e}")
    assert rec >= floor
    assert both.all()
    assert dmax <= 1e-2
    s8.close()
    f32.close()


# ---- 9 ------------------------------------------------------------------------------------------------------------------
def test_refusals_with_a_device_present():
    lib = native.load()
    x = np.ones((64, 8), np.float32)
    ids = (ctypes.c_int32 * 2)(0, 0)
    h = ctypes.c_void_p()
    for fn in (lib.ls_create_sharded, lib.ls_create_replicated):
        assert fn(ctypes.byref(h), x.ctypes.data, 64, 8, native.LS_DTYPE_SQ8, ids, 2) == native.LS_ERR_INVALID_ARG
        assert not h.value
    ix = FlatIPIndex.from_array(x, dtype="sq8")
    assert lib.ls_set_f16_small_batch(ix._handle, 1) == native.LS_ERR_INVALID_ARG
    assert b"sq8" in lib.ls_last_error()
    f32 = FlatIPIndex.from_array(x, dtype="f32")
    out = np.empty(8, np.float32)
    assert lib.ls_sq8_step(f32._handle, out.ctypes.data) == native.LS_ERR_INVALID_ARG  # not an sq8 handle
    ix.close()
    f32.close()


# ---- 10 -----------------------------------------------------------------------------------------------------------------
def test_search_engine_storage_dtype_sq8(tmp_path):
    n, d = 2_000, 96
    corpus, _ = mixture(71, n, d, 16)
    rows = [(5000 + i, f"Mathlib.decl{i}", "Mathlib.Mod", "doc", f"theorem t{i}", f"http://x/{i}", None,
             f"statement {i}", loader.embedding_to_blob(corpus[i].tolist())) for i in range(n)]
    db = tmp_path / "lean_explore.db"
    _make_db(db, rows)
    ids, loaded = loader.load_corpus_from_sqlite(db)
    loader.save_ids_map(tmp_path / "informalization_faiss_ids_map.json", ids)
    faiss_compat.write_index(FlatIPIndex.from_array(loaded), tmp_path / "informalization_faiss.index")
    qvec = corpus[123] * 3.0
    eng = S.SearchEngine(base_path=tmp_path, embedding_client=FakeEmbed(qvec), lexical_retriever=False,
                         storage_dtype="sq8")
    sem = run(eng._retrieve_semantic_candidates("q", 50))
    assert eng.faiss_informal_index.storage_dtype == "sq8"
    direct = FlatIPIndex.from_array(loaded, dtype="sq8")
    D, I = direct.search(np.ascontiguousarray(qvec[None, :], np.float32), 50, normalize=True)
    assert list(sem) == [ids[r] for r in I[0]] and list(sem)[0] == 5123
    assert [np.float32(v) for v in sem.values()] == [max(s, np.float32(0)) for s in D[0]]
    # lossy write: the decoded rows as a flat file; reading it back as sq8 or as IVF keeps working
    with pytest.raises(ValueError):
        faiss_compat.write_index(direct, tmp_path / "lossy.index")
    faiss_compat.write_index(direct, tmp_path / "lossy.index", allow_lossy=True)
    back = faiss_compat.read_index(tmp_path / "lossy.index", dtype="f32")
    assert np.array_equal(back.host_corpus(), sq8.decode(direct.codes(), direct.sq8_step))
    again = faiss_compat.read_index(tmp_path / "informalization_faiss.index", dtype="sq8")
    assert again.storage_dtype == "sq8" and np.array_equal(again.search(qvec[None, :], 5, normalize=True)[1], I[:, :5])
    for ix in (direct, back, again):
        ix.close()
