"""Small batches on an sq8 index with the opt-in small-batch pass (csrc/ls_mq8.hip, ls_set_sq8_small_batch /
FlatIPIndex(sq8_small_batch=True)): 2..16 queries share ONE pass over the codes on the f32 matrix cores. The contract
is the sq8 scan's, bit for bit: every comparison is np.array_equal against tests/sq8_ref.c or against the scan kernel's
own results. Debug counter 36 counts the launches of the new kernel."""

import threading

import numpy as np
import pytest

from lean_explore_amd import native, sq8
from lean_explore_amd.index import FlatIPIndex
from tests.test_sq8_cpu import NEG, geom, padded_codes, ref_scores
from tests.test_sq8_gpu import Case, assert_topk

pytestmark = pytest.mark.gpu

_cases = {}


def case(n, d):
    """A corpus, its sq8 index (the option ON) and the restatement's scores of its 16 queries, once per shape."""
    if (n, d) not in _cases:
        c = Case(n, d)
        c.ix.set_sq8_small_batch(True)
        _cases[(n, d)] = c
    c = _cases[(n, d)]
    c.ix.set_sq8_small_batch(True)
    return c


def launches(ix):
    return ix.debug_counter(36)


# ---- 1 ------------------------------------------------------------------------------------------------------------------
# every built geometry: (chunks, L, V) of the stored row; n just over the 4096-row threshold, a ragged last 16-row tile
GEOMETRIES = {64: (8, 8, 1), 100: (8, 8, 1), 200: (16, 16, 1), 384: (24, 8, 3), 512: (32, 16, 2), 768: (48, 16, 3),
              1024: (64, 16, 4)}
ZERO_EXCUSE = [(5_000, 64, 10), (5_000, 100, 10), (5_000, 200, 10), (5_000, 384, 50), (4_100, 512, 10),
               (4_100, 768, 50), (4_100, 1024, 100)]
# ... and every geometry at every key-list size: at n = 4100, k = 10 / 30 / 100 select 3 / 5 / 8 keys per lane
# (tests/mq_plan_check.cpp asserts it)
ZERO_EXCUSE += [(4_100, d, k) for d in GEOMETRIES for k in (10, 30, 100) if (4_100, d, k) not in ZERO_EXCUSE]


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("n, d, k", ZERO_EXCUSE)
def test_zero_excuse_every_geometry(n, d, k, normalize):
    assert geom(d) == (native.LS_OK, GEOMETRIES[d])
    c = case(n, d)
    ref = c.ref(normalize)
    for nq in (2, 3, 8, 15, 16):
        before = launches(c.ix)
        D, I = c.ix.search(c.q[:nq], k, normalize=normalize)
        assert launches(c.ix) == before + 1, f"{nq} queries must be one ls_mq8 launch"
        assert_topk(D, I, ref[:nq], k)
    assert c.ix.debug_counter(23) == 0 and c.ix.debug_counter(34) == 0  # never ls_mq / ls_mq16


# ---- 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, d, k", [(5_000, 384, 50), (4_100, 1024, 100)])
def test_same_bits_as_the_scan(n, d, k):
    c = case(n, d)
    c.ix.set_sq8_small_batch(False)
    before = launches(c.ix)
    Doff, Ioff = c.ix.search(c.q, k, normalize=True)
    assert launches(c.ix) == before
    c.ix.set_sq8_small_batch(True)
    Don, Ion = c.ix.search(c.q, k, normalize=True)
    assert launches(c.ix) == before + 1
    assert np.array_equal(Don, Doff) and np.array_equal(Ion, Ioff)
    for i in range(16):  # a lone query stays on the scan kernel
        D1, I1 = c.ix.search(c.q[i:i + 1], k, normalize=True)
        assert np.array_equal(D1[0], Don[i]) and np.array_equal(I1[0], Ion[i]), i
    assert launches(c.ix) == before + 1


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def test_column_and_company_independence():
    c = case(5_000, 384)
    k, d = 50, c.d
    x = c.q[5]
    D1, I1 = c.ix.search(x[None, :], k, normalize=True)
    rng = np.random.default_rng(5)
    zero = np.zeros(d, np.float32)
    dirty = c.q[9].copy()
    dirty[3], dirty[200] = np.nan, np.inf
    for col, seed in ((0, 1), (7, 2), (15, 3)):
        batch = (c.q[rng.permutation(16)] * np.float32(seed)).astype(np.float32)  # different companions every time
        zc, nc = (col + 3) % 16, (col + 9) % 16
        batch[zc], batch[nc], batch[col] = zero, dirty, x
        D, I = c.ix.search(batch, k, normalize=True)
        assert np.array_equal(D[col], D1[0]) and np.array_equal(I[col], I1[0]), col
        assert (I[nc] == -1).all() and (D[nc] == NEG).all()  # the NaN query: no row qualifies
        c.ix.set_sq8_small_batch(False)
        Doff, Ioff = c.ix.search(batch, k, normalize=True)
        c.ix.set_sq8_small_batch(True)
        assert np.array_equal(D, Doff) and np.array_equal(I, Ioff), col
        assert (Ioff[nc] == -1).all() and (Doff[nc] == NEG).all()
        assert (D[zc] == 0).all() and np.array_equal(I[zc], np.arange(k))  # the zero query: every score 0, rows in order


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def test_more_than_one_pass():
    c = case(5_000, 384)
    k = 50
    D, I = c.ix.search(c.q, k, normalize=True)
    q40 = np.concatenate([c.q, c.q, c.q[:8]])
    # 16 + 1 (the lone rest stays on the scan kernel), 16 + 16, 16 + 16 + 8
    for nq, passes in ((17, 1), (32, 2), (40, 3)):
        before = launches(c.ix)
        Dn, In = c.ix.search(q40[:nq], k, normalize=True)
        assert launches(c.ix) == before + passes, nq
        for b0 in range(0, nq, 16):
            m = min(16, nq - b0)
            assert np.array_equal(Dn[b0:b0 + m], D[:m]) and np.array_equal(In[b0:b0 + m], I[:m]), (nq, b0)


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def test_padding_rows_are_never_returned():
    n, d, k = 4_101, 64, 50  # the last tile holds 5 rows; 11 zero pad rows score 0, above every true score
    rng = np.random.default_rng(11)
    corpus = (rng.random((n, d), dtype=np.float32) + np.float32(0.1))
    q = -(rng.random((16, d), dtype=np.float32) + np.float32(0.1))
    step = sq8.train_step(corpus)
    codes = sq8.encode(corpus, step)
    rc, g = geom(d)
    scores = ref_scores(padded_codes(codes, g[0]), g, q * step)
    assert (scores < 0).all()
    ix = FlatIPIndex.from_array(corpus, dtype="sq8", sq8_small_batch=True)
    D, I = ix.search(q, k)
    assert launches(ix) == 1
    assert (I >= 0).all() and (I < n).all()
    assert_topk(D, I, scores, k)
    ix.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_ties_equal_the_fp32_index_bit_for_bit():
    n, d, k = 20_000, 384, 50
    rng = np.random.default_rng(42)
    base = rng.integers(-127, 128, size=(400, d)).astype(np.float32)
    corpus = base[rng.integers(0, 400, size=n)]  # thousands of exact ties
    q = rng.integers(-8, 9, size=(16, d)).astype(np.float32)
    s8 = FlatIPIndex.from_array(corpus, dtype="sq8", sq8_step=np.ones(d, np.float32), sq8_small_batch=True)
    f32 = FlatIPIndex.from_array(corpus, dtype="f32")
    D8, I8 = s8.search(q, k)
    D32, I32 = f32.search(q, k)
    assert launches(s8) == 1 and f32.debug_counter(23) == 1  # ls_mq8 against ls_mq
    assert np.array_equal(I8, I32) and np.array_equal(D8, D32)
    assert (np.diff(D8, axis=1) == 0).sum() > 100  # the ties are really there
    s8.close()
    f32.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, d", [(4_095, 64), (4_100, 2048)])
def test_predicate_edges_rows_and_row_length(n, d):
    """Under 4096 rows, and rows of more than 64 chunks (d = 2048: 128): the option changes nothing."""
    c = case(n, d)
    D, I = c.ix.search(c.q, 10, normalize=True)
    assert launches(c.ix) == 0
    assert_topk(D, I, c.ref(True), 10)


def test_predicate_edge_k_too_large_for_the_key_lists():
    c = case(4_100, 512)

    def served_by_mq8(k):  # ask the library: does a two-query call of this k take the small-batch pass?
        before = launches(c.ix)
        c.ix.search(c.q[:2], k, normalize=True)
        return launches(c.ix) > before

    assert served_by_mq8(10)
    big = [k for k in (100, 200, 400, 800, 1600, 2048) if not served_by_mq8(k)]
    assert big, "no k was declined by the key-list rule"
    k = big[0]
    before = launches(c.ix)
    D, I = c.ix.search(c.q, k, normalize=True)
    assert launches(c.ix) == before
    assert_topk(D, I, c.ref(True), k)


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_entry_points():
    import torch

    c = case(5_000, 384)
    k = 50
    ref = c.ref(True)
    ix = FlatIPIndex.from_array(c.corpus, dtype="sq8", sq8_small_batch=True)  # (the same trained step: c.ref holds)
    assert np.array_equal(ix.sq8_step, c.step)
    tq = torch.from_numpy(c.q).cuda()
    for kw in ({}, {"asynchronous": True}):  # (asynchronous: the launch keeps its score vectors)
        before = launches(ix)
        s, i = ix.search_device(tq, k, normalize=True, **kw)
        torch.cuda.synchronize()
        assert launches(ix) == before + 1, kw
        assert_topk(s.cpu().numpy(), i.cpu().numpy(), ref, k)
    for lanes in (1, 2):  # one stream; then the two scan lanes whatever the corpus size
        ix.debug_option(24, lanes)
        before = launches(ix)
        outs = [ix.search_device(tq, k, normalize=True, pipeline=True) for _ in range(4)]  # 16 queries per call
        ix.check()
        assert launches(ix) == before + 4, lanes
        for s, i in outs:
            assert_topk(s.cpu().numpy(), i.cpu().numpy(), ref, k)
    ix.debug_option(24, 1)
    # 8 concurrent host callers: the combining queue serves them together in one pass
    gate = threading.Barrier(8)
    got = [None] * 8

    def caller(t):
        gate.wait()
        got[t] = [ix.search(c.q[j:j + 1], k, normalize=True) for j in (t, t + 8, t)]

    combined, passes = ix.debug_counter(16), launches(ix)
    for _ in range(5):  # (whether callers meet in the queue is the scheduler's choice: a few rounds)
        th = [threading.Thread(target=caller, args=(t,)) for t in range(8)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for t in range(8):
            for (Dt, It), j in zip(got[t], (t, t + 8, t)):
                assert_topk(Dt, It, ref[j:j + 1], k)
        if ix.debug_counter(16) > combined and launches(ix) > passes:
            break
    assert ix.debug_counter(16) > combined and launches(ix) > passes
    # a selection that cannot be proven (k' forced to 1) is repaired on the scan kernel: host call, pipelined call
    ix.debug_option(0, 1)
    served_again, before = ix.debug_counter(25), launches(ix)
    D, I = ix.search(c.q, k, normalize=True)
    assert ix.debug_counter(25) > served_again and launches(ix) == before + 1
    assert_topk(D, I, ref, k)
    served_again = ix.debug_counter(25)
    s, i = ix.search_device(tq, k, normalize=True, pipeline=True)
    ix.check()
    assert ix.debug_counter(25) > served_again and launches(ix) == before + 2
    assert_topk(s.cpu().numpy(), i.cpu().numpy(), ref, k)
    assert ix.debug_counter(23) == 0 and ix.debug_counter(34) == 0
    ix.close()


# ---- 9 ------------------------------------------------------------------------------------------------------------------
def test_add_after_enabling():
    c = case(5_000, 384)
    ix = FlatIPIndex.from_array(c.corpus[:4_700], dtype="sq8", sq8_step=c.step, sq8_small_batch=True)
    D, I = ix.search(c.q, 50, normalize=True)
    assert_topk(D, I, c.ref(True)[:, :4_700], 50)
    ix.add(c.corpus[4_700:])
    before = launches(ix)
    D, I = ix.search(c.q, 50, normalize=True)
    assert launches(ix) == before + 1
    assert_topk(D, I, c.ref(True), 50)
    ix.close()


# ---- 10 -----------------------------------------------------------------------------------------------------------------
def test_toggle():
    c = case(5_000, 100)
    k = 10
    results = []
    for on, moved in ((True, 1), (False, 0), (True, 1)):
        c.ix.set_sq8_small_batch(on)
        assert c.ix.sq8_small_batch is on
        before = launches(c.ix)
        results.append(c.ix.search(c.q, k, normalize=False))
        assert launches(c.ix) == before + moved, on
    for D, I in results[1:]:
        assert np.array_equal(D, results[0][0]) and np.array_equal(I, results[0][1])
    assert_topk(results[0][0], results[0][1], c.ref(False), k)
    f32 = FlatIPIndex.from_array(c.corpus[:64], dtype="f32")  # the C entry refuses other dtypes with a message
    lib = native.load()
    assert lib.ls_set_sq8_small_batch(f32._handle, 1) == native.LS_ERR_INVALID_ARG
    assert b"ls_set_sq8_small_batch" in lib.ls_last_error()
    assert lib.ls_set_f16_small_batch(c.ix._handle, 1) == native.LS_ERR_INVALID_ARG  # ... and the fp16 option still refuses sq8
    f32.close()
