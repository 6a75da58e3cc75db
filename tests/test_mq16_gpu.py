"""Small batches on an fp16 index with the opt-in small-batch pass (csrc/ls_mq16.hip, ls_set_f16_small_batch /
FlatIPIndex(f16_small_batch=True)): 1..32 queries share ONE corpus pass on the f16 matrix cores. The contract
(include/leansearch.h): exact top-k of the fp16 semantics within the 1e-5 / near-tie bar every fp16 test uses
(oracle.compare_topk), bit-exact on integer corpora, and a query's bits do not depend on its company, its column,
the entry point, a retry / repair, or row sharding; with the option off nothing changes. Reference call being
replaced: `index.search(x, k)`, src/lean_explore/search/engine.py:250 (issued concurrently by several MCP clients,
mcp/server.py:147-151)."""

import threading

import numpy as np
import pytest

from lean_explore_amd.index import FlatIPIndex
from oracle import oracle
from tests import helpers as H

pytestmark = pytest.mark.gpu

NQS = (1, 2, 3, 5, 8, 13, 16, 17, 24, 31, 32)


def one_by_one(ix, q, k, normalize=False):
    outs = [ix.search(q[j:j + 1], k, normalize=normalize) for j in range(q.shape[0])]
    return np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs])


def assert_usable(ix, q, k, normalize=False):
    """The pass serves this (index, k): a 2-query call is an ls_mq16 launch (counter 34)."""
    before = ix.debug_counter(34)
    ix.search(q[:2], k, normalize=normalize)
    assert ix.debug_counter(34) > before, "the fp16 small-batch pass is not usable for this (index, k)"


def tolerant_parity(D, I, c, qn, k):
    Dr, Ir = oracle.c_search(c, qn, k, f16=True)
    _, _, S = oracle.np_search(c, qn, k, f16=True)
    rep = oracle.compare_topk(D, I, Dr, Ir, S, score_tol=1e-5)
    assert rep["recall"] == 1.0, rep
    return rep


@pytest.mark.parametrize("d,k,normalize", [(384, 50, True), (1024, 1000, True), (100, 10, False), (64, 100, False),
                                           (768, 200, True), (36, 7, False), (2048, 50, True)])
def test_mq16_parity_and_invariance(d, k, normalize):
    n = 24_000 if d == 2048 else 40_000
    c = H.gauss(100 + d, n, d)
    q = H.gauss(200 + d, 32, d, normalize=not normalize) * (1.0 if not normalize else 3.0)
    ix = FlatIPIndex.from_array(c, dtype="f16", f16_small_batch=True)
    assert_usable(ix, q, k, normalize)
    D1, I1 = one_by_one(ix, q, k, normalize)
    qn = oracle.c_normalize_l2(q) if normalize else q
    Dr, Ir = oracle.c_search(c, qn, k, f16=True)
    _, _, S = oracle.np_search(c, qn, k, f16=True)
    res = {}
    for nq in NQS:
        b34, b25 = ix.debug_counter(34), ix.debug_counter(25)
        D, I = ix.search(q[:nq], k, normalize=normalize)
        d34, d25 = ix.debug_counter(34) - b34, ix.debug_counter(25) - b25
        print("mq16", d, k, nq, "launches", d34, "served again", d25)
        # ONE pass per call, plus one per query served again (a 1e-3 event on random data)
        assert d34 == 1 + d25 and ix.debug_counter(10) == 1, (nq, d34, d25, ix.debug_counter(10))
        rep = oracle.compare_topk(D, I, Dr[:nq], Ir[:nq], S[:nq], score_tol=1e-5)
        assert rep["recall"] == 1.0, (nq, rep)
        assert np.array_equal(D, D1[:nq]) and np.array_equal(I, I1[:nq]), (d, k, nq)
        res[nq] = (D, I)
    assert np.array_equal(res[32][0][:16], res[16][0]) and np.array_equal(res[32][1][:16], res[16][1])
    ix.close()


# One d per stored row length (16, 32, 48, 64, 96, 128, 192, 256 chunks: the kernel is instantiated by it, from the row
# geometry table) x the key-list sizes x one and two B blocks at their smallest and largest query counts: the launcher's
# whole dispatch. n = 4100 is just over LS_MQ_MIN_ROWS with a ragged last tile; there k = 10 / 30 / 100 select 3 / 5 / 8
# keys per lane (33 workgroups of four waves): tests/mq_plan_check.cpp asserts it.
@pytest.mark.parametrize("d", [64, 200, 384, 512, 768, 1024, 1536, 2048])
def test_mq16_every_row_length_key_count_and_block_count(d):
    n = 4100
    c = H.gauss(300 + d, n, d)
    q = H.gauss(400 + d, 32, d)
    ix = FlatIPIndex.from_array(c, dtype="f16", f16_small_batch=True)
    for k in (10, 30, 100):
        D1, I1 = one_by_one(ix, q, k)
        for nq in (1, 16, 17, 32):
            b34, b25 = ix.debug_counter(34), ix.debug_counter(25)
            D, I = ix.search(q[:nq], k)
            d34, d25 = ix.debug_counter(34) - b34, ix.debug_counter(25) - b25
            print("mq16 dispatch", d, k, nq, "launches", d34, "served again", d25)
            assert d34 == 1, (d, k, nq, d34, d25)
            assert np.array_equal(D, D1[:nq]) and np.array_equal(I, I1[:nq]), (d, k, nq)
            tolerant_parity(D, I, c, q[:nq], k)
    ix.close()


def test_mq16_full_size_is_one_pass():
    """N = 200 k, d = 384, k = 50: 16 and 32 queries are ONE launch each; the same 16 queries with the option off
    are two (a group of 8 + a group of 8): the structural evidence of the gain (timings: tools/f16_small_batch_time.py)."""
    c = H.gauss(1234, 200_000, 384)
    q = np.concatenate([H.gauss(5678, 16, 384), H.gauss(91011, 16, 384)])
    k = 50
    ix = FlatIPIndex.from_array(c, dtype="f16", f16_small_batch=True)
    assert_usable(ix, q, k)
    out = {}
    for nq in (16, 32):
        b34, b25 = ix.debug_counter(34), ix.debug_counter(25)
        D, I = ix.search(q[:nq], k)
        assert ix.debug_counter(34) - b34 == 1 + ix.debug_counter(25) - b25 and ix.debug_counter(10) == 1
        out[nq] = (D, I)
    rep = tolerant_parity(out[32][0], out[32][1], c, q, k)
    assert np.array_equal(out[32][0][:16], out[16][0]) and np.array_equal(out[32][1][:16], out[16][1])
    ix.set_f16_small_batch(False)
    b11, b20, b34 = ix.debug_counter(11), ix.debug_counter(20), ix.debug_counter(34)
    Doff, Ioff = ix.search(q[:16], k)
    assert ix.debug_counter(11) - b11 == 2 + ix.debug_counter(20) - b20, "option off: 16 queries are two scan groups"
    assert ix.debug_counter(34) == b34
    tolerant_parity(Doff, Ioff, c, q[:16], k)
    ix.close()
    print("mq16 full size", rep)


def test_mq16_integer_corpus_is_bit_exact_and_independent_of_the_deal():
    """Integer-valued rows and queries: every product and sum is exact, thousands of ties (a block of duplicated
    rows on top). Scores and indices equal the oracle's, also under a forced workgroup count (another deal of the
    tiles to waves and workgroups)."""
    c = H.int_corpus(7, 60_000, 128)
    c[30_000:30_400] = c[100:500]  # duplicated rows: exact ties far apart
    q = H.int_corpus(8, 32, 128)
    ix = FlatIPIndex.from_array(c, dtype="f16", f16_small_batch=True)
    for forced in (0, 64):
        ix.debug_option(7, forced)
        for k in (50, 1000):
            # (64 workgroups are 256 waves: at k = 1000 a wave would hold 3.9 of a query's top-k on average, more than
            # the 8-key lists are granted - by ls_mq_plan_lane_keys' rule that (index, k) stays on the scan groups. Exact
            # either way: integer arithmetic has one answer)
            usable = forced == 0 or k == 50
            if usable:
                assert_usable(ix, q, k)
            for nq in (9, 32):
                D, I = ix.search(q[:nq], k)
                assert ix.debug_counter(10) == 1 or not usable  # (unusable: as with the option off, 32 go batched)
                Dr, Ir = oracle.c_search(c, q[:nq], k, f16=True)
                assert np.array_equal(D, Dr) and np.array_equal(I, Ir), (forced, k, nq)
    ix.close()


@pytest.mark.parametrize("n", [4096, 4097, 5000, 8191, 16_400, 33_333])
def test_mq16_ragged_shards_and_base(n):
    c = H.gauss(n, n, 384)
    q = H.gauss(n + 1, 7, 384)
    base = 10_000_000_000
    ix = FlatIPIndex.from_array(c, dtype="f16", base=base, f16_small_batch=True)
    for k in (1, 50, 300):
        if k <= 50:  # (k = 300 of the smallest shards is more than the key lists take: the scan groups serve it, all 7 alike)
            assert_usable(ix, q, k)
        D, I = ix.search(q, k)
        assert I.min() >= base
        tolerant_parity(D, I - base, c, q, k)
        D1, I1 = one_by_one(ix, q, k)
        assert np.array_equal(D, D1) and np.array_equal(I, I1), (n, k)
    ix.close()


def test_mq16_special_values():
    c2 = H.gauss(8, 10_000, 64)
    c2[10, 0] = np.nan
    c2[11, 0] = -np.inf
    c2[12, 0] = np.inf
    ix = FlatIPIndex.from_array(c2, dtype="f16", f16_small_batch=True)
    qq = np.ones((3, 64), np.float32)
    assert_usable(ix, qq, 100)
    D, I = ix.search(qq, 100)
    Dr, Ir = oracle.c_search(c2, qq, 100, f16=True)
    _, _, S = oracle.np_search(c2, qq, 100, f16=True)
    # rank 0 is the +inf row (inf - inf has no tolerance: compared exactly), the finite ranks meet the usual bar;
    # the NaN and -inf rows are never returned
    assert np.all(I[:, 0] == 12) and np.all(np.isposinf(D[:, 0])) and np.array_equal(I[:, 0], Ir[:, 0])
    assert oracle.compare_topk(D[:, 1:], I[:, 1:], Dr[:, 1:], Ir[:, 1:], S, score_tol=1e-5)["recall"] == 1.0
    assert 10 not in I and 11 not in I
    D1, I1 = one_by_one(ix, qq, 100)
    assert np.array_equal(D, D1) and np.array_equal(I, I1)
    ix.close()


def test_mq16_retries_and_repairs_keep_the_bits():
    """A clustered corpus (rows sorted by one query's score) and k' = 1: nothing can be proven from the workgroups'
    keys, every query goes through the retry / repair of its entry point - and comes out with the bits of a query
    served alone: the re-serves run on the same kernel."""
    import torch

    d, k = 384, 100
    c = H.gauss(3, 30_000, d)
    q = H.gauss(4, 29, d)
    c = np.ascontiguousarray(c[np.argsort(c @ q[0])])
    ix = FlatIPIndex.from_array(c, dtype="f16", f16_small_batch=True)
    assert_usable(ix, q, k)
    D1, I1 = one_by_one(ix, q, k)
    tolerant_parity(D1, I1, c, q, k)
    ix.debug_option(0, 1)  # k' = 1
    # the host call: the launch wrote no score vectors, the unproven queries are served again (counter 25)
    b25, b34 = ix.debug_counter(25), ix.debug_counter(34)
    D, I = ix.search(q, k)
    assert ix.debug_counter(25) >= b25 + 20
    assert ix.debug_counter(34) - b34 == 1 + ix.debug_counter(25) - b25, "the re-serves must be ls_mq16 launches"
    assert np.array_equal(D, D1) and np.array_equal(I, I1)
    # pipelined device calls, repaired at check()
    tq = torch.from_numpy(q).cuda()
    b25 = ix.debug_counter(25)
    Dt, It = ix.search_device(tq, k, pipeline=True)
    Dt2, It2 = ix.search_device(tq[:19], k, pipeline=True)
    Dt3, It3 = ix.search_device(tq[5:6], k, pipeline=True)
    ix.check()
    assert ix.debug_counter(25) >= b25 + 20
    assert np.array_equal(Dt.cpu().numpy(), D1) and np.array_equal(It.cpu().numpy(), I1)
    assert np.array_equal(Dt2.cpu().numpy(), D1[:19]) and np.array_equal(It2.cpu().numpy(), I1[:19])
    assert np.array_equal(Dt3.cpu().numpy(), D1[5:6]) and np.array_equal(It3.cpu().numpy(), I1[5:6])
    # LS_FLAG_ASYNC alone keeps the score vectors: rescued from S in stream order
    b25 = ix.debug_counter(25)
    Dt, It = ix.search_device(tq, k, asynchronous=True)
    torch.cuda.synchronize()
    assert ix.debug_counter(25) == b25
    assert np.array_equal(Dt.cpu().numpy(), D1) and np.array_equal(It.cpu().numpy(), I1)
    # in-order pipelined calls keep them too
    outs = [ix.search_device(tq[:m], k, pipeline=True, inorder=True) for m in (29, 1, 3)]
    ix.check()
    assert ix.debug_counter(25) == b25
    for m, (Dt, It) in zip((29, 1, 3), outs):
        assert np.array_equal(Dt.cpu().numpy(), D1[:m]) and np.array_equal(It.cpu().numpy(), I1[:m])
    ix.debug_option(19, 0)  # host calls keep their score vectors: the stand-alone finalize rescues from S
    D, I = ix.search(q, k)
    assert ix.debug_counter(25) == b25
    assert np.array_equal(D, D1) and np.array_equal(I, I1)
    ix.close()


def test_option_off_is_untouched_and_fp32_refuses():
    c = H.gauss(91, 60_000, 128)
    q = H.gauss(92, 12, 128)
    ix = FlatIPIndex.from_array(c, dtype="f16")

    def off_call():
        b11, b20, b34 = ix.debug_counter(11), ix.debug_counter(20), ix.debug_counter(34)
        D, I = ix.search(q, 10)
        return D, I, ix.debug_counter(11) - b11 - (ix.debug_counter(20) - b20), ix.debug_counter(34) - b34

    D0, I0, l0, m0 = off_call()
    assert l0 == 2 and m0 == 0, "12 queries on an fp16 index: one group of 8 + one of 4"
    ix.set_f16_small_batch(True)
    b34 = ix.debug_counter(34)
    Don, Ion = ix.search(q, 10)
    assert ix.debug_counter(34) > b34
    tolerant_parity(Don, Ion, c, q, 10)
    ix.set_f16_small_batch(False)
    D2, I2, l2, m2 = off_call()
    assert (l2, m2) == (l0, m0)
    assert np.array_equal(D2, D0) and np.array_equal(I2, I0)
    ix.close()
    ix32 = FlatIPIndex.from_array(c[:5000])
    ix32.search(q[:1], 10)
    with pytest.raises(ValueError):
        ix32.set_f16_small_batch(True)
    from lean_explore_amd import native
    assert native.load().ls_set_f16_small_batch(ix32._handle, 1) == native.LS_ERR_INVALID_ARG
    ix32.close()


def test_mq16_concurrent_callers_are_combined_and_bit_identical():
    """16 threads, one query per ls_search: the combining queue gathers up to 32 of them into one pass; every answer
    is the single-threaded answer, bit for bit, and there were fewer launches than requests."""
    n, d, T, per, k = 120_000, 256, 16, 200, 50
    corpus = H.gauss(81, n, d)
    pool = H.gauss(82, 64, d, normalize=False)
    ix = FlatIPIndex.from_array(corpus, dtype="f16", f16_small_batch=True)
    try:
        assert_usable(ix, pool, k, True)
        want = [ix.search(pool[qi:qi + 1], k, normalize=True) for qi in range(64)]
        errors = []
        b34, b25 = ix.debug_counter(34), ix.debug_counter(25)

        def worker(t):
            rng = np.random.default_rng(t)
            for j in range(per):
                qi = int(rng.integers(64))
                D, I = ix.search(pool[qi:qi + 1], k, normalize=True)
                if not (np.array_equal(D, want[qi][0]) and np.array_equal(I, want[qi][1])):
                    errors.append((t, j, qi))

        threads = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors[:5]
        launches = ix.debug_counter(34) - b34 - (ix.debug_counter(25) - b25)
        print("mq16 concurrent:", T * per, "requests in", launches, "passes")
        assert launches < T * per, "16 threads hammering one handle never met in a batch"
        assert ix.debug_counter(16) >= 1
        D = np.concatenate([want[qi][0] for qi in range(4)])
        I = np.concatenate([want[qi][1] for qi in range(4)])
        tolerant_parity(D, I, corpus, oracle.c_normalize_l2(pool[:4]), k)
    finally:
        ix.close()


def test_mq16_sharded_rehearsal_equals_the_unsharded_index():
    """Three row shards rehearsed on one GPU (20 000 rows each: the pass is usable on every shard). A score depends
    on the row and the query only and the merge is exact: the unsharded option-on index's bits."""
    c = H.gauss(61, 60_000, 384)
    q = H.gauss(62, 32, 384)
    k = 50
    one = FlatIPIndex.from_array(c, dtype="f16", f16_small_batch=True)
    assert_usable(one, q, k)
    sh = FlatIPIndex.from_array(c, dtype="f16", devices=[0, 0, 0], f16_small_batch=True)
    for nq in (1, 12, 32):
        D, I = one.search(q[:nq], k)
        b34 = sh.debug_counter(34)
        Ds, Is = sh.search(q[:nq], k)
        assert sh.debug_counter(34) - b34 >= 3, "every shard must have used the pass"
        assert np.array_equal(Ds, D) and np.array_equal(Is, I), nq
    sh.close()
    one.close()


def test_batched_path_still_serves_large_batches_with_the_option_on():
    """nq = 64 > 32 on a big enough shard: the batched MFMA path (counter 10 == 2); its repairs (a planted cluster
    overflows the candidate queues) are re-served by the small-batch pass and stay within the fp16 tolerance."""
    c = H.gauss(21, 60_000, 384)
    q = H.gauss(22, 64, 384)
    rng = np.random.default_rng(5)
    lo = 3125 * 7 + 40 * 32
    for r in range(lo, lo + 300):
        v = q[0] + 0.05 * rng.standard_normal(384).astype(np.float32)
        c[r] = v / np.linalg.norm(v)
    ix = FlatIPIndex.from_array(c, dtype="f16", f16_small_batch=True)
    assert_usable(ix, q, 100)
    b8, b34 = ix.debug_counter(8), ix.debug_counter(34)
    D, I = ix.search(q, 100)
    assert ix.debug_counter(10) == 2, "64 queries must take the batched fp16 MFMA path"
    print("mq16 + batched: repaired queries", ix.debug_counter(8) - b8, "ls_mq16 launches", ix.debug_counter(34) - b34)
    assert ix.debug_counter(8) > b8, "the planted cluster must have gone through the repair"
    assert ix.debug_counter(34) > b34, "the repair must run on the small-batch pass"
    tolerant_parity(D, I, c, q, 100)
    ix.close()
