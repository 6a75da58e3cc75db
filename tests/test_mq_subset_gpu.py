"""Subset search with the opt-in pass (csrc/ls_mq_subset.hip, ls_set_subset_small_batch /
FlatIPIndex(subset_small_batch=True)): groups of 2..16 queries of a call share ONE pass over the selected rows on the f32
matrix cores. The contract is bit-identity: every result is array_equal to the oracle over corpus[rows] in the scan
kernel's summation order (the `expect` of tests/test_subset_gpu.py), to the option-off result of the same call and to
each query's lone call. Counter 37 counts the passes.

The shapes are the smallest at which the kernel can go wrong: 12 001 rows (n % 16 == 1: the all-ones subset ends in a
ragged tile), subsets just above the 4096-row predicate, 48 workgroups (every wave has two tiles and prefetches past its
last one)."""

import threading

import numpy as np
import pytest

from lean_explore_amd import faiss_compat as fc
from lean_explore_amd import native
from lean_explore_amd.index import FlatIPIndex
from oracle import oracle
from tests import helpers as H
from tests import mq_subset_shapes as SH

pytestmark = pytest.mark.gpu

N = SH.N
NEG = -np.finfo(np.float32).max


def sub_search(ix, q, k, sel, normalize=False):
    return ix.search(q, k, normalize=normalize, params=fc.SearchParameters(sel=sel))


def expect(corpus, rows, q, k, normalize=False):
    """Oracle over corpus[rows] in the scan kernel's summation order, indices mapped through rows."""
    qq = oracle.c_normalize_l2(q) if normalize else q
    D, I = oracle.c_search(corpus[rows], qq, k, order="scan")
    return D, np.where(I >= 0, rows[np.maximum(I, 0)], -1)


def passes(ix):
    return ix.debug_counter(37)


def equal(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def on_and_off(ix, q, k, sel, normalize=False):
    """The same call with the option on and off: (result on, result off, passes the on call took)."""
    ix.set_subset_small_batch(True)
    before = passes(ix)
    got = sub_search(ix, q, k, sel, normalize)
    took = passes(ix) - before
    ix.set_subset_small_batch(False)
    off = sub_search(ix, q, k, sel, normalize)
    assert passes(ix) == before + took, "the option-off call must not take a pass"
    return got, off, took


class Case:
    """One d = 384 index of 12 001 rows, the half subset and its references, shared by the tests that need them."""

    def __init__(self):
        self.d = 384
        self.corpus = H.gauss(301, N, self.d)
        self.q = H.gauss(302, 40, self.d, normalize=False)
        self.rows = SH.half_rows()
        self.ix = FlatIPIndex.from_array(self.corpus)
        self.sub = self.ix.subset(self.rows)
        self._ref = {}

    def ref(self, k, normalize=False):
        if (k, normalize) not in self._ref:
            self._ref[(k, normalize)] = expect(self.corpus, self.rows, self.q, k, normalize)
        return self._ref[(k, normalize)]


@pytest.fixture(scope="module")
def c():
    case = Case()
    yield case
    case.ix.close()


@pytest.mark.parametrize("d", [64, 128, 192, 256, 384, 512, 768, 1024, 100, 1000, 160])
def test_every_geometry_matches_the_oracle_and_option_off(d):
    """The eight fp32 row geometries (and three ragged row lengths): a random half of the rows, 16 queries, k = 10."""
    corpus = H.gauss(100 + d, N, d)
    q = H.gauss(200 + d, 16, d, normalize=False)
    rows = SH.half_rows()
    assert SH.plan(rows.size, 10)[2] == 3
    ix = FlatIPIndex.from_array(corpus)
    sub = ix.subset(rows)
    for normalize in (False, True):
        got, off, took = on_and_off(ix, q, 10, sub, normalize)
        assert took == 1
        assert equal(got, expect(corpus, rows, q, 10, normalize)) and equal(got, off), (d, normalize)
    ix.close()


@pytest.mark.parametrize("k", SH.K_SWEEP)
def test_every_key_list_size(c, k):
    """k = 10 / 50 / 150: 3 / 5 / 8 keys per lane serve the pass; k = 1000 is declined (tests/test_mq_subset_cpu.py)."""
    keys = SH.plan(c.rows.size, k)[2]
    got, off, took = on_and_off(c.ix, c.q[:16], k, c.sub)
    assert took == (1 if keys else 0), (k, keys)
    ref = c.ref(k)
    assert equal(got, (ref[0][:16], ref[1][:16])) and equal(got, off), k


def test_query_counts(c):
    k = 10
    lone = [sub_search(c.ix, c.q[i:i + 1], k, c.sub) for i in range(40)]
    ref = c.ref(k)
    for nq, groups in zip((1, 2, 3, 15, 16, 17, 18, 32, 33, 40), (0, 1, 1, 1, 1, 1, 2, 2, 2, 3)):
        assert SH.groups(nq) == groups
        got, off, took = on_and_off(c.ix, c.q[:nq], k, c.sub)
        assert took == groups, nq
        assert equal(got, off) and equal(got, (ref[0][:nq], ref[1][:nq])), nq
        for i in range(nq):
            assert np.array_equal(got[0][i], lone[i][0][0]) and np.array_equal(got[1][i], lone[i][1][0]), (nq, i)


def test_subset_shapes(c):
    k, q = 10, c.q[:16]
    ends = np.concatenate(([0], np.arange(2000, 2000 + 4500), [N - 1]))
    shapes = {
        "all ones": (np.arange(N), 1),                             # ragged last tile (12 001 = 750 x 16 + 1)
        "m = 4096": (np.sort(np.random.default_rng(5).choice(N, SH.MIN_ROWS, replace=False)), 1),
        "m = 4095": (np.sort(np.random.default_rng(6).choice(N, SH.MIN_ROWS - 1, replace=False)), 0),
        "one block": (np.arange(3001, 3001 + 5003), 1),
        "rows 0 and n - 1": (ends, 1),
    }
    for name, (rows, want) in shapes.items():
        got, off, took = on_and_off(c.ix, q, k, rows)
        assert took == want, name
        assert equal(got, expect(c.corpus, rows, q, k)) and equal(got, off), name
    # (a query aimed at a row finds it: the first and the last row of the index are really read)
    for r in (0, N - 1):
        D, I = sub_search_on(c.ix, c.corpus[r:r + 1].repeat(2, 0), 1, ends)
        assert (I == r).all()


def test_every_third_row():
    """(12 001 rows hold 4001 of them, under the predicate: an index of 13 001 rows holds 4334)"""
    n, d, k = 13_001, 64, 10
    corpus = H.gauss(340, n, d)
    q = H.gauss(341, 16, d, normalize=False)
    rows = np.arange(0, n, 3)
    assert rows.size > SH.MIN_ROWS and SH.plan(rows.size, k)[2] == 3
    ix = FlatIPIndex.from_array(corpus)
    got, off, took = on_and_off(ix, q, k, rows)
    assert took == 1 and equal(got, expect(corpus, rows, q, k)) and equal(got, off)
    ix.close()


def sub_search_on(ix, q, k, sel):
    ix.set_subset_small_batch(True)
    before = passes(ix)
    out = sub_search(ix, q, k, sel)
    assert passes(ix) == before + 1
    ix.set_subset_small_batch(False)
    return out


def test_subset_survives_add_and_base():
    """A subset created before a later ls_add keeps its rows; ls_set_base shifts the returned rows only."""
    d, k, base = 128, 10, 1_000_000
    corpus = H.gauss(310, N, d)
    q = H.gauss(311, 16, d, normalize=False)
    rows = SH.half_rows()
    want = expect(corpus, rows, q, k)
    ix = FlatIPIndex.from_array(corpus, subset_small_batch=True)
    sub = ix.subset(rows)
    assert equal(sub_search(ix, q, k, sub), want) and passes(ix) == 1
    ix.add(10.0 * H.gauss(312, 700, d))  # (rows that would win every query: not in the subset)
    assert equal(sub_search(ix, q, k, sub), want) and passes(ix) == 2
    native.check(native.load().ls_set_base(ix._handle, base))
    D, I = sub_search(ix, q, k, sub)
    assert np.array_equal(D, want[0]) and np.array_equal(I, want[1] + base) and passes(ix) == 3
    ix.close()


def test_rows_that_must_never_come_back():
    d, k = 128, 20
    corpus = H.gauss(320, N, d)
    rows = SH.half_rows()
    bad = rows[[0, 17, 1000, 3001, rows.size - 1]]
    corpus[bad[0::2]] = np.nan
    corpus[bad[1::2]] = -np.inf
    q = np.abs(H.gauss(321, 16, d, normalize=False))  # (positive: a -inf row scores -inf, not NaN)
    ix = FlatIPIndex.from_array(corpus)
    got, off, took = on_and_off(ix, q, k, rows)
    assert took == 1 and not np.isin(got[1], bad).any()
    assert equal(got, expect(corpus, rows, q, k)) and equal(got, off)
    ix.close()


def test_integer_ties_come_out_row_ascending():
    """An integer corpus (every score exact) with a thousand duplicated rows: ties everywhere, k = 500."""
    n, d, k = SH.TIES_N, 128, 500
    ic = H.int_corpus(2, n, d)
    ic[1000:2000] = ic[:1000]
    qi = H.int_corpus(3, 16, d)
    rows = SH.ties_rows()
    assert SH.plan(rows.size, k)[2] == 8
    ix = FlatIPIndex.from_array(ic)
    got, off, took = on_and_off(ix, qi, k, rows)
    assert took == 1
    assert equal(got, expect(ic, rows, qi, k)) and equal(got, off)
    ix.close()


@pytest.mark.parametrize("which,value,k", [(0, 1, 50), (1, 1, 50), (7, 1, 2), (7, 3, 2), (7, SH.MAX_BLOCKS, 2)])
def test_forced_paths_stay_exact(c, which, value, k):
    """Debug option 0: one key per workgroup (the keys prove nothing: the rescue sweeps the score vectors the pass
    wrote); option 1: the general selection; option 7: 1, 3 and the most workgroups a handle takes (at a k the key lists
    of 4 and 12 waves still take: the plan declines larger ones there)."""
    assert SH.plan(c.rows.size, k, forced_blocks=value if which == 7 else 0)[2] > 0
    ref = c.ref(k)
    c.ix.debug_option(which, value)
    try:
        got, off, took = on_and_off(c.ix, c.q[:16], k, c.sub)
    finally:
        c.ix.debug_option(which, 0)
    assert took == 1, (which, value)
    assert equal(got, (ref[0][:16], ref[1][:16])) and equal(got, off), (which, value)


def test_plain_passes_and_subset_passes_alternate(c):
    k = 10
    plain_ref = oracle.c_search(c.corpus, c.q[:8], k, order="scan")
    ref = c.ref(k)
    c.ix.set_subset_small_batch(True)
    try:
        for _ in range(3):
            mq0, p0 = c.ix.debug_counter(23), passes(c.ix)
            assert equal(c.ix.search(c.q[:8], k), plain_ref)
            assert equal(sub_search(c.ix, c.q[:16], k, c.sub), (ref[0][:16], ref[1][:16]))
            assert c.ix.debug_counter(23) >= mq0 + 1 and passes(c.ix) == p0 + 1
    finally:
        c.ix.set_subset_small_batch(False)


def test_concurrent_plain_and_subset_callers_with_the_option_on(c):
    k, rounds = 10, 12
    ref = c.ref(k)
    want_plain = [c.ix.search(c.q[i:i + 1], k) for i in range(8)]
    bad = []
    c.ix.set_subset_small_batch(True)
    p0 = passes(c.ix)

    def worker(t):
        rng = np.random.default_rng(t)
        for _ in range(rounds):
            if t % 2 == 0:
                i = int(rng.integers(8))
                if not equal(c.ix.search(c.q[i:i + 1], k), want_plain[i]):
                    bad.append((t, "plain", i))
            else:
                i = int(rng.integers(0, 24))
                if not equal(sub_search(c.ix, c.q[i:i + 16], k, c.sub), (ref[0][i:i + 16], ref[1][i:i + 16])):
                    bad.append((t, "subset", i))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(6)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    c.ix.set_subset_small_batch(False)
    assert not bad
    assert passes(c.ix) == p0 + 3 * rounds


def test_default_is_off_and_switching_back_restores_it():
    d, k = 64, 10
    corpus = H.gauss(330, N, d)
    q = H.gauss(331, 16, d, normalize=False)
    rows = SH.half_rows()
    ix = FlatIPIndex.from_array(corpus)
    assert ix.subset_small_batch is False
    first = sub_search(ix, q, k, rows)
    assert passes(ix) == 0
    ix.set_subset_small_batch(True)
    assert equal(sub_search(ix, q, k, rows), first) and passes(ix) == 1
    ix.set_subset_small_batch(False)
    assert equal(sub_search(ix, q, k, rows), first) and passes(ix) == 1
    # the C entry point refuses what it does not serve, and says so
    lib = native.load()
    f16 = FlatIPIndex.from_array(corpus[:2000], dtype="f16")
    assert lib.ls_set_subset_small_batch(f16._handle, 1) == native.LS_ERR_INVALID_ARG
    assert b"ls_set_subset_small_batch" in lib.ls_last_error()
    assert lib.ls_set_subset_small_batch(f16._handle, 0) == 0
    f16.close()
    ix.close()
