"""``ls_remove`` on the MI355X (include/leansearch_remove.h): after ``remove_ids`` a flat index is, in everything
observable, the index built from the surviving rows - stored rows, codes and step, every search result bit for bit,
its subsets, a later ``add`` - on one device, row-sharded and replicated, with the corpus compacted in place through
staging slabs of any size.

The reference in every case is a FRESH index built from ``host_corpus()`` of the index before the removal (same
dtype; sq8: ``sq8_step=`` the original's step), never the index under test itself; everything is ``array_equal``."""

import ctypes

import numpy as np
import pytest

from lean_explore_amd import faiss_compat as fc
from lean_explore_amd import native
from lean_explore_amd.index import FlatIPIndex
from tests import helpers as H

pytestmark = pytest.mark.gpu

NEG = np.float32(-3.4028234663852886e38)
N = 20_011  # three compaction blocks of 8192 with a ragged tail; above the 4096-row threshold of the small-batch passes


def build(x, dtype, step=None, **kw):
    return FlatIPIndex.from_array(x, dtype=dtype, sq8_step=step if dtype == "sq8" else None, **kw)


def fresh_like(ix, rows_before, keep, extra=None, **kw):
    """The reference: a fresh index of the surviving rows (``rows_before``: host_corpus() before the removal)."""
    x = rows_before[keep]
    if extra is not None:
        x = np.concatenate([x, extra])
    dtype = ix.storage_dtype
    return build(np.ascontiguousarray(x), dtype, ix.sq8_step if dtype == "sq8" else None, **kw)


def same_stored(a, b):
    assert a.ntotal == b.ntotal
    assert np.array_equal(a.host_corpus(), b.host_corpus())
    if a.storage_dtype == "sq8":
        assert np.array_equal(a.codes(), b.codes()) and np.array_equal(a.sq8_step, b.sq8_step)


def same_searches(a, b, q, shapes=((1, 10), (5, 10), (1, 100), (5, 100))):
    for nq, k in shapes:
        Da, Ia = a.search(q[:nq], k)
        Db, Ib = b.search(q[:nq], k)
        assert np.array_equal(Ia, Ib) and np.array_equal(Da, Db), (nq, k)


def big_removal(n, seed=1):
    gone = np.random.default_rng(seed).random(n) < 0.3
    gone[0] = gone[n - 1] = True
    gone[8192:16384] = True
    return gone


@pytest.mark.parametrize("dtype,d", [("f32", 384), ("f32", 100), ("f32", 1024), ("f16", 384), ("sq8", 384), ("sq8", 20),
                                     ("f32", 64), ("f32", 256), ("f32", 512), ("f32", 768)])
def test_removal_equals_the_fresh_index(dtype, d):
    x, q = H.gauss(100 + d, N, d), H.gauss(200 + d, 40, d, normalize=False)
    ix = build(x, dtype)
    ref = None
    try:
        before = ix.host_corpus()
        gone = big_removal(N)
        ix.set_remove_slab_rows(1000)
        assert ix.remove_ids(gone) == gone.sum() and ix.ntotal == N - gone.sum()
        moved, slabs, _, _ = ix.remove_stats()
        assert slabs > 1 and moved == ix.ntotal - 0 and slabs == -(-moved // 1000)  # (row 0 is removed: r0 == 0)
        ref = fresh_like(ix, before, ~gone)
        same_stored(ix, ref)
        same_searches(ix, ref, q)
        if dtype == "f32":
            same_searches(ix, ref, q, shapes=((40, 10),))
    finally:
        ix.close()
        if ref is not None:
            ref.close()


def test_slab_size_does_not_matter():
    n, d = 997, 100
    x, q = H.gauss(7, n, d), H.gauss(8, 5, d, normalize=False)
    gone = np.random.default_rng(3).random(n) < 0.4
    gone[:5] = False  # r0 == 5
    gone[5] = True
    n_new = int((~gone).sum())
    ref = build(np.ascontiguousarray(x[~gone]), "f32")
    try:
        for slab in (7, 64, 1000, 0):
            ix = build(x, "f32")
            try:
                ix.set_remove_slab_rows(slab)
                assert ix.remove_ids(gone) == gone.sum()
                moved, slabs, _, _ = ix.remove_stats()
                assert moved == n_new - 5, slab
                assert slabs == (-(-moved // slab) if slab else 1), slab
                same_stored(ix, ref)
                same_searches(ix, ref, q)
            finally:
                ix.close()
    finally:
        ref.close()


@pytest.mark.parametrize("dtype", ["f32", "sq8"])
def test_edges(dtype):
    n, d = 5000, 100
    x, q, y = H.gauss(17, n, d), H.gauss(18, 5, d, normalize=False), H.gauss(19, 300, d)
    ix = build(x, dtype)
    refs = []

    def fresh(keep, extra=None):
        refs.append(fresh_like(ix, before, keep, extra))
        return refs[-1]

    try:
        before = ix.host_corpus()
        keep = np.ones(n, bool)
        # nothing removed
        assert ix.remove_ids(np.zeros(n, bool)) == 0 and ix.remove_ids(np.zeros(0, np.int64)) == 0
        assert ix.remove_stats()[:2] == (0, 0) and ix.ntotal == n
        same_stored(ix, fresh(keep))
        # only a tail removed: nothing moves; a later add proves the pad rows and the append position
        assert ix.remove_ids(fc.IDSelectorRange(4000, n)) == 1000
        keep[4000:] = False
        assert ix.remove_stats()[:2] == (0, 0) and ix.ntotal == 4000
        same_stored(ix, fresh(keep))
        same_searches(ix, refs[-1], q)
        ix.add(y)
        r = fresh(keep, y)
        same_stored(ix, r)
        same_searches(ix, r, q)
        before, keep = ix.host_corpus(), np.ones(4300, bool)
        # only a head removed: everything moves, the slab once smaller and once larger than the shift
        for shift, slab in ((100, 30), (64, 1000)):
            ix.set_remove_slab_rows(slab)
            assert ix.remove_ids(np.arange(shift)) == shift
            keep[np.flatnonzero(keep)[:shift]] = False
            moved, slabs, _, _ = ix.remove_stats()
            assert moved == ix.ntotal == keep.sum() and slabs == -(-moved // slab)
            r = fresh(keep)
            same_stored(ix, r)
            same_searches(ix, r, q)
        # one row left
        last = np.flatnonzero(keep)[1234]
        assert ix.remove_ids(np.arange(ix.ntotal) != 1234) == keep.sum() - 1
        keep[:] = False
        keep[last] = True
        assert ix.ntotal == 1
        r = fresh(keep)
        same_stored(ix, r)
        same_searches(ix, r, q, shapes=((1, 10), (5, 10)))
        # everything removed: all padding, then add equals a fresh index
        assert ix.remove_ids(np.ones(1, bool)) == 1 and ix.ntotal == 0
        D, I = ix.search(q, 10)
        assert (I == -1).all() and (D == NEG).all()
        assert ix.host_corpus().shape == (0, d)
        ix.add(y)
        keep[:] = False
        r = fresh(keep, y)
        same_stored(ix, r)
        same_searches(ix, r, q)
    finally:
        ix.close()
        for r in refs:
            r.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_remove_and_add_in_both_orders(dtype):
    n, d = 9000, 384
    x, y, q = H.gauss(27, n, d), H.gauss(28, 700, d), H.gauss(29, 5, d, normalize=False)
    gone = np.random.default_rng(4).random(n) < 0.2
    a, b = build(x, dtype), build(x, dtype)
    ra = rb = None
    try:
        before = a.host_corpus()
        a.remove_ids(gone)
        a.add(y)                                   # remove, then add
        ra = fresh_like(a, before, ~gone, y)
        same_stored(a, ra)
        same_searches(a, ra, q)
        b.add(y)                                   # add, then remove (old and new rows)
        before_b = b.host_corpus()
        gone_b = np.concatenate([gone, np.arange(700) % 3 == 0])
        assert b.remove_ids(gone_b) == gone_b.sum()
        rb = fresh_like(b, before_b, ~gone_b)
        same_stored(b, rb)
        same_searches(b, rb, q)
    finally:
        for ix in (a, b, ra, rb):
            if ix is not None:
                ix.close()


def sub_search(ix, q, k, sel):
    return ix.search(q, k, params=fc.SearchParameters(sel=sel))


@pytest.mark.parametrize("dtype", ["f32", "sq8"])
def test_subsets_made_before_the_removal(dtype):
    d = 100
    x, q = H.gauss(37, N, d), H.gauss(38, 5, d, normalize=False)
    kw = {"subset_small_batch": True} if dtype == "f32" else {}
    ix = build(x, dtype, **kw)
    ref = None
    try:
        before = ix.host_corpus()
        rng = np.random.default_rng(6)
        masks = {"wholly removed": np.zeros(N, bool), "untouched": np.zeros(N, bool), "partly removed": rng.random(N) < 0.6}
        masks["wholly removed"][9000:9500] = True
        masks["untouched"][3000:3700] = True
        subs = {name: ix.subset(m) for name, m in masks.items()}
        assert all(subs[name].rows == m.sum() for name, m in masks.items())
        gone = rng.random(N) < 0.25
        gone[9000:9500] = True
        gone[3000:3700] = False
        gone[0] = True
        ix.set_remove_slab_rows(3000)
        assert ix.remove_ids(gone) == gone.sum()
        renum = np.cumsum(~gone) - 1  # old row -> new row (survivors)
        ref = fresh_like(ix, before, ~gone, **kw)
        same_stored(ix, ref)
        for name, m in masks.items():
            want = renum[m & ~gone]
            assert subs[name].valid and subs[name].rows == want.size, name
            for nq, k in ((1, 10), (5, 10), (5, 100)):
                c37 = ix.debug_counter(37)
                D, I = sub_search(ix, q[:nq], k, subs[name])
                Dr, Ir = sub_search(ref, q[:nq], k, want)
                assert np.array_equal(I, Ir) and np.array_equal(D, Dr), (name, nq, k)
                if name == "wholly removed":
                    assert (I == -1).all() and (D == NEG).all()
                elif dtype == "f32" and (nq, k) == (5, 10) and want.size >= 4096:
                    assert ix.debug_counter(37) > c37, "the 5-query call takes the subset pass"
        assert subs["wholly removed"].rows == 0 and subs["untouched"].rows == 700
        assert subs["partly removed"].rows >= 4096
        # a subset created afterwards
        after = ix.subset(np.arange(0, ix.ntotal, 3))
        D, I = sub_search(ix, q[:1], 10, after)
        Dr, Ir = sub_search(ref, q[:1], 10, np.arange(0, ref.ntotal, 3))
        assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
        for s in list(subs.values()) + [after]:
            s.close()
    finally:
        ix.close()
        if ref is not None:
            ref.close()


@pytest.mark.parametrize("dtype,base", [("f32", 0), ("f16", 0), ("f32", 1000)])
def test_sharded_handle(dtype, base):
    d = 100
    x, y, q = H.gauss(47, N, d), H.gauss(48, 500, d), H.gauss(49, 5, d, normalize=False)
    ix = build(x, dtype, devices=[0, 0, 0], base=base)
    plain = build(x, dtype, base=base)  # (the rows as this dtype stores them)
    refs = []
    try:
        before = plain.host_corpus()
        assert np.array_equal(before, ix.host_corpus())
        sh = ix.shards()
        lo1, n1 = sh[1][1] - base, sh[1][2]
        rng = np.random.default_rng(8)
        sel = rng.random(N) < 0.5
        sub = ix.subset(sel)
        gone = rng.random(N) < 0.1
        gone[lo1 - 600:lo1 + n1 + 900] = True  # empties the middle shard and trims the other two
        ix.set_remove_slab_rows(1500)
        assert ix.remove_ids(gone) == gone.sum() and ix.ntotal == N - gone.sum()
        sh = ix.shards()
        assert sh[1][2] == 0 and sh[0][2] > 0 and sh[2][2] > 0
        assert sum(r for _, _, r in sh) == ix.ntotal
        assert [r0 for _, r0, _ in sh] == [base, base + sh[0][2], base + sh[0][2] + sh[1][2]]
        assert sh[0][2] == (~gone[:lo1]).sum() and sh[2][2] == (~gone[lo1 + n1:]).sum()
        refs.append(fresh_like(plain, before, ~gone, base=base))
        same_stored(ix, refs[-1])
        same_searches(ix, refs[-1], q)
        renum = np.cumsum(~gone) - 1
        want = renum[sel & ~gone]
        assert sub.rows == want.size
        for nq, k in ((1, 10), (3, 100)):
            D, I = sub_search(ix, q[:nq], k, sub)
            Dr, Ir = sub_search(refs[-1], q[:nq], k, want)
            assert np.array_equal(I, Ir) and np.array_equal(D, Dr), (nq, k)
        sub.close()
        ix.add(y)  # extends the last shard
        sh2 = ix.shards()
        assert sh2[2][2] == sh[2][2] + 500 and sh2[:2] == sh[:2]
        refs.append(fresh_like(plain, before, ~gone, y, base=base))
        same_stored(ix, refs[-1])
        same_searches(ix, refs[-1], q)
    finally:
        ix.close()
        plain.close()
        for r in refs:
            r.close()


def test_replicated_handle():
    d = 100
    x, q = H.gauss(57, N, d), H.gauss(58, 5, d, normalize=False)
    ix = build(x, "f32", devices=[0, 0, 0], replicate=True)
    ref = None
    try:
        before = ix.host_corpus()
        gone = big_removal(N, seed=9)
        ix.set_remove_slab_rows(2000)
        assert ix.remove_ids(gone) == gone.sum() and ix.ntotal == N - gone.sum()
        ref = fresh_like(ix, before, ~gone)
        same_stored(ix, ref)
        for _ in range(3):  # consecutive host searches: one per replica
            same_searches(ix, ref, q, shapes=((1, 10), (5, 100)))
    finally:
        ix.close()
        if ref is not None:
            ref.close()


def test_pending_pipelined_calls_see_the_index_as_it_was():
    import torch

    d, k = 384, 10
    x, q = H.gauss(67, N, d), H.gauss(68, 7, d, normalize=False)
    ix = build(x, "f32")
    ref = None
    try:
        before = ix.host_corpus()
        D0, I0 = ix.search(q, k)
        tq = torch.from_numpy(q).cuda()
        parts = (slice(0, 1), slice(1, 6), slice(6, 7))
        qs = [tq[p].contiguous() for p in parts]
        outs = [ix.search_device(t, k, pipeline=True) for t in qs]
        gone = big_removal(N, seed=11)
        assert ix.remove_ids(gone) == gone.sum()  # (no check() in between)
        ix.check()
        torch.cuda.synchronize()
        for p, (s, i) in zip(parts, outs):
            assert np.array_equal(i.cpu().numpy(), I0[p]) and np.array_equal(s.cpu().numpy(), D0[p])
        ref = fresh_like(ix, before, ~gone)
        same_stored(ix, ref)
        same_searches(ix, ref, q)
    finally:
        ix.close()
        if ref is not None:
            ref.close()


def test_refused_calls_change_nothing():
    n, d = 3000, 100
    x, q = H.gauss(77, n, d), H.gauss(78, 2, d, normalize=False)
    ix = build(x, "f32")
    try:
        D0, I0 = ix.search(q, 10)
        lib, removed = native.load(), ctypes.c_int64(-7)
        bm = np.full(n // 8, 0xff, np.uint8)
        assert lib.ls_remove(ix._handle, None, 5, ctypes.byref(removed)) == native.LS_ERR_INVALID_ARG
        assert lib.ls_remove(ix._handle, bm.ctypes.data, -1, ctypes.byref(removed)) == native.LS_ERR_INVALID_ARG
        assert lib.ls_remove_set_slab_rows(ix._handle, -5) == native.LS_ERR_INVALID_ARG
        assert lib.ls_subset_rows(ix._handle, 99, ctypes.byref(removed)) == native.LS_ERR_INVALID_ARG
        for bad in (np.zeros(n + 1, bool), np.array([0.5])):
            with pytest.raises(ValueError):
                ix.remove_ids(bad)
        assert removed.value == -7 and ix.ntotal == n and native.load().ls_ntotal(ix._handle) == n
        assert np.array_equal(ix.host_corpus(), x)
        D, I = ix.search(q, 10)
        assert np.array_equal(I, I0) and np.array_equal(D, D0)
    finally:
        ix.close()


@pytest.mark.parametrize("kind", ["IndexFlatIP", "IndexIVFFlat", "IndexScalarQuantizer"])
def test_faiss_surface(kind, tmp_path):
    n, d = 6000, 64
    x, q = H.gauss(87, n, d), H.gauss(88, 5, d, normalize=False)
    ix = {"IndexFlatIP": lambda: fc.IndexFlatIP(d), "IndexIVFFlat": lambda: fc.IndexIVFFlat(None, d, 16),
          "IndexScalarQuantizer": lambda: fc.IndexScalarQuantizer(d)}[kind]()
    ref = back = None
    try:
        if kind != "IndexFlatIP":
            ix.train(x)
        ix.add(x)
        ix.search(q, 10)  # builds the handle
        before, keep = ix.host_corpus(), np.ones(n, bool)
        bits = np.zeros(n, bool)
        bits[::7] = True
        # (selection, the positions it names in the numbering of the moment; the bitmap is longer than the index by then)
        for sel, pos in ((np.arange(n) % 5 == 0, np.arange(0, n, 5)), (np.array([3, 3, 17, 10**9, -1]), [3, 17]),
                         (fc.IDSelectorRange(100, 400), range(100, 400)),
                         (fc.IDSelectorBatch([0, 1, 1, 4000]), [0, 1, 4000]),
                         (fc.IDSelectorBitmap(np.packbits(bits, bitorder="little")), None)):
            alive = np.flatnonzero(keep)
            pos = np.flatnonzero(bits[:alive.size]) if pos is None else np.array(list(pos))
            assert ix.remove_ids(sel) == pos.size
            keep[alive[pos]] = False
            assert ix.ntotal == keep.sum()
        ref = fresh_like(ix, before, keep)
        same_stored(ix, ref)
        same_searches(ix, ref, q)
        fc.write_index(ix, tmp_path / "ix.index", allow_lossy=kind == "IndexScalarQuantizer")
        back = fc.read_index(tmp_path / "ix.index")
        assert back.ntotal == keep.sum() and np.array_equal(back.host_corpus(), ix.host_corpus())
        assert np.array_equal(ix.host_corpus(), before[keep])
    finally:
        for i in (ix, ref, back):
            if i is not None:
                i.close()
