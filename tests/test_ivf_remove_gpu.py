"""``remove_ids`` on a built IVF index on the MI355X (include/leansearch_ivf_remove.h): the lists are compacted in HBM.
Every case builds two indices and demands ``np.array_equal`` between them: the ORACLE is built from scratch from the
surviving rows, the SUBJECT is built from all rows, has served a search and then has rows removed. Compared: ntotal,
list sizes, assignment, the stored rows read back, and search results for nq in {1, 5}, k in {1, 10, 100}, nprobe in
{1, 4, nlist}. Corpora are seeded Gaussians of 4500 rows, made once per shape."""

import ctypes
import functools

import numpy as np
import pytest

from lean_explore_amd import faiss_compat, native
from lean_explore_amd.id_selectors import SearchParametersIVF
from lean_explore_amd.ivf import IVFFlatIndex

pytestmark = pytest.mark.gpu

N, NB, NLIST = 4500, 700, 16
FLT_MAX = np.finfo(np.float32).max


@functools.lru_cache(maxsize=None)
def shape(d, seed=9, n=N, nb=NB, nlist=NLIST):
    """(rows, fresh rows, centroids, queries): seeded Gaussian rows. Row 0 holds every column's largest magnitude over
    all of them and is never removed, so that an sq8 step trained on the survivors is the step trained on all rows: one
    set of codes on both sides."""
    rng = np.random.default_rng(seed * 1000 + d)
    x = rng.standard_normal((n + nb, d), dtype=np.float32)
    x[0] = np.abs(x).max(axis=0) * np.where(rng.random(d) < 0.5, -1.0, 1.0).astype(np.float32)
    cent = rng.standard_normal((nlist, d), dtype=np.float32)
    q = rng.standard_normal((16, d), dtype=np.float32)
    for a in (x, cent, q):
        a.setflags(write=False)
    return x[:n], x[n:], cent, q


def lists(n, seed, choices):
    return np.random.default_rng(seed).choice(np.asarray(choices, dtype=np.int32), n).astype(np.int32)


def some_rows(n, seed, share):
    """A bool mask over n rows with about `share` of them set; row 0 never is."""
    gone = np.random.default_rng(seed).random(n) < share
    gone[0] = False
    return gone


def stored_row_bytes(dtype, d):
    """Bytes of a stored row: 16-byte chunks, padded up to the next row geometry (ls_pick_geom's table)."""
    elem = {"f32": 4, "f16": 2, "sq8": 1}[dtype]
    raw = -(-d * elem // 16)
    sizes = [8, 16, 24, 32, 48, 64, 96, 128, 192, 256] if dtype == "sq8" else [16, 32, 48, 64, 96, 128, 192, 256]
    return 16 * min(c for c in sizes if c >= raw)


def new_index(cent, dtype="f32", **kw):
    ix = IVFFlatIndex(cent.shape[1], cent.shape[0], dtype=dtype, **kw)
    ix.set_centroids(cent)
    return ix


def built(cent, rows, assign, dtype="f32", **kw):
    """An index built from scratch from `rows` (the device object exists when this returns)."""
    ix = new_index(cent, dtype, **kw)
    ix.add(rows, assign=assign)
    ix._ensure_built()
    return ix


def assert_same(sub, ora, q, ks=(1, 10, 100), nqs=(1, 5)):
    assert sub.ntotal == ora.ntotal
    assert native.load().ls_ivf_ntotal(sub._ensure_built()) == ora.ntotal  # (an index read from a file: built here)
    assert np.array_equal(sub.list_sizes(), ora.list_sizes())
    assert np.array_equal(sub.assignment(), ora.assignment())
    assert np.array_equal(sub.reconstruct_n().view(np.uint32), ora.reconstruct_n().view(np.uint32))
    for nq in nqs:
        for k in ks:
            for nprobe in (1, 4, sub.nlist):
                par = SearchParametersIVF(nprobe=nprobe)
                Ds, Is = sub.search(q[:nq], k, params=par)
                Do, Io = ora.search(q[:nq], k, params=par)
                assert np.array_equal(Is, Io), (nq, k, nprobe, np.argwhere(Is != Io)[:5])
                assert np.array_equal(Ds.view(np.uint32), Do.view(np.uint32)), (nq, k, nprobe)


def close_all(*ixs):
    for ix in ixs:
        ix.close()


# ---- 1. every storage shape: the row mover copies rows of `chunks` 16-byte chunks as stored ----------------------------
@pytest.mark.parametrize("dtype,d", [("f32", 384), ("f32", 100), ("f32", 1024), ("f16", 384), ("sq8", 384), ("sq8", 20),
                                     ("f32", 64), ("f32", 256), ("f32", 512), ("f32", 768)])
def test_remove_equals_the_index_built_from_the_survivors(dtype, d):
    x, _, cent, q = shape(d)
    a = lists(N, 1, range(NLIST))
    gone = some_rows(N, 2, 0.30)
    sub = built(cent, x, a, dtype)
    ora = built(cent, x[~gone], a[~gone], dtype)
    try:
        sub.search(q[:5], 10)  # (the index has served a search before the removal)
        sub.set_profiling(True)
        assert sub.remove_ids(gone) == gone.sum()
        ms, nbytes = sub.last_remove_kernel_ms()
        assert ms > 0.0 and nbytes == 2 * int((~gone).sum()) * stored_row_bytes(dtype, d), (ms, nbytes)
        sub.set_profiling(False)
        assert_same(sub, ora, q)
    finally:
        close_all(sub, ora)


# ---- 2. list shapes, through explicit lists (fp32, d = 384) -----------------------------------------------------------------
def test_lists_empty_emptied_untouched_and_trimmed_at_either_end():
    """Lists 2-13 hold the rows; 0, 1, 14 and 15 are empty before the removal. The removal empties list 2 (with it goes
    the first storage row of the index), leaves lists 3 and 4 untouched, takes only the first row of list 5 and only the
    last row of list 6, the last row of list 13 (the last storage row of the index) and a random third of lists 7-13.
    Then a removal of nothing, and a second removal."""
    x, _, cent, q = shape(384)
    a = lists(N, 3, range(2, 14))
    rng = np.random.default_rng(4)
    gone = (a >= 7) & (rng.random(N) < 0.33)
    gone[a == 2] = True
    gone[np.flatnonzero(a == 5)[0]] = True
    gone[np.flatnonzero(a == 6)[-1]] = True
    gone[np.flatnonzero(a == 13)[-1]] = True
    keep = ~gone
    sub = built(cent, x, a)
    ora = built(cent, x[keep], a[keep])
    ora2 = None
    try:
        sub.search(q[:5], 10)
        before = sub.list_sizes()
        assert sub.remove_ids(gone) == gone.sum()
        sizes = sub.list_sizes()
        assert (before[[0, 1, 14, 15]] == 0).all() and before[2] > 0 and sizes[2] == 0
        assert (sizes[[3, 4]] == before[[3, 4]]).all() and (sizes[[5, 6]] == before[[5, 6]] - 1).all()
        assert_same(sub, ora, q)
        # a removal of nothing: 0, and the index equals itself
        removed = ctypes.c_int64(-1)
        assert native.load().ls_ivf_remove(sub._handle, None, 0, ctypes.byref(removed)) == native.LS_OK
        assert removed.value == 0
        assert sub.remove_ids(np.zeros(sub.ntotal, bool)) == 0 and sub.remove_ids(np.array([sub.ntotal, -3])) == 0
        assert_same(sub, ora, q, ks=(10,))
        # two removals in a row
        gone2 = some_rows(int(keep.sum()), 5, 0.10)
        assert sub.remove_ids(np.flatnonzero(gone2)) == gone2.sum()
        ora2 = built(cent, x[keep][~gone2], a[keep][~gone2])
        assert_same(sub, ora2, q)
    finally:
        close_all(sub, ora, *([ora2] if ora2 is not None else []))


def test_one_row_left_in_the_whole_index():
    x, _, cent, q = shape(384)
    a = lists(N, 6, range(NLIST))
    gone = np.ones(N, bool)
    gone[1234] = False
    sub = built(cent, x, a)
    ora = built(cent, x[1234:1235], a[1234:1235])
    try:
        sub.search(q[:5], 10)
        assert sub.remove_ids(gone) == N - 1
        assert_same(sub, ora, q)
        D, I = sub.search(q[:5], 3, params=SearchParametersIVF(nprobe=NLIST))
        assert (I[:, 0] == 0).all() and (I[:, 1:] == -1).all()
    finally:
        close_all(sub, ora)


# ---- 3. remove everything -----------------------------------------------------------------------------------------------
def test_remove_everything_then_add_fresh_rows():
    x, fresh, cent, q = shape(384)
    a, af = lists(N, 7, range(NLIST)), lists(NB, 8, range(NLIST))
    sub = built(cent, x, a)
    ora = built(cent, fresh, af)
    try:
        sub.search(q[:5], 10)
        assert sub.remove_ids(faiss_compat.IDSelectorRange(0, N)) == N
        assert sub.ntotal == 0 and native.load().ls_ivf_ntotal(sub._handle) == 0
        assert (sub.list_sizes() == 0).all() and sub.assignment().size == 0
        D, I = sub.search(q[:5], 10, params=SearchParametersIVF(nprobe=4))
        assert (I == -1).all() and (D == -FLT_MAX).all()
        assert sub.remove_ids(np.zeros(0, bool)) == 0
        sub.add(fresh, assign=af)
        assert_same(sub, ora, q)
    finally:
        close_all(sub, ora)


# ---- 4. remove and add ----------------------------------------------------------------------------------------------------
def test_remove_then_add_and_add_then_remove():
    x, fresh, cent, q = shape(384)
    a, af = lists(N, 9, range(NLIST)), lists(NB, 10, range(NLIST))
    gone = some_rows(N, 11, 0.25)
    sub = built(cent, x, a)
    ora = built(cent, np.concatenate([x[~gone], fresh]), np.concatenate([a[~gone], af]))
    sub2 = built(cent, x, a)
    ora2 = built(cent, x, a)
    try:
        sub.search(q[:5], 10)
        assert sub.remove_ids(gone) == gone.sum()
        sub.add(fresh, assign=af)  # the update: remove the stale rows, add the fresh ones
        assert_same(sub, ora, q)
        sub2.search(q[:5], 10)
        sub2.add(fresh, assign=af)
        assert sub2.remove_ids(faiss_compat.IDSelectorRange(N, N + NB)) == NB  # exactly the added rows
        assert_same(sub2, ora2, q)
    finally:
        close_all(sub, ora, sub2, ora2)


# ---- 5. the default assignment ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build_on_device", [False, True])
def test_default_assignment_survives_the_removal(build_on_device):
    x, fresh, cent, q = shape(384)
    gone = some_rows(N, 12, 0.30)
    sub = new_index(cent, build_on_device=build_on_device)
    sub.add(x)
    sub._ensure_built()
    ora = new_index(cent, build_on_device=build_on_device)
    ora.add(x[~gone])
    ora._ensure_built()
    try:
        sub.search(q[:5], 10)
        assert sub.remove_ids(gone) == gone.sum()
        assert_same(sub, ora, q)
        sub.add(fresh[:50])  # (none of its adds named their lists: the rule holds after the removal)
        ora.add(fresh[:50])
        assert_same(sub, ora, q, ks=(10,))
        with pytest.raises(ValueError, match="either every add"):
            sub.add(fresh[:3], assign=np.zeros(3, np.int32))
    finally:
        close_all(sub, ora)


# ---- 6. subsets ---------------------------------------------------------------------------------------------------------
SIZED = (0, 1, 63, 64, 65, 255, 256, 257, 1000)  # selected rows of lists 0-8 before the removal


def sized_lists_and_selection(seed):
    """(assign, mask): lists 0-8 hold SIZED[l] selected rows and 40 unselected ones each, lists 9-15 share the rest of
    the N rows, about half of them selected; the rows are dealt to the lists in random order."""
    rng = np.random.default_rng(seed)
    a, m = [], []
    for l, s in enumerate(SIZED):
        a += [l] * (s + 40)
        m += [True] * s + [False] * 40
    rest = N - len(a)
    a += list(rng.integers(9, NLIST, rest))
    m += list(rng.random(rest) < 0.5)
    order = rng.permutation(N)
    return np.asarray(a, np.int32)[order], np.asarray(m, bool)[order]


@pytest.mark.parametrize("dtype", ["f32", "sq8"])
def test_subsets_made_before_the_removal_cover_their_survivors(dtype):
    x, _, cent, q = shape(384)
    a, sized = sized_lists_and_selection(13)
    assert tuple(np.bincount(a[sized], minlength=NLIST)[:9]) == SIZED
    gone = some_rows(N, 14, 0.30)
    keep = ~gone
    rng = np.random.default_rng(15)
    masks = {
        "sized": sized,
        "wholly removed": gone & (rng.random(N) < 0.2),
        "untouched": keep & (rng.random(N) < 0.1),
        "empty": np.zeros(N, bool),
    }
    sub = built(cent, x, a, dtype)
    ora = built(cent, x[keep], a[keep], dtype)
    try:
        sub.search(q[:5], 10)
        subsets = {name: sub.subset(m) for name, m in masks.items()}
        assert all(subsets[name].rows == m.sum() for name, m in masks.items())
        assert sub.remove_ids(gone) == gone.sum()
        assert_same(sub, ora, q, ks=(10,))
        after = np.random.default_rng(16).random(int(keep.sum())) < 0.3
        subsets["made after the removal"] = sub.subset(after)
        masks["made after the removal"] = np.zeros(N, bool)
        masks["made after the removal"][np.flatnonzero(keep)[after]] = True
        for name, s in subsets.items():
            want = masks[name][keep]  # the same selection restricted to the survivors, under their new numbers
            o = ora.subset(want)
            assert s.valid and s.rows == o.rows == want.sum(), name
            assert np.array_equal(s.list_sizes(), o.list_sizes()), name
            assert np.array_equal(s.list_sizes(), np.bincount(a[keep][want], minlength=NLIST)), name
            for k in (10, 100):
                for nprobe in (1, 4, NLIST):
                    Ds, Is = sub.search(q[:5], k, params=SearchParametersIVF(nprobe=nprobe, sel=s))
                    Do, Io = ora.search(q[:5], k, params=SearchParametersIVF(nprobe=nprobe, sel=o))
                    assert np.array_equal(Is, Io), (name, k, nprobe)
                    assert np.array_equal(Ds.view(np.uint32), Do.view(np.uint32)), (name, k, nprobe)
                    if name in ("wholly removed", "empty"):
                        assert (Is == -1).all() and (Ds == -FLT_MAX).all(), name
                    elif nprobe == NLIST:
                        assert (Is[:, 0] >= 0).all(), name
            o.close()
        assert subsets["wholly removed"].rows == 0 and subsets["untouched"].rows == masks["untouched"].sum()
    finally:
        close_all(sub, ora)


# ---- 7. the small-batch pass --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [5, 16])
def test_small_batch_pass_serves_the_index_after_the_removal(nq):
    """9000 rows, a third removed, nlist = nprobe = 8: the group bound stays above the pass's 4096-row floor on both
    sides of the removal, so the union pass serves the call before and after it."""
    d, nlist, n = 128, 8, 9000
    rng = np.random.default_rng(21)
    x = rng.standard_normal((n, d), dtype=np.float32)
    cent = rng.standard_normal((nlist, d), dtype=np.float32)
    q = rng.standard_normal((16, d), dtype=np.float32)
    a = lists(n, 22, range(nlist))
    gone = some_rows(n, 23, 1 / 3)
    par = SearchParametersIVF(nprobe=8)
    sub = built(cent, x, a, small_batch=True)  # (switched on before the removal)
    ora = built(cent, x[~gone], a[~gone], small_batch=True)
    plain = built(cent, x[~gone], a[~gone])
    try:
        sub.search(q[:nq], 10, params=par)
        assert sub.last_passes()[0] >= 1
        assert sub.remove_ids(gone) == gone.sum()
        Ds, Is = sub.search(q[:nq], 10, params=par)
        assert sub.last_passes()[0] >= 1, "the union pass served the call, not the per-query chain"
        Do, Io = ora.search(q[:nq], 10, params=par)
        assert ora.last_passes() == sub.last_passes()
        Dp, Ip = plain.search(q[:nq], 10, params=par)
        assert np.array_equal(Is, Io) and np.array_equal(Ds.view(np.uint32), Do.view(np.uint32))
        assert np.array_equal(Is, Ip) and np.array_equal(Ds.view(np.uint32), Dp.view(np.uint32))
    finally:
        close_all(sub, ora, plain)


# ---- 8. a refused removal leaves the handle as it was ---------------------------------------------------------------------
def test_refused_calls_change_nothing():
    x, _, cent, q = shape(384)
    a = lists(N, 24, range(NLIST))
    sub = built(cent, x, a)
    ora = built(cent, x, a)
    try:
        sub.search(q[:5], 10)
        half = sub.subset(some_rows(N, 25, 0.5))
        rows_before = half.rows
        lib = native.load()
        bm = np.full((N + 7) // 8, 0xff, np.uint8)
        removed = ctypes.c_int64(-7)
        for args in ((sub._handle, bm.ctypes.data, -1, ctypes.byref(removed)),
                     (sub._handle, None, bm.size, ctypes.byref(removed)),
                     (None, bm.ctypes.data, bm.size, ctypes.byref(removed))):
            assert lib.ls_ivf_remove(*args) == native.LS_ERR_INVALID_ARG
            assert b"ls_ivf_remove" in lib.ls_last_error()
            assert removed.value == -7 and lib.ls_ivf_ntotal(sub._handle) == N
            assert_same(sub, ora, q, ks=(10,), nqs=(5,))
        with pytest.raises(ValueError, match="bool mask"):
            sub.remove_ids(np.ones(N - 1, bool))  # the wrapper's own check
        assert half.valid and half.rows == rows_before
        assert_same(sub, ora, q, ks=(10,), nqs=(5,))
    finally:
        close_all(sub, ora)


# ---- 9. the faiss surface -----------------------------------------------------------------------------------------------
def test_faiss_surface_remove_ids_then_write_and_read_back(tmp_path):
    d, nlist, n = 64, 8, 900
    rng = np.random.default_rng(31)
    x = rng.standard_normal((n, d), dtype=np.float32)
    q = rng.standard_normal((5, d), dtype=np.float32)
    stale = rng.choice(n, 200, replace=False)
    keep = np.ones(n, bool)
    keep[stale] = False
    ix = faiss_compat.IndexIVFFlat(None, d, nlist, ivf=True)
    ora = back = None
    try:
        ix.train(x)
        ix.add(x)
        ix.nprobe = 3
        ix.search(q, 10)
        lists_before = ix.assignment()
        assert ix.remove_ids(faiss_compat.IDSelectorBatch(np.concatenate([stale, stale[:7], [n + 5]]))) == 200
        assert ix.ntotal == n - 200
        ora = built(ix.centroids, x[keep], lists_before[keep])
        ora.nprobe = 3
        assert_same(ix, ora, q)
        faiss_compat.write_index(ix, tmp_path / "removed.index")
        back = faiss_compat.read_index(tmp_path / "removed.index", ivf=True)
        assert back.ntotal == n - 200 and back.nprobe == 3
        assert np.array_equal(back.reconstruct_n(), x[keep])
        assert_same(back, ora, q)
    finally:
        close_all(*[i for i in (ix, ora, back) if i is not None])
