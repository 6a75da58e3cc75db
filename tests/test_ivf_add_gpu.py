"""``add`` on a built IVF index on the MI355X (include/leansearch_ivf_add.h, ``IVFFlatIndex.add`` after a search): the
lists are merged in HBM. Every case builds two indices and demands ``np.array_equal`` between them: the ORACLE is built
from scratch from rows A followed by rows B, the SUBJECT is built from A and then gets ``add(B)``. Compared: ntotal,
list sizes, assignment, the stored rows read back, and search results for nq in {1, 5}, k in {1, 10, 100}, nprobe in
{1, 4, nlist}. Corpora are seeded Gaussians of a few thousand rows, made once per shape."""

import ctypes
import functools

import numpy as np
import pytest

from lean_explore_amd import faiss_compat, native
from lean_explore_amd.id_selectors import SearchParametersIVF
from lean_explore_amd.ivf import IVFFlatIndex

pytestmark = pytest.mark.gpu

NA, NB, NLIST = 3000, 1500, 16


@functools.lru_cache(maxsize=None)
def shape(d, seed=7, na=NA, nb=NB, nlist=NLIST):
    """(A, B, centroids, queries): seeded Gaussian rows. Row 0 of A holds every column's largest magnitude over A and B,
    so that an sq8 step trained on A alone is the step trained on A and B together: one set of codes either way."""
    rng = np.random.default_rng(seed * 1000 + d)
    x = rng.standard_normal((na + nb, d), dtype=np.float32)
    x[0] = np.abs(x).max(axis=0) * np.where(rng.random(d) < 0.5, -1.0, 1.0).astype(np.float32)
    cent = rng.standard_normal((nlist, d), dtype=np.float32)
    q = rng.standard_normal((5, d), dtype=np.float32)
    for a in (x, cent, q):
        a.setflags(write=False)
    return x[:na], x[na:], cent, q


def lists(n, seed, choices):
    return np.random.default_rng(seed).choice(np.asarray(choices, dtype=np.int32), n).astype(np.int32)


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


# ---- 1. every storage shape: the row mover copies rows of `chunks` 16-byte chunks as stored ---------------------------
@pytest.mark.parametrize("dtype,d", [("f32", 384), ("f32", 100), ("f32", 1024), ("f16", 384), ("sq8", 384), ("sq8", 20),
                                     ("f32", 64), ("f32", 256), ("f32", 512), ("f32", 768)])
def test_add_equals_the_index_built_from_all_rows(dtype, d):
    A, B, cent, q = shape(d)
    aA, aB = lists(NA, 1, range(NLIST)), lists(NB, 2, range(NLIST))
    sub = built(cent, A, aA, dtype)
    ora = built(cent, np.concatenate([A, B]), np.concatenate([aA, aB]), dtype)
    try:
        sub.search(q, 10)  # (the index has served a search before the add)
        sub.set_profiling(True)
        sub.add(B, assign=aB)
        ms, nbytes = sub.last_add_kernel_ms()
        row_bytes = {"f32": 4, "f16": 2, "sq8": 1}[dtype] * d
        assert ms > 0.0 and nbytes >= 2 * (NA + NB) * row_bytes and nbytes % (32 * (NA + NB)) == 0, (ms, nbytes)
        sub.set_profiling(False)
        assert_same(sub, ora, q)
    finally:
        close_all(sub, ora)


# ---- 2. list shapes, through explicit lists (fp32, d = 384) -----------------------------------------------------------------
def test_lists_empty_on_either_side_or_both():
    """A fills lists 0-7, B lists 4-11: 8-11 are empty in A and filled by B, 0-3 have A rows and no B rows, 12-15 are
    empty in both."""
    A, B, cent, q = shape(384)
    aA, aB = lists(NA, 3, range(0, 8)), lists(NB, 4, range(4, 12))
    sub = built(cent, A, aA)
    ora = built(cent, np.concatenate([A, B]), np.concatenate([aA, aB]))
    try:
        sub.add(B, assign=aB)
        sizes = sub.list_sizes()
        assert (sizes[:12] > 0).all() and (sizes[12:] == 0).all()
        assert_same(sub, ora, q)
    finally:
        close_all(sub, ora)


def test_one_row_zero_rows_and_two_adds_in_a_row():
    A, B, cent, q = shape(384)
    aA, aB = lists(NA, 5, range(NLIST)), lists(NB, 6, range(NLIST))
    sub = built(cent, A, aA)
    oraA = built(cent, A, aA)
    ora1 = built(cent, np.concatenate([A, B[:1]]), np.concatenate([aA, aB[:1]]))
    ora = built(cent, np.concatenate([A, B]), np.concatenate([aA, aB]))
    try:
        sub.add(B[:0], assign=aB[:0])  # nothing
        rc = native.load().ls_ivf_add(sub._handle, None, 0, None)  # ... and the library's own answer to nothing
        assert rc == native.LS_OK
        assert_same(sub, oraA, q, ks=(10,))
        sub.add(B[:1], assign=aB[:1])  # |B| = 1
        assert_same(sub, ora1, q, ks=(10,))
        sub.add(B[1:700], assign=aB[1:700])  # B1 ...
        sub.add(B[700:], assign=aB[700:])    # ... then B2
        assert_same(sub, ora, q)
    finally:
        close_all(sub, oraA, ora1, ora)


def test_add_to_a_handle_created_empty():
    A, B, cent, q = shape(384)
    aB = lists(NB, 8, range(NLIST))
    sub = new_index(cent)
    sub._ensure_built()  # ls_ivf_create with n = 0
    ora = built(cent, B, aB)
    try:
        assert sub.ntotal == 0 and sub.search(q, 3)[1].max() == -1
        sub.add(B, assign=aB)
        assert_same(sub, ora, q)
    finally:
        close_all(sub, ora)


# ---- 3. the default assignment ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build_on_device", [False, True])
def test_default_assignment_is_ls_ivf_creates_rule(build_on_device):
    A, B, cent, q = shape(384)
    sub = new_index(cent, build_on_device=build_on_device)
    sub.add(A)
    sub._ensure_built()
    ora = new_index(cent)
    ora.add(np.concatenate([A, B]))
    ora._ensure_built()
    try:
        sub.add(B)
        want = np.zeros(NB, np.int32)
        native.check(native.load().ls_ivf_assign(B.ctypes.data, NB, 384, cent.ctypes.data, NLIST, want.ctypes.data, 0))
        assert np.array_equal(sub.assignment()[NA:], want)
        assert_same(sub, ora, q)
        with pytest.raises(ValueError, match="either every add"):
            sub.add(B[:3], assign=want[:3])
        assert sub.ntotal == NA + NB
    finally:
        close_all(sub, ora)


# ---- 4. subsets ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "sq8"])
def test_a_subset_made_before_the_add_stays_valid_and_one_made_after_covers_both(dtype):
    A, B, cent, q = shape(384)
    aA, aB = lists(NA, 9, range(0, 12)), lists(NB, 10, range(6, NLIST))
    rng = np.random.default_rng(11)
    half = np.zeros(NA, bool)
    half[rng.choice(NA, NA // 2, replace=False)] = True
    sub = built(cent, A, aA, dtype)
    ora = built(cent, np.concatenate([A, B]), np.concatenate([aA, aB]), dtype)
    try:
        before = sub.subset(half)
        sizes_before = before.list_sizes()
        assert before.rows == NA // 2 and np.array_equal(sizes_before, np.bincount(aA[half], minlength=NLIST))
        sub.add(B, assign=aB)
        assert before.valid and before.rows == NA // 2 and np.array_equal(before.list_sizes(), sizes_before)
        same_rows = np.concatenate([half, np.zeros(NB, bool)])  # zero bits for B
        both = np.zeros(NA + NB, bool)
        both[rng.choice(NA + NB, (NA + NB) // 3, replace=False)] = True
        after = sub.subset(both)
        assert both[:NA].any() and both[NA:].any() and after.rows == both.sum()
        for k in (1, 10, 100):
            for nprobe in (1, 4, NLIST):
                for s, mask in ((before, same_rows), (after, both)):
                    Ds, Is = sub.search(q, k, params=SearchParametersIVF(nprobe=nprobe, sel=s))
                    Do, Io = ora.search_subset(q, k, mask, nprobe=nprobe)
                    assert np.array_equal(Is, Io), (k, nprobe, s is after)
                    assert np.array_equal(Ds.view(np.uint32), Do.view(np.uint32)), (k, nprobe, s is after)
                    assert (Is[Is >= 0] < NA).all() or s is after
    finally:
        close_all(sub, ora)


# ---- 5. the small-batch pass --------------------------------------------------------------------------------------------
def test_small_batch_pass_serves_the_index_after_the_add():
    """|A| = 6000, |B| = 3000, nlist = nprobe = 8: the group bound stays above the pass's 4096-row floor on both sides of
    the add, so the union pass serves the call before and after it."""
    d, nlist, na, nb = 128, 8, 6000, 3000
    rng = np.random.default_rng(21)
    x = rng.standard_normal((na + nb, d), dtype=np.float32)
    cent = rng.standard_normal((nlist, d), dtype=np.float32)
    q = rng.standard_normal((6, d), dtype=np.float32)
    a = lists(na + nb, 22, range(nlist))
    par = SearchParametersIVF(nprobe=8)
    sub = built(cent, x[:na], a[:na], small_batch=True)  # (switched on before the add)
    ora = built(cent, x, a, small_batch=True)
    plain = built(cent, x, a)
    try:
        sub.search(q, 10, params=par)
        assert sub.last_passes()[0] >= 1
        sub.add(x[na:], assign=a[na:])
        Ds, Is = sub.search(q, 10, params=par)
        assert sub.last_passes()[0] >= 1, "the union pass served the call, not the per-query chain"
        Do, Io = ora.search(q, 10, params=par)
        assert ora.last_passes() == sub.last_passes()
        Dp, Ip = plain.search(q, 10, params=par)
        assert np.array_equal(Is, Io) and np.array_equal(Ds.view(np.uint32), Do.view(np.uint32))
        assert np.array_equal(Is, Ip) and np.array_equal(Ds.view(np.uint32), Dp.view(np.uint32))
        assert (Is >= na).any(), "no added row among the results: the case shows nothing"
    finally:
        close_all(sub, ora, plain)


# ---- 6. a refused add leaves the handle as it was -------------------------------------------------------------------------
def test_a_refused_add_changes_nothing():
    A, B, cent, q = shape(384)
    aA = lists(NA, 12, range(NLIST))
    sub = built(cent, A, aA)
    try:
        par = SearchParametersIVF(nprobe=4)
        sizes, (D0, I0) = sub.list_sizes(), sub.search(q, 10, params=par)
        bad = lists(NB, 13, range(NLIST))
        bad[7] = NLIST
        with pytest.raises(ValueError, match="assign must name"):
            sub.add(B, assign=bad)  # the wrapper's own check
        lib = native.load()
        rc = lib.ls_ivf_add(sub._handle, B.ctypes.data, NB, bad.ctypes.data)  # ... and the library's
        assert rc == native.LS_ERR_INVALID_ARG
        assert b"assign[7] = 16" in lib.ls_last_error(), lib.ls_last_error()
        assert lib.ls_ivf_add(sub._handle, None, 5, None) == native.LS_ERR_INVALID_ARG
        assert sub.ntotal == NA and lib.ls_ivf_ntotal(sub._handle) == NA
        assert np.array_equal(sub.list_sizes(), sizes) and np.array_equal(sub.assignment(), aA)
        D1, I1 = sub.search(q, 10, params=par)
        assert np.array_equal(I1, I0) and np.array_equal(D1.view(np.uint32), D0.view(np.uint32))
    finally:
        sub.close()


# ---- 7. the faiss surface -----------------------------------------------------------------------------------------------
def test_faiss_surface_add_after_search_then_write_and_read_back(tmp_path):
    d, nlist, na, nb = 64, 8, 600, 300
    rng = np.random.default_rng(31)
    x = rng.standard_normal((na + nb, d), dtype=np.float32)
    q = rng.standard_normal((5, d), dtype=np.float32)
    ix = faiss_compat.IndexIVFFlat(None, d, nlist, ivf=True)
    back = None
    try:
        ix.train(x[:na])
        ix.add(x[:na])
        ix.nprobe = 3
        ix.search(q, 10)
        ix.add(x[na:])
        assert ix.ntotal == na + nb
        faiss_compat.write_index(ix, tmp_path / "added.index")
        back = faiss_compat.read_index(tmp_path / "added.index", ivf=True)
        assert back.ntotal == na + nb and back.nprobe == 3
        assert np.array_equal(back.assignment(), ix.assignment())
        assert np.array_equal(back.reconstruct_n(), ix.reconstruct_n()) and np.array_equal(back.reconstruct_n(), x)
        for k in (1, 10, 100):
            Db, Ib = back.search(q, k)
            Di, Ii = ix.search(q, k)
            assert np.array_equal(Ib, Ii) and np.array_equal(Db.view(np.uint32), Di.view(np.uint32)), k
    finally:
        ix.close()
        if back is not None:
            back.close()
