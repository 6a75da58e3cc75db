"""The L2 metric on the IVF index without a GPU (include/leansearch_ivf_l2.h): the ABI surface, the
refusals that come before any device check, the IwFl round trip of an L2 index on host bytes, and the host reference of
the definition (probe by tests/l2_ref.c distances to the centroids, then the flat L2 order over the probed lists' rows)
against float64. Everything tests/test_ivf_l2_gpu.py shares lives here."""

import ctypes
import re
import struct
from pathlib import Path

import numpy as np
import pytest

from lean_explore_amd import faiss_compat, native
from lean_explore_amd.index import FlatL2Index
from lean_explore_amd.ivf import IVFFlatIndex
from tests import helpers as H
from tests.test_geometry_cpu import NQ, geom_of, uneven_assignment
from tests.test_l2_cpu import FMAX, REF_DIMS, exact_topk_l2, query_seen, range_l2, ref_dists, stored_values

ROOT = Path(__file__).resolve().parent.parent
IVF_L2_HEADER = ROOT / "include" / "leansearch_ivf_l2.h"
HEADER_OFF_METRIC = 4 + 4 + 8 + 8 + 8 + 1  # fourcc, d, ntotal, two dummies, is_trained -> metric_type


# ---- shared with tests/test_ivf_l2_gpu.py ---------------------------------------------------------------------------------
def probe_l2(cent, q, nprobe, normalize):
    """[nq, min(nprobe, nlist)] probed lists of the definition: the centroids count as an f32 corpus, the order is
    (distance ascending, list ascending), a centroid whose distance is NaN or >= FLT_MAX is never probed (-1)."""
    dc = ref_dists(cent, "f32", query_seen(q, normalize, "f32"))
    return np.stack([exact_topk_l2(dv, min(nprobe, cent.shape[0]))[1] for dv in dc]), dc


def probed_rows(assign, lists):
    return np.flatnonzero(np.isin(assign, lists[lists >= 0]))


def ivf_l2_reference(corpus, cent, assign, q, k, nprobe, normalize, dtype, dists=None, among=None):
    """The definition on the host. Returns (D, I, rows of every query). dists: ref_dists(corpus, dtype, query_seen(q,
    normalize, dtype)) to reuse; among: an ascending row list the result is restricted to (a subset)."""
    P, _ = probe_l2(cent, q, nprobe, normalize)
    dv = ref_dists(corpus, dtype, query_seen(q, normalize, dtype)) if dists is None else dists
    D = np.empty((q.shape[0], k), np.float32)
    I = np.empty((q.shape[0], k), np.int64)
    rows_of = []
    for i in range(q.shape[0]):
        rows = probed_rows(assign, P[i])
        if among is not None:
            rows = np.intersect1d(rows, among)
        D[i], I[i] = exact_topk_l2(dv[i][rows], k, rows)
        rows_of.append(rows)
    return D, I, rows_of


def ivf_l2_range_reference(dists, rows_of, radius):
    """(lims, D, I) of the definition over every query's probed rows."""
    lims, Ds, Is = [0], [], []
    for dv, rows in zip(dists, rows_of):
        _, Dq, Iq = range_l2(dv[None, :], radius, rows)
        Ds.append(Dq)
        Is.append(Iq)
        lims.append(lims[-1] + Dq.size)
    return np.array(lims, np.uint64), np.concatenate(Ds).astype(np.float32), np.concatenate(Is).astype(np.int64)


def nearest_l2(cent, x):
    """The default assignment on the host: the k = 1 L2 search of the centroids with the row as the query (ties to the
    lowest list, no valid distance: list 0)."""
    dc = ref_dists(cent, "f32", np.ascontiguousarray(x, np.float32))
    a = np.array([exact_topk_l2(dv, 1)[1][0] for dv in dc], np.int64)
    a[a < 0] = 0
    return a.astype(np.int32)


# ---- 1: the header against native.IVF_L2_SYMBOLS (fails on a library without the feature) ---------------------------------
def test_header_symbols_and_null_metric():
    text = re.sub(r"/\*.*?\*/", "", IVF_L2_HEADER.read_text(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ls_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(native.IVF_L2_SYMBOLS) == ["ls_ivf_assign_l2", "ls_ivf_create_l2", "ls_ivf_metric",
                                                      "ls_ivf_trainer_create_l2"]
    raw = ctypes.CDLL(str(native.LIB_PATH))
    lib = native.load()
    for n in names:
        assert hasattr(raw, n), f"{n} is not exported"
        assert getattr(lib, n).argtypes == native.IVF_L2_SYMBOLS[n][1]
        assert getattr(lib, n).restype == native.IVF_L2_SYMBOLS[n][0]
    assert lib.ls_ivf_metric(None) == -1
    # the creator has ls_ivf_create's signature, the trainer ls_ivf_trainer_create's, the assignment ls_ivf_assign's
    assert native.IVF_L2_SYMBOLS["ls_ivf_create_l2"] == native.IVF_SYMBOLS["ls_ivf_create"]
    assert native.IVF_L2_SYMBOLS["ls_ivf_trainer_create_l2"] == native.IVF_BUILD_SYMBOLS["ls_ivf_trainer_create"]
    assert native.IVF_L2_SYMBOLS["ls_ivf_assign_l2"] == native.IVF_BUILD_SYMBOLS["ls_ivf_assign"]
    # the flat header no longer says that IVF indexes are inner-product only
    assert "leansearch_ivf_l2.h" in (ROOT / "include" / "leansearch_l2.h").read_text()


# ---- 2: the refusals, before any device check (device 9999 exists nowhere) ------------------------------------------------
def test_refusals_come_before_the_device_check():
    lib = native.load()
    x = np.ones((4, 8), np.float32)
    cent = np.ones((2, 8), np.float32)
    h = ctypes.c_void_p()
    rc = lib.ls_ivf_create_l2(ctypes.byref(h), x.ctypes.data, 4, 8, native.LS_DTYPE_SQ8, cent.ctypes.data, 2, None, 9999)
    assert rc == native.LS_ERR_INVALID_ARG and b"L2" in lib.ls_last_error() and not h.value
    for dtype in (native.LS_DTYPE_F32, native.LS_DTYPE_F16):  # (these get as far as the device check)
        rc = lib.ls_ivf_create_l2(ctypes.byref(h), x.ctypes.data, 4, 8, dtype, cent.ctypes.data, 2, None, 9999)
        assert rc == native.LS_ERR_NO_DEVICE and not h.value
    a = np.zeros(4, np.int32)
    assert lib.ls_ivf_assign_l2(x.ctypes.data, 4, 8, cent.ctypes.data, 2, a.ctypes.data, 9999) == native.LS_ERR_NO_DEVICE
    assert lib.ls_ivf_assign_l2(x.ctypes.data, 4, 8, cent.ctypes.data, 8192, a.ctypes.data, 9999) == native.LS_ERR_INVALID_ARG
    assert lib.ls_ivf_trainer_create_l2(ctypes.byref(h), x.ctypes.data, 4, 8, 2, 9999) == native.LS_ERR_NO_DEVICE
    assert lib.ls_ivf_trainer_create_l2(ctypes.byref(h), x.ctypes.data, 4, 1025, 2, 9999) == native.LS_ERR_INVALID_ARG


# ---- 3: the Python refusals -------------------------------------------------------------------------------------------------
def test_python_refusals_touch_no_device():
    ix = IVFFlatIndex(8, 4, metric="l2", device=9999)
    assert ix.metric == "l2" and IVFFlatIndex(8, 4).metric == "ip" and IVFFlatIndex(8, 4, metric=1).metric == "l2"
    assert IVFFlatIndex(8, 4, dtype="f16", metric="l2").storage_dtype == "f16"
    with pytest.raises(ValueError, match="l2"):
        IVFFlatIndex(8, 4, dtype="sq8", metric="l2", device=9999)
    with pytest.raises(ValueError, match="L2"):
        IVFFlatIndex(8, 4, small_batch=True, metric="l2", device=9999)
    with pytest.raises(ValueError, match="L2"):
        ix.set_small_batch(True)
    ix.set_small_batch(False)  # (switching it off is always allowed)
    with pytest.raises(ValueError):
        IVFFlatIndex(8, 4, metric="cosine")
    l2 = faiss_compat.IndexIVFFlatL2(faiss_compat.IndexFlatL2(8), 8, 4, dtype="f16")
    assert isinstance(l2, IVFFlatIndex) and (l2.metric, l2.d, l2.nlist, l2.storage_dtype) == ("l2", 8, 4, "f16")
    with pytest.raises(ValueError):
        faiss_compat.IndexIVFFlatL2(None, 8, 4, dtype="sq8")
    # IndexIVFFlat itself keeps refusing METRIC_L2 with its present message
    for kw in (dict(), dict(ivf=True)):
        with pytest.raises(ValueError, match="only METRIC_INNER_PRODUCT is supported"):
            faiss_compat.IndexIVFFlat(None, 8, 4, faiss_compat.METRIC_L2, **kw)


# ---- 4: the IwFl round trip of an L2 index on host bytes ------------------------------------------------------------------
def test_iwfl_round_trip_of_an_l2_index(tmp_path):
    n, d, nlist = 61, 24, 7
    x = H.gauss(5, n, d, normalize=False)
    cent = H.gauss(6, nlist, d, normalize=False)
    assign = (np.arange(n) * 5 % nlist).astype(np.int32)
    assign[assign == 3] = 4  # (list 3 is empty)
    ix = IVFFlatIndex(d, nlist, metric="l2", device=9999)
    ix.set_centroids(cent)
    ix.add(x, assign=assign)
    ix.nprobe = 3
    p = tmp_path / "ivf_l2.index"
    faiss_compat.write_index(ix, p)  # (unbuilt and every add named its lists: nothing reaches a device)
    raw = p.read_bytes()
    assert raw[:4] == b"IwFl"
    assert struct.unpack_from("<i", raw, HEADER_OFF_METRIC)[0] == faiss_compat.METRIC_L2
    nested = 4 + 33 + 16  # the outer header, then nlist and nprobe
    assert struct.unpack_from("<QQ", raw, 4 + 33) == (nlist, 3)
    assert raw[nested:nested + 4] == b"IxF2"
    assert struct.unpack_from("<i", raw, nested + HEADER_OFF_METRIC)[0] == faiss_compat.METRIC_L2
    back = faiss_compat.read_index(p, ivf=True, device=9999)
    assert isinstance(back, IVFFlatIndex) and back.metric == "l2" and (back.d, back.nlist, back.ntotal) == (d, nlist, n)
    assert back.nprobe == 3 and np.array_equal(back.centroids, cent)
    assert np.array_equal(np.concatenate(back._assign), assign) and np.array_equal(back.reconstruct_n(), x)
    p2 = tmp_path / "again.index"
    faiss_compat.write_index(back, p2)
    assert p2.read_bytes() == raw
    assert faiss_compat.read_index(p, ivf=True, dtype="f16", device=9999).storage_dtype == "f16"
    with pytest.raises(ValueError, match="not an inner-product index"):
        faiss_compat.read_index(p)
    with pytest.raises(ValueError):
        faiss_compat.read_index(p, ivf=True, ivf_small_batch=True)
    # an inner-product IVF index still writes METRIC_INNER_PRODUCT and a nested IxFI, and reads back as one
    ip = IVFFlatIndex(d, nlist, device=9999)
    ip.set_centroids(cent)
    ip.add(x, assign=assign)
    p3 = tmp_path / "ivf_ip.index"
    faiss_compat.write_index(ip, p3)
    raw3 = p3.read_bytes()
    assert struct.unpack_from("<i", raw3, HEADER_OFF_METRIC)[0] == 0 and raw3[nested:nested + 4] == b"IxFI"
    assert faiss_compat.read_index(p3, ivf=True, device=9999).metric == "ip"
    assert len(raw3) == len(raw)


# ---- 5: the host reference alone against float64 ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, d", [(t, d) for t in ("f32", "f16") for d in REF_DIMS[t] if d <= 1024])
def test_ivf_l2_reference_alone_against_float64(dtype, d):
    """ivf_l2_reference on one small shape per geometry against a float64 brute force: the probed lists are recomputed
    from float64 centroid distances (the Gaussian data has no near ties among them: asserted), every query returns
    min(k, rows) real rows in distance order, every distance is within the bound of
    test_l2_cpu.py::test_restatement_on_gaussian_data_against_float64 of the float64 distance of ITS row, and the
    returned set is the float64 top-k up to rows whose float64 distances are within that bound of the cut."""
    import math

    n, nlist, k, nprobe = 600, 37, 30, 5
    L, V = geom_of(dtype, d)
    per = {"f32": 4, "f16": 8}[dtype]
    rel = (per * V + math.log2(L) + 3) * 2.0 ** -24
    Lc, Vc = geom_of("f32", d)  # the centroids are an f32 corpus
    rel_c = (4 * Vc + math.log2(Lc) + 3) * 2.0 ** -24
    corpus = H.gauss(1, n, d, normalize=False)
    cent = H.gauss(2, nlist, d, normalize=False)
    assign = uneven_assignment(n, nlist)
    q = H.gauss(3, NQ, d, normalize=False) * np.float32(2.5)
    assert np.bincount(assign, minlength=nlist)[[0, 20, 36]].tolist() == [0, 0, 1]
    for normalize in (False, True):
        D, I, rows_of = ivf_l2_reference(corpus, cent, assign, q, k, nprobe, normalize, dtype)
        qc = query_seen(q, normalize, "f32").astype(np.float64)   # the coarse stage stays f32
        qf = query_seen(q, normalize, dtype).astype(np.float64)   # the fine stage sees the dtype's query
        x64 = stored_values(corpus, dtype).astype(np.float64)
        for i in range(NQ):
            dc = ((cent.astype(np.float64) - qc[i][None, :]) ** 2).sum(axis=1)
            order = np.argsort(dc, kind="stable")
            # (no near tie at the cut: the gap is beyond twice the f32 restatement's error of either distance)
            assert dc[order[nprobe]] - dc[order[nprobe - 1]] > 4 * rel_c * dc[order[nprobe]]
            rows = np.flatnonzero(np.isin(assign, order[:nprobe]))
            assert np.array_equal(rows, rows_of[i]) and 0 < rows.size < n
            m = min(k, rows.size)
            assert (I[i] >= 0).sum() == m and (I[i][m:] == -1).all() and (D[i][m:] == FMAX).all()
            assert np.isin(I[i][:m], rows).all() and np.unique(I[i][:m]).size == m
            want = ((x64[I[i][:m]] - qf[i][None, :]) ** 2).sum(axis=1)
            assert (np.abs(D[i][:m].astype(np.float64) - want) <= rel * want).all()
            assert (np.diff(D[i][:m]) >= 0).all()
            all64 = ((x64[rows] - qf[i][None, :]) ** 2).sum(axis=1)
            cut = np.sort(all64)[m - 1]
            assert (want <= cut * (1 + 2 * rel)).all()
    # every list probed: the flat reference over all rows
    dv = ref_dists(corpus, dtype, query_seen(q, True, dtype))
    Da, Ia, _ = ivf_l2_reference(corpus, cent, assign, q, k, nlist, True, dtype, dists=dv)
    for i in range(NQ):
        Df, If = exact_topk_l2(dv[i], k)
        assert np.array_equal(Da[i], Df) and np.array_equal(Ia[i], If)


def test_probe_order_ties_and_invalid_centroids():
    """The probe order of the reference on hand-made centroids: identical centroids keep the lower list at the cut, a
    NaN and an inf centroid are never probed."""
    d = 8
    cent = np.zeros((6, d), np.float32)
    cent[0] = cent[1] = 1.0
    cent[2] = cent[3] = 2.0
    cent[4, 0] = np.nan
    cent[5, 0] = np.inf
    q = np.full((1, d), 1.25, np.float32)
    P, dc = probe_l2(cent, q, 6, False)
    assert P[0].tolist() == [0, 1, 2, 3, -1, -1] and np.isnan(dc[0][4]) and dc[0][5] == np.inf
    assert probe_l2(cent, q, 3, False)[0][0].tolist() == [0, 1, 2]
    assert probe_l2(cent, q, 1, False)[0][0].tolist() == [0]
    assert nearest_l2(cent[:4], np.stack([cent[2], np.full(d, np.nan, np.float32)])).tolist() == [2, 0]


def test_the_l2_index_keeps_an_l2_quantizer_class():
    ix = IVFFlatIndex(8, 2, metric="l2", device=9999)
    ix.set_centroids(np.ones((2, 8), np.float32))
    q = ix.quantizer  # (buffers the centroids: no device until it is searched)
    assert isinstance(q, FlatL2Index) and q.metric == "l2" and q.ntotal == 2
