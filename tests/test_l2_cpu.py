"""The L2 metric without a GPU (include/leansearch_l2.h): the ABI surface and the refusals that come
before any device check, the plain-C restatement of a row's distance (tests/l2_ref.c) against integer arithmetic and
against float64, and the IxF2 file round trip on host bytes. Everything tests/test_l2_gpu.py shares lives here."""

import ctypes
import math
import re
import struct
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

from lean_explore_amd import faiss_compat, native
from lean_explore_amd.index import FlatIPIndex, FlatL2Index
from tests import helpers as H
from tests.test_geometry_cpu import DIMS, GEOMS, PER_CHUNK, geom_of, seen_queries

ROOT = Path(__file__).resolve().parent.parent
L2_HEADER = ROOT / "include" / "leansearch_l2.h"
FMAX = np.float32(np.finfo(np.float32).max)


# ---- shared with tests/test_l2_gpu.py -------------------------------------------------------------------------------------
_ref_lib = None
_ref_dir = None


def ref_lib():
    """tests/l2_ref.c, built once per process into a temporary directory."""
    global _ref_lib, _ref_dir
    if _ref_lib is None:
        _ref_dir = tempfile.TemporaryDirectory(prefix="l2_ref_")
        so = Path(_ref_dir.name) / "libl2_ref.so"
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", str(ROOT / "tests" / "l2_ref.c"), "-o",
                        str(so), "-lm"], check=True)
        _ref_lib = ctypes.CDLL(str(so))
        _ref_lib.l2_ref_dists.restype = None
        _ref_lib.l2_ref_dists.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return _ref_lib


def stored_values(x, dtype):
    """What the index holds of float32 values x: themselves, or - f16 - rounded to fp16 and widened again."""
    x = np.ascontiguousarray(x, np.float32)
    return x.astype(np.float16).astype(np.float32) if dtype == "f16" else x


def query_seen(q, normalize, dtype):
    """The query as the kernel sees it: scaled by the LS_FLAG_NORMALIZE factor (the library's summation order), then
    - f16 - rounded to fp16."""
    return stored_values(seen_queries(q, normalize), dtype)


def padded(x, dtype, d):
    """[n, chunks * per] float32: the stored values of x, zero padded to the row geometry of (dtype, d)."""
    L, V = geom_of(dtype, d)
    out = np.zeros((x.shape[0], L * V * PER_CHUNK[dtype]), np.float32)
    out[:, :x.shape[1]] = stored_values(x, dtype)
    return out


def ref_dists(corpus, dtype, qs):
    """Distances [nq, n] of l2_ref.c: corpus float32 [n, d] as added, qs [nq, d] the queries as seen (query_seen)."""
    d = corpus.shape[1]
    L, V = geom_of(dtype, d)
    per = PER_CHUNK[dtype]
    rows = padded(corpus, dtype, d)
    qp = np.zeros((qs.shape[0], rows.shape[1]), np.float32)
    qp[:, :d] = qs
    n = rows.shape[0]
    out = np.empty((qs.shape[0], n), np.float32)
    lib = ref_lib()

    def one(i):
        lib.l2_ref_dists(rows.ctypes.data, n, L * V, L, V, per, qp[i].ctypes.data, out[i].ctypes.data)

    with ThreadPoolExecutor(max_workers=min(16, max(qs.shape[0], 1))) as ex:  # (ctypes releases the GIL)
        list(ex.map(one, range(qs.shape[0])))
    return out


def int_dists(corpus, qs):
    """Plain integer arithmetic on integer-valued data: [nq, n] float32 (every value an exact integer below 2^24)."""
    c, q = corpus.astype(np.int64), qs.astype(np.int64)
    out = ((c * c).sum(axis=1)[None, :] - 2 * (q @ c.T) + (q * q).sum(axis=1)[:, None])
    assert out.min() >= 0 and out.max() < (1 << 24)
    return out.astype(np.float32)


def exact_topk_l2(dists, k, rows=None, base=0):
    """The library's order over one distance vector: distance ascending, row ascending; NaN and >= FLT_MAX rows never
    returned; (+FLT_MAX, -1) padding. rows: the row numbers the distances belong to (default 0..n-1)."""
    dists = np.asarray(dists, np.float32)
    rows = np.arange(dists.shape[0], dtype=np.int64) if rows is None else np.asarray(rows, np.int64)
    ok = dists < FMAX  # (False for NaN)
    s, r = dists[ok], rows[ok]
    order = np.lexsort((r, s.astype(np.float64)))[:k]
    D = np.full(k, FMAX, np.float32)
    I = np.full(k, -1, np.int64)
    D[:order.size], I[:order.size] = s[order], r[order] + base
    return D, I


def topk_l2(dists, k, rows=None, base=0):
    """exact_topk_l2 of every query: dists [nq, n] over all rows, restricted to `rows` where given."""
    out = [exact_topk_l2(dv if rows is None else dv[rows], k, rows, base) for dv in dists]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def range_l2(dists, radius, rows=None, base=0):
    """(lims, D, I) of the definition: dist < radius, valid rows only, rows ascending."""
    lims, Ds, Is = [0], [], []
    for dv in dists:
        r = np.arange(dv.shape[0], dtype=np.int64) if rows is None else np.asarray(rows, np.int64)
        v = dv if rows is None else dv[rows]
        with np.errstate(invalid="ignore"):
            hit = (v < np.float32(radius)) & (v < FMAX)
        Ds.append(v[hit])
        Is.append(r[hit] + base)
        lims.append(lims[-1] + int(hit.sum()))
    return (np.array(lims, np.uint64), np.concatenate(Ds).astype(np.float32) if Ds else np.zeros(0, np.float32),
            np.concatenate(Is).astype(np.int64) if Is else np.zeros(0, np.int64))


REF_DIMS = {dtype: [max(d for d in DIMS[dtype] if geom_of(dtype, d) == g and d % PER_CHUNK[dtype]) for g in GEOMS[dtype]]
            for dtype in ("f32", "f16")}  # one ragged d per geometry


# ---- 1: symbols and refusals (fails on a library without the L2 metric) ----------------------------------------------------
def test_symbols_constants_and_refusals(tmp_path):
    head = L2_HEADER.read_text()
    for name in ("LS_METRIC_INNER_PRODUCT", "LS_METRIC_L2"):
        m = re.search(rf"#define\s+{name}\s+(\d+)", head)
        assert m and int(m.group(1)) == getattr(native, name), name
    assert native.LS_METRIC_L2 == faiss_compat.METRIC_L2 == 1 and native.LS_METRIC_INNER_PRODUCT == 0
    text = re.sub(r"/\*.*?\*/", "", head, flags=re.S)
    names = sorted(set(re.findall(r"\b(ls_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(native.L2_SYMBOLS) == ["ls_create_l2", "ls_create_l2_from_device", "ls_metric"]
    raw = ctypes.CDLL(str(native.LIB_PATH))
    lib = native.load()
    for n in names:
        assert hasattr(raw, n), f"{n} is not exported"
        assert getattr(lib, n).argtypes == native.L2_SYMBOLS[n][1]
    assert lib.ls_metric(None) == -1

    # LS_DTYPE_SQ8 at creation: an argument error, before any device check (device 9999 exists nowhere)
    x = np.ones((4, 8), np.float32)
    h = ctypes.c_void_p()
    for fn in (lib.ls_create_l2, lib.ls_create_l2_from_device):
        assert fn(ctypes.byref(h), x.ctypes.data, 4, 8, native.LS_DTYPE_SQ8, 9999) == native.LS_ERR_INVALID_ARG
        assert b"L2" in lib.ls_last_error() and not h.value
    # (the other dtypes get as far as the device check there)
    assert lib.ls_create_l2(ctypes.byref(h), x.ctypes.data, 4, 8, native.LS_DTYPE_F32, 9999) == native.LS_ERR_NO_DEVICE

    # Python: the metric keyword, the subclass, what it is refused with
    ix = FlatIPIndex(8, metric="l2")
    assert ix.metric == "l2" and FlatIPIndex(8).metric == "ip" and FlatL2Index(8, dtype="f16").metric == "l2"
    assert FlatL2Index(8).storage_dtype == "f32"
    for bad in (dict(devices=[0, 1]), dict(dtype="sq8"), dict(f16_small_batch=True, dtype="f16"),
                dict(sq8_small_batch=True), dict(subset_small_batch=True)):
        with pytest.raises(ValueError):
            FlatIPIndex(8, metric="l2", **bad)
    with pytest.raises(ValueError):
        FlatIPIndex(8, metric="cosine")
    with pytest.raises(ValueError):
        FlatL2Index(8, metric="ip")
    for setter in (ix.set_f16_small_batch, ix.set_sq8_small_batch, ix.set_subset_small_batch):
        with pytest.raises(ValueError):
            setter(True)

    # faiss_compat: IndexFlatL2, IndexFlat, and what keeps refusing METRIC_L2 with its present message
    l2 = faiss_compat.IndexFlatL2(8)
    assert isinstance(l2, FlatL2Index) and l2.metric == "l2" and l2.d == 8 and l2.ntotal == 0
    assert isinstance(faiss_compat.IndexFlat(8, faiss_compat.METRIC_L2), faiss_compat.IndexFlatL2)
    ip = faiss_compat.IndexFlat(8, faiss_compat.METRIC_INNER_PRODUCT)
    assert isinstance(ip, faiss_compat.IndexFlatIP) and ip.metric == "ip"
    with pytest.raises(ValueError):
        faiss_compat.IndexFlat(8, 2)
    with pytest.raises(ValueError, match="only METRIC_INNER_PRODUCT is supported"):
        faiss_compat.IndexIVFFlat(None, 8, 4, faiss_compat.METRIC_L2)
    with pytest.raises(ValueError, match="only METRIC_INNER_PRODUCT is supported"):
        faiss_compat.IndexIVFFlat(None, 8, 4, faiss_compat.METRIC_L2, ivf=True)
    with pytest.raises(ValueError, match="only METRIC_INNER_PRODUCT is supported"):
        faiss_compat.IndexScalarQuantizer(8, faiss_compat.QT_8bit, faiss_compat.METRIC_L2)
    # an IwFl file whose header says L2 stays refused
    p = tmp_path / "ivf_l2.index"
    H.write_ivf_flat(p, np.ones((4, 8), np.float32), np.zeros(4, np.int64), 2)
    raw_bytes = bytearray(p.read_bytes())
    off = 4 + 4 + 8 + 8 + 8 + 1  # fourcc, d, ntotal, two dummies, is_trained -> metric_type
    assert struct.unpack_from("<i", raw_bytes, off)[0] == faiss_compat.METRIC_INNER_PRODUCT
    struct.pack_into("<i", raw_bytes, off, faiss_compat.METRIC_L2)
    p.write_bytes(bytes(raw_bytes))
    with pytest.raises(ValueError, match="not an inner-product index"):
        faiss_compat.read_index(p)


# ---- 2: the restatement is itself correct ----------------------------------------------------------------------------------
def test_reference_dimensions_are_one_per_geometry():
    for dtype in ("f32", "f16"):
        assert sorted(geom_of(dtype, d) for d in REF_DIMS[dtype]) == sorted(GEOMS[dtype])


@pytest.mark.parametrize("dtype, d", [(t, d) for t in ("f32", "f16") for d in REF_DIMS[t]])
def test_restatement_on_integer_data_is_integer_arithmetic(dtype, d):
    """Values -3..3: every difference, square and partial sum is an exact integer below 2^24, in any order."""
    corpus = H.int_corpus(10 + d, 300, d)
    q = H.int_corpus(11 + d, 4, d)
    got = ref_dists(corpus, dtype, query_seen(q, False, dtype))
    assert np.array_equal(got, int_dists(corpus, q))
    # a row against itself: +0.0
    self_d = ref_dists(corpus[:4], dtype, query_seen(corpus[:4], False, dtype))
    assert (np.diag(self_d) == 0).all() and not np.signbit(np.diag(self_d)).any()


@pytest.mark.parametrize("dtype, d", [(t, d) for t in ("f32", "f16") for d in REF_DIMS[t]])
def test_restatement_on_gaussian_data_against_float64(dtype, d):
    """|dist - dist64| <= (m + log2 L + 3) 2^-24 dist64, dist64 the float64 sum over the same rounded operands: one
    rounding for the subtraction (two for its square), m fma steps and log2 L tree adds, all over non-negative terms."""
    L, V = geom_of(dtype, d)
    m = PER_CHUNK[dtype] * V
    corpus = H.gauss(20 + d, 400, d)
    q = H.gauss(21 + d, 4, d)
    q[:2] *= np.float32(2.5)
    for normalize in (False, True):
        qs = query_seen(q, normalize, dtype)
        got = ref_dists(corpus, dtype, qs).astype(np.float64)
        x64 = stored_values(corpus, dtype).astype(np.float64)
        want = np.stack([((x64 - qv[None, :]) ** 2).sum(axis=1) for qv in qs.astype(np.float64)])
        bound = (m + math.log2(L) + 3) * 2.0 ** -24 * want
        assert got.shape == want.shape == (4, 400) and (want >= 0).all()
        assert (np.abs(got - want) <= bound).all(), float((np.abs(got - want) / want).max())


def test_order_and_padding_of_the_host_top_k():
    d = np.array([2.0, 0.0, np.nan, 1.0, np.inf, FMAX, 1.0, 0.0], np.float32)
    D, I = exact_topk_l2(d, 7)
    assert I.tolist() == [1, 7, 3, 6, 0, -1, -1] and D[:5].tolist() == [0, 0, 1, 1, 2] and (D[5:] == FMAX).all()
    lims, Dr, Ir = range_l2(d[None, :], 1.5)
    assert lims.tolist() == [0, 4] and Ir.tolist() == [1, 3, 6, 7]
    assert range_l2(d[None, :], np.inf)[2].tolist() == [0, 1, 3, 6, 7]
    for radius in (0.0, -1.0, -np.inf, np.nan):
        assert range_l2(d[None, :], radius)[0].tolist() == [0, 0]


# ---- 3: the IxF2 container on host bytes -----------------------------------------------------------------------------------
def test_ixf2_file_round_trip(tmp_path):
    x = H.gauss(5, 37, 24, normalize=False)
    ix = faiss_compat.IndexFlatL2(24)
    ix.add(x)
    p = tmp_path / "l2.index"
    faiss_compat.write_index(ix, p)  # (nothing was searched: the rows are still on the host)
    raw = p.read_bytes()
    assert raw[:4] == b"IxF2"
    d, ntotal, _, _, trained, metric = struct.unpack_from("<iqqqBi", raw, 4)
    assert (d, ntotal, trained, metric) == (24, 37, 1, faiss_compat.METRIC_L2)
    assert struct.unpack_from("<Q", raw, 4 + 33)[0] == 37 * 24 and len(raw) == 4 + 33 + 8 + 37 * 24 * 4
    back = faiss_compat.read_index(p)
    assert isinstance(back, faiss_compat.IndexFlatL2) and back.metric == "l2" and (back.d, back.ntotal) == (24, 37)
    assert np.array_equal(back.host_corpus(), x)
    p2 = tmp_path / "l2_again.index"
    faiss_compat.write_index(back, p2)
    assert p2.read_bytes() == raw
    f16 = faiss_compat.read_index(p, dtype="f16")
    assert f16.metric == "l2" and f16.storage_dtype == "f16"
    for bad in (dict(devices=[0, 1]), dict(f16_small_batch=True), dict(sq8_small_batch=True), dict(ivf=True)):
        with pytest.raises(ValueError):
            faiss_compat.read_index(p, **bad)
    # an inner-product index still writes IxFI, and reads back as one
    ipx = faiss_compat.IndexFlatIP(24)
    ipx.add(x)
    p3 = tmp_path / "ip.index"
    faiss_compat.write_index(ipx, p3)
    assert p3.read_bytes()[:4] == b"IxFI" and struct.unpack_from("<i", p3.read_bytes(), 4 + 29)[0] == 0
    assert faiss_compat.read_index(p3).metric == "ip"
