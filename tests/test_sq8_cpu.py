"""The sq8 storage dtype without a GPU (include/leansearch_sq8.h): the ABI surface, the argument checks
that come before any device check, the host restatement of the codes (lean_explore_amd/sq8.py), the plain-C
restatement of a row's score (tests/sq8_ref.c) and the quality of the definition itself in float64."""

import ctypes
import re
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

from lean_explore_amd import faiss_compat, native, sq8
from lean_explore_amd import search as S
from lean_explore_amd.index import FlatIPIndex
from lean_explore_amd.ivf import IVFFlatIndex
from tests.test_ivf_gpu import mixture, queries

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "leansearch.h"
SQ8_HEADER = ROOT / "include" / "leansearch_sq8.h"
NEG = np.float32(-np.finfo(np.float32).max)


# ---- shared with tests/test_sq8_gpu.py ----------------------------------------------------------------------------------
def geom(d):
    c, L, V = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    rc = native.load().ls_sq8_geom(d, ctypes.byref(c), ctypes.byref(L), ctypes.byref(V))
    return rc, (c.value, L.value, V.value)


_ref_lib = None
_ref_dir = None


def ref_lib():
    """tests/sq8_ref.c, built once per process into a temporary directory."""
    global _ref_lib, _ref_dir
    if _ref_lib is None:
        _ref_dir = tempfile.TemporaryDirectory(prefix="sq8_ref_")
        so = Path(_ref_dir.name) / "libsq8_ref.so"
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", str(ROOT / "tests" / "sq8_ref.c"), "-o",
                        str(so), "-lm"], check=True)
        _ref_lib = ctypes.CDLL(str(so))
        _ref_lib.sq8_ref_scores.restype = None
        _ref_lib.sq8_ref_scores.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_void_p, ctypes.c_void_p]
    return _ref_lib


def padded_codes(codes, chunks):
    out = np.zeros((codes.shape[0], chunks * 16), np.int8)
    out[:, :codes.shape[1]] = codes
    return out


def ref_scores(codes_padded, g, qprime):
    """Scores [nq, n] of sq8_ref.c; qprime [nq, d] float32 (q' = (q * inv) * step), padded here."""
    chunks, L, V = g
    lib = ref_lib()
    n = codes_padded.shape[0]
    qp = np.zeros((qprime.shape[0], chunks * 16), np.float32)
    qp[:, :qprime.shape[1]] = qprime
    out = np.empty((qprime.shape[0], n), np.float32)

    def one(i):
        lib.sq8_ref_scores(codes_padded.ctypes.data, n, chunks, L, V, qp[i].ctypes.data, out[i].ctypes.data)

    with ThreadPoolExecutor(max_workers=min(16, max(qprime.shape[0], 1))) as ex:  # (ctypes releases the GIL)
        list(ex.map(one, range(qprime.shape[0])))
    return out


def exact_topk(scores, k, rows=None):
    """The library's order over one score vector: score descending, row ascending; NaN and <= -FLT_MAX rows never
    returned; (-FLT_MAX, -1) padding. rows: the row numbers the scores belong to (default 0..n-1)."""
    scores = np.asarray(scores, np.float32) + np.float32(0.0)
    rows = np.arange(scores.shape[0], dtype=np.int64) if rows is None else np.asarray(rows, np.int64)
    ok = scores > NEG  # (False for NaN)
    s, r = scores[ok], rows[ok]
    order = np.lexsort((r, -s.astype(np.float64)))[:k]
    D = np.full(k, NEG, np.float32)
    I = np.full(k, -1, np.int64)
    D[:order.size], I[:order.size] = s[order], r[order]
    return D, I


def recall_at(I_got, I_want):
    return float(np.mean([len(set(a) & set(b)) / len(b) for a, b in zip(I_got.tolist(), I_want.tolist())]))


QUALITY = [(5_000, 64, 64, 10, 0.90), (20_000, 384, 141, 50, 0.95)]  # (n, d, nlist, k, floor of mean recall@k)
_quality_data = {}


def quality_data(n, d, nlist):
    if (n, d) not in _quality_data:
        corpus, cent = mixture(1000 + n + d, n, d, nlist)
        q = queries(77 + d, corpus, nq=64)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        _quality_data[(n, d)] = (corpus, cent, np.ascontiguousarray(q, np.float32))
    return _quality_data[(n, d)]


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def test_header_constant_and_symbols():
    m = re.search(r"#define\s+LS_DTYPE_SQ8\s+(\d+)", HEADER.read_text())
    assert m and int(m.group(1)) == native.LS_DTYPE_SQ8 == 2
    text = re.sub(r"/\*.*?\*/", "", SQ8_HEADER.read_text(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ls_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(native.SQ8_SYMBOLS) == ["ls_create_sq8", "ls_sq8_codes", "ls_sq8_geom", "ls_sq8_step"]
    raw = ctypes.CDLL(str(native.LIB_PATH))
    lib = native.load()
    for n in names:
        assert hasattr(raw, n), f"{n} is not exported"
        assert getattr(lib, n).argtypes == native.SQ8_SYMBOLS[n][1]
    assert "QT_8bit" in SQ8_HEADER.read_text()  # the header says what it is not


@pytest.mark.parametrize("d, want", [(64, (8, 8, 1)), (100, (8, 8, 1)), (384, (24, 8, 3)), (768, (48, 16, 3)),
                                     (1024, (64, 16, 4)), (2048, (128, 32, 4)), (4096, (256, 64, 4))])
def test_geometry(d, want):
    assert geom(d) == (native.LS_OK, want)


def test_geometry_refuses_rows_past_4_kib():
    assert geom(4097)[0] == native.LS_ERR_INVALID_ARG
    assert geom(0)[0] == native.LS_ERR_INVALID_ARG


@pytest.mark.parametrize("bad", [0.0, -1.0, np.nan, np.inf])
def test_step_is_validated_before_any_device_check(bad):
    lib = native.load()
    x = np.ones((4, 8), np.float32)
    step = np.ones(8, np.float32)
    step[5] = bad
    h = ctypes.c_void_p()
    # (device 9999 does not exist anywhere: the argument error must come first)
    assert lib.ls_create_sq8(ctypes.byref(h), x.ctypes.data, 4, 8, step.ctypes.data, 9999) == native.LS_ERR_INVALID_ARG
    assert b"step[5]" in lib.ls_last_error()
    with pytest.raises(ValueError):
        FlatIPIndex(8, dtype="sq8", sq8_step=step)


@pytest.mark.parametrize("fn", ["ls_create_sharded", "ls_create_replicated"])
def test_sharded_and_replicated_creation_refuse_sq8_before_looking_for_devices(fn):
    lib = native.load()
    x = np.ones((4, 8), np.float32)
    ids = (ctypes.c_int32 * 2)(9998, 9999)
    h = ctypes.c_void_p()
    assert getattr(lib, fn)(ctypes.byref(h), x.ctypes.data, 4, 8, native.LS_DTYPE_SQ8, ids, 2) == native.LS_ERR_INVALID_ARG
    assert b"sq8" in lib.ls_last_error()
    # ... also with no device list at all, where the other dtypes answer LS_ERR_NO_DEVICE
    assert getattr(lib, fn)(ctypes.byref(h), x.ctypes.data, 4, 8, native.LS_DTYPE_SQ8, ids, 0) == native.LS_ERR_INVALID_ARG
    blocks = (ctypes.c_void_p * 2)(1, 1)
    rows = (ctypes.c_int64 * 2)(2, 2)
    assert lib.ls_create_sharded_from_device(ctypes.byref(h), blocks, rows, 8, native.LS_DTYPE_SQ8, ids,
                                             2) == native.LS_ERR_INVALID_ARG


def test_no_device_without_a_gpu(gpu_available):
    if gpu_available:
        return  # (nothing to observe on a GPU box: tests/test_sq8_gpu.py runs there)
    lib = native.load()
    x = np.ones((4, 8), np.float32)
    h = ctypes.c_void_p()
    assert lib.ls_create_sq8(ctypes.byref(h), x.ctypes.data, 4, 8, None, 0) == native.LS_ERR_NO_DEVICE
    assert lib.ls_create(ctypes.byref(h), x.ctypes.data, 4, 8, native.LS_DTYPE_SQ8, 0) == native.LS_ERR_NO_DEVICE
    cent = np.ones((2, 8), np.float32)
    assert lib.ls_ivf_create(ctypes.byref(h), x.ctypes.data, 4, 8, native.LS_DTYPE_SQ8, cent.ctypes.data, 2, None,
                             0) == native.LS_ERR_NO_DEVICE


def test_python_refusals(tmp_path):
    ix = FlatIPIndex(8, dtype="sq8")
    assert ix.storage_dtype == "sq8" and IVFFlatIndex(8, 4, dtype="sq8").storage_dtype == "sq8"
    with pytest.raises(ValueError, match="shard"):
        FlatIPIndex(8, dtype="sq8", devices=[0, 1])
    with pytest.raises(ValueError, match="shard"):
        FlatIPIndex.from_array(np.ones((4, 8), np.float32), dtype="sq8", devices=[0, 0], replicate=True)
    with pytest.raises(ValueError, match="f16_small_batch"):
        FlatIPIndex(8, dtype="sq8", f16_small_batch=True)
    with pytest.raises(ValueError, match="f16_small_batch"):
        ix.set_f16_small_batch(True)
    with pytest.raises(ValueError):
        FlatIPIndex(8, dtype="f32", sq8_step=np.ones(8, np.float32))
    with pytest.raises(ValueError):
        FlatIPIndex(8, dtype="sq8", sq8_step=np.ones(7, np.float32))
    ix.add(np.ones((3, 8), np.float32))
    with pytest.raises(ValueError, match="allow_lossy"):
        faiss_compat.write_index(ix, tmp_path / "x.index")
    with pytest.raises(ValueError, match="QT_8bit"):
        faiss_compat.IndexScalarQuantizer(8, faiss_compat.QT_fp16)
    with pytest.raises(ValueError, match="INNER_PRODUCT"):
        faiss_compat.IndexScalarQuantizer(8, faiss_compat.QT_8bit, faiss_compat.METRIC_L2)
    sq = faiss_compat.IndexScalarQuantizer(8, faiss_compat.QT_8bit, faiss_compat.METRIC_INNER_PRODUCT)
    assert sq.storage_dtype == "sq8" and not sq.is_trained
    x = np.arange(24, dtype=np.float32).reshape(3, 8) - 10
    sq.train(x)
    assert sq.is_trained and np.array_equal(sq._sq8_step, sq8.train_step(x))
    with pytest.raises(ValueError, match="sq8"):
        S.SearchEngine(index=object(), ids_map=[], lexical_retriever=False, storage_dtype="sq8", devices=[0, 1])
    from lean_explore_amd.sharded import ShardedFlatIPIndex

    with pytest.raises(ValueError, match="sq8"):
        ShardedFlatIPIndex.from_array(np.ones((4, 8), np.float32), dtype="sq8")
    with pytest.raises(ValueError, match="sq8"):
        ShardedFlatIPIndex(ix, 3)


# ---- the codes ----------------------------------------------------------------------------------------------------------
def test_train_encode_decode_on_hand_made_rows():
    f = np.float32
    x = np.array([[0.0, 127.0, 1.0, np.nan, 3.0, -2.0],
                  [0.0, -63.5, 2.5, 1.0, np.inf, 0.5],
                  [0.0, 0.5, -254.0, -2.0, -np.inf, np.nan],
                  [0.0, 1.5, 0.5, np.inf, 1.0, 2.0]], f)
    step = sq8.train_step(x)
    # zero column -> 1; inf / NaN do not train the step
    assert step.dtype == np.float32
    assert np.array_equal(step, np.array([1.0, 1.0, 2.0, f(2.0) / f(127.0), f(3.0) / f(127.0), f(2.0) / f(127.0)], f))
    c = sq8.encode(x, step)
    assert c.dtype == np.int8
    assert c[:, 0].tolist() == [0, 0, 0, 0]
    # ties to even: -63.5 -> -64, 0.5 -> 0, 1.5 -> 2; with step 2: 1/2 -> 0, 2.5/2 = 1.25 -> 1, 0.5/2 -> 0
    assert c[:, 1].tolist() == [127, -64, 0, 2]
    assert c[:, 2].tolist() == [0, 1, -127, 0]
    # NaN -> 0, +-inf -> +-127, the column's largest finite value -> +-127
    assert c[:, 3].tolist() == [0, 64, -127, 127]
    assert c[:, 4].tolist() == [127, 127, -127, 42]
    assert c[:, 5].tolist() == [-127, 32, 0, 127]
    # clamping with a given step: values beyond +-127 * step
    c2 = sq8.encode(np.array([[1000.0, -1000.0, 127.4, -127.6, 3.4e38, 126.5]], f), np.ones(6, f))
    assert c2.tolist() == [[127, -127, 127, -127, 127, 126]]
    dec = sq8.decode(c, step)
    assert dec.dtype == np.float32 and np.array_equal(dec, c.astype(f) * step)
    assert np.array_equal(sq8.train_step(np.zeros((0, 3), f)), np.ones(3, f))


# ---- the score ----------------------------------------------------------------------------------------------------------
def test_c_restatement_against_float64():
    n, d = 2_000, 384
    corpus, _ = mixture(5, n, d, 16)
    rng = np.random.default_rng(6)
    q = rng.standard_normal((8, d)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    step = sq8.train_step(corpus)
    codes = sq8.encode(corpus, step)
    rc, g = geom(d)
    assert rc == 0
    got = ref_scores(padded_codes(codes, g[0]), g, q * step)
    want = q.astype(np.float64) @ sq8.decode(codes, step).astype(np.float64).T
    assert got.shape == want.shape == (8, n)
    assert np.abs(got - want).max() <= 1e-5
    # the geometry matters to the bits, not to the value: another (L, V) of the same padded rows stays within the bound
    alt = ref_scores(padded_codes(codes, 32), (32, 16, 2), q * step)
    assert np.abs(alt - want).max() <= 1e-5


@pytest.mark.parametrize("n, d, nlist, k, floor", QUALITY)
def test_quality_of_the_definition(n, d, nlist, k, floor):
    """float64, no library: the decoded rows against the float32 rows."""
    corpus, _, q = quality_data(n, d, nlist)
    step = sq8.train_step(corpus)
    dec = sq8.decode(sq8.encode(corpus, step), step)
    S32 = q.astype(np.float64) @ corpus.astype(np.float64).T
    S8 = q.astype(np.float64) @ dec.astype(np.float64).T
    I32 = np.argsort(-S32, axis=1, kind="stable")[:, :k]
    I8 = np.argsort(-S8, axis=1, kind="stable")[:, :k]
    rec, dmax = recall_at(I8, I32), float(np.abs(S8 - S32).max())
    print(f"sq8 definition n={n} d={d}: recall@{k} {rec:.4f}  top-1 equal {int((I8[:, 0] == I32[:, 0]).sum())}/64  "
          f"max |dscore| {dmax:.2e}")
    assert rec >= floor
    assert np.array_equal(I8[:, 0], I32[:, 0])
    assert dmax <= 1e-2
