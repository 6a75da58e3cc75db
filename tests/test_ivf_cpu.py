"""IVF-flat search without a GPU: the C ABI of include/leansearch_ivf.h is exported and bound, nothing computes
without a device, arguments are validated on the host, and the ``IwFl`` parser keeps the centroids and lists a
writer put into the file (``read_index(..., ivf=True)``) while the default still drops them."""

import ctypes
import re
import struct
from pathlib import Path

import numpy as np
import pytest

from lean_explore_amd import faiss_compat, native
from lean_explore_amd.id_selectors import IDSelectorRange, SearchParameters, SearchParametersIVF
from lean_explore_amd.index import FlatIPIndex
from lean_explore_amd.ivf import IVFFlatIndex

ROOT = Path(__file__).resolve().parent.parent
IVF_HEADER = ROOT / "include" / "leansearch_ivf.h"


def write_iwfl(path, corpus, assign, centroids, nprobe=1):
    """An ``IwFl`` file (layout of upstream faiss's index_write.cpp, as lean_explore_amd.faiss_compat reads it) with
    REAL centroids in the nested flat quantiser and the given row -> list assignment."""
    fc = faiss_compat
    corpus = np.ascontiguousarray(corpus, dtype="<f4")
    centroids = np.ascontiguousarray(centroids, dtype="<f4")
    n, d = corpus.shape
    nlist = centroids.shape[0]
    with open(path, "wb") as f:
        f.write(struct.pack("<I", fc._fourcc("IwFl")))
        fc._write_header(f, d, n, fc.METRIC_INNER_PRODUCT)
        f.write(struct.pack("<QQ", nlist, nprobe))
        f.write(struct.pack("<I", fc._fourcc("IxFI")))
        fc._write_header(f, d, nlist, fc.METRIC_INNER_PRODUCT)
        f.write(struct.pack("<Q", nlist * d))
        f.write(centroids.tobytes())
        f.write(struct.pack("<b", 0))  # no direct map
        f.write(struct.pack("<Q", 0))
        f.write(struct.pack("<I", fc._fourcc("ilar")))
        f.write(struct.pack("<QQ", nlist, 4 * d))
        f.write(struct.pack("<I", fc._fourcc("full")))
        f.write(struct.pack("<Q", nlist))
        f.write(np.bincount(assign, minlength=nlist).astype("<u8").tobytes())
        for li in range(nlist):
            ids = np.nonzero(assign == li)[0].astype("<i8")
            if ids.size:
                f.write(corpus[ids].tobytes())
                f.write(ids.tobytes())


def declared(header=IVF_HEADER):
    text = re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(ls_[a-z0-9_]+)\s*\(", text)))


def test_ivf_header_symbols_exported_and_bound():
    names = declared()
    assert {"ls_ivf_create", "ls_ivf_search", "ls_ivf_ntotal", "ls_ivf_dim", "ls_ivf_nlist", "ls_ivf_list_sizes",
            "ls_ivf_destroy", "ls_ivf_last_kernel_ms"} <= set(names)
    assert sorted(native.IVF_SYMBOLS) == names
    assert not set(native.IVF_SYMBOLS) & set(native.SYMBOLS)
    raw = ctypes.CDLL(str(native.LIB_PATH))
    lib = native.load()
    for n in names:
        assert hasattr(raw, n), f"{n} declared in leansearch_ivf.h but not exported"
        assert getattr(lib, n).argtypes == native.IVF_SYMBOLS[n][1], n  # load() bound it


def test_ivf_create_needs_a_device(gpu_available):
    if gpu_available:
        pytest.skip("a GPU is visible; the refusal path is for CPU-only hosts")
    lib = native.load()
    x = np.ones((4, 8), np.float32)
    c = np.ones((2, 8), np.float32)
    h = ctypes.c_void_p()
    rc = lib.ls_ivf_create(ctypes.byref(h), x.ctypes.data, 4, 8, native.LS_DTYPE_F32, c.ctypes.data, 2, None, 0)
    assert rc == native.LS_ERR_NO_DEVICE and not h.value
    assert b"no CPU path" in lib.ls_last_error()
    ix = IVFFlatIndex(8, 2)
    ix.set_centroids(c)
    ix.add(x)
    with pytest.raises(native.LeanSearchError) as e:
        ix.search(x[:1], 2)
    assert e.value.code == native.LS_ERR_NO_DEVICE


def test_ivf_argument_validation_needs_no_gpu():
    lib = native.load()
    x = np.ones((4, 8), np.float32)
    c = np.ones((2, 8), np.float32)
    h = ctypes.c_void_p()
    # the library refuses these before it looks for a device
    assert lib.ls_ivf_create(ctypes.byref(h), x.ctypes.data, 4, 8, 0, c.ctypes.data, 0, None, 0) == native.LS_ERR_INVALID_ARG
    assert b"nlist" in lib.ls_last_error()
    assert lib.ls_ivf_create(ctypes.byref(h), x.ctypes.data, 4, 8, 7, c.ctypes.data, 2, None, 0) == native.LS_ERR_INVALID_ARG
    assert lib.ls_ivf_create(ctypes.byref(h), x.ctypes.data, -1, 8, 0, c.ctypes.data, 2, None, 0) == native.LS_ERR_INVALID_ARG
    assert lib.ls_ivf_search(None, x.ctypes.data, 1, 2, 1, 0, None, None) == native.LS_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        IVFFlatIndex(8, 0)
    with pytest.raises(ValueError):
        IVFFlatIndex(0, 4)
    with pytest.raises(ValueError):
        IVFFlatIndex(8, 4, dtype="int8")
    ix = IVFFlatIndex(8, 2)
    assert ix.nprobe == 1 and not ix.is_trained and ix.ntotal == 0 and ix.d == 8 and ix.nlist == 2
    with pytest.raises(ValueError):
        ix.add(x)  # not trained
    with pytest.raises(ValueError):
        ix.set_centroids(np.ones((3, 8), np.float32))
    with pytest.raises(ValueError):
        ix.train(np.ones((1, 8), np.float32))  # fewer rows than lists
    ix.set_centroids(c)
    assert ix.is_trained
    with pytest.raises(ValueError):
        ix.add(np.ones((2, 7), np.float32))
    with pytest.raises(ValueError):
        ix.add(x, assign=np.array([0, 1, 2, 0]))  # list 2 of 2
    ix.add(x)
    assert ix.ntotal == 4
    with pytest.raises(ValueError):
        ix.search(x[:1], 2, params=SearchParameters(sel=IDSelectorRange(0, 2)))
    with pytest.raises(ValueError):
        ix.search(x[:1], 2, params=SearchParametersIVF(nprobe=0))
    ix.nprobe = 0
    with pytest.raises(ValueError):
        ix.search(x[:1], 2)
    ix.nprobe = 1
    with pytest.raises(ValueError):
        ix.search(x[:1], 0)
    with pytest.raises(ValueError):
        ix.search(np.ones((1, 7), np.float32), 2)
    D, I = ix.search(np.zeros((0, 8), np.float32), 3)  # nq = 0 never reaches the device
    assert D.shape == (0, 3) and I.shape == (0, 3)


def test_faiss_compat_ivf_switches():
    # default: today's pretender, an exact flat index with plain attributes
    flat = faiss_compat.IndexIVFFlat(faiss_compat.IndexFlatIP(8), 8, 4)
    assert isinstance(flat, FlatIPIndex) and type(flat) is faiss_compat.IndexIVFFlat
    assert flat.nlist == 4 and flat.nprobe == 1 and not flat.is_trained
    flat.train(np.ones((2, 8), np.float32))
    assert flat.is_trained
    real = faiss_compat.IndexIVFFlat(faiss_compat.IndexFlatIP(8), 8, 4, faiss_compat.METRIC_INNER_PRODUCT, ivf=True)
    assert isinstance(real, IVFFlatIndex) and not isinstance(real, FlatIPIndex)
    assert real.nlist == 4 and real.nprobe == 1 and not real.is_trained and real.storage_dtype == "f32"
    with pytest.raises(ValueError):
        faiss_compat.IndexIVFFlat(None, 8, 4, faiss_compat.METRIC_L2, ivf=True)


def test_read_index_keeps_centroids_and_lists_only_when_asked(tmp_path):
    rng = np.random.default_rng(5)
    n, d, nlist = 300, 24, 7
    corpus = rng.standard_normal((n, d), dtype=np.float32)
    centroids = rng.standard_normal((nlist, d), dtype=np.float32)
    assign = rng.integers(0, nlist, n).astype(np.int32)
    assign[assign == 3] = 2  # an empty list
    p = tmp_path / "real.index"
    write_iwfl(p, corpus, assign, centroids, nprobe=5)

    with open(p, "rb") as f:
        f.read(4)
        dd, rows, cent, lists, nprobe = faiss_compat._read_ivf_flat(f, keep_lists=True)
    assert dd == d and nprobe == 5
    assert np.array_equal(rows, corpus) and np.array_equal(cent, centroids) and np.array_equal(lists, assign)

    ivf = faiss_compat.read_index(p, ivf=True)
    assert isinstance(ivf, IVFFlatIndex) and ivf.is_trained
    assert (ivf.d, ivf.nlist, ivf.ntotal, ivf.nprobe) == (d, nlist, n, 5)
    assert np.array_equal(ivf.centroids, centroids)
    assert np.array_equal(np.concatenate(ivf._assign), assign) and np.array_equal(ivf._pending[0], corpus)

    flat = faiss_compat.read_index(p)  # the default: rows back in add order, searched exactly, no lists
    assert type(flat) is FlatIPIndex and flat.ntotal == n and not hasattr(flat, "nprobe") and not hasattr(flat, "nlist")
    assert np.array_equal(flat.host_corpus(), corpus)

    q = tmp_path / "flat.index"
    faiss_compat.write_index(flat, q)
    with pytest.raises(ValueError):
        faiss_compat.read_index(q, ivf=True)  # IxFI: no centroids, no lists
    assert faiss_compat.read_index(q).ntotal == n
    with pytest.raises(ValueError):
        faiss_compat.read_index(p, ivf=True, devices=[0, 0])


def test_engine_semantic_index_switch(tmp_path):
    from lean_explore_amd.search.engine import SearchEngine

    with pytest.raises(ValueError):
        SearchEngine(base_path=tmp_path, index=object(), ids_map=[], lexical_retriever=False, semantic_index="hnsw")
    eng = SearchEngine(base_path=tmp_path, index=object(), ids_map=[], lexical_retriever=False, semantic_index="ivf")
    import asyncio

    with pytest.raises(ValueError):
        asyncio.run(eng.search_prefiltered("x", ["Mathlib"]))
    assert SearchEngine(base_path=tmp_path, index=object(), ids_map=[], lexical_retriever=False)._semantic_index == "flat"
