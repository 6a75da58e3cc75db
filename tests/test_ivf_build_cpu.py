"""IVF build without a GPU: the C ABI of include/leansearch_ivf_build.h is exported and bound, arguments are validated
before any device is touched, nothing computes without one, the host plan of the two kernels holds under sanitizers,
the kernels fit their registers, and ``write_index`` of an IVFFlatIndex writes the ``IwFl`` file the reader parses."""

import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from lean_explore_amd import faiss_compat, native
from lean_explore_amd.ivf import IVFFlatIndex
from tests.test_ivf_cpu import declared, write_iwfl

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "lean-explore_amd" / "csrc"
HEADER = ROOT / "include" / "leansearch_ivf_build.h"
INVALID, NO_DEVICE = native.LS_ERR_INVALID_ARG, native.LS_ERR_NO_DEVICE


def test_header_symbols_exported_bound_and_disjoint():
    names = declared(HEADER)
    assert names == sorted(["ls_ivf_trainer_create", "ls_ivf_trainer_assign", "ls_ivf_trainer_means",
                            "ls_ivf_trainer_last_kernel_ms", "ls_ivf_trainer_destroy", "ls_ivf_assign",
                            "ls_ivf_reconstruct"])
    assert sorted(native.IVF_BUILD_SYMBOLS) == names
    for other in (native.SYMBOLS, native.IVF_SYMBOLS, native.IVF_SUBSET_SYMBOLS, native.SQ8_SYMBOLS,
                  native.SQ8_BATCH_SYMBOLS, native.SUBSET_BATCH_SYMBOLS, native.BM25_SUBSET_SYMBOLS):
        assert not set(native.IVF_BUILD_SYMBOLS) & set(other)
    raw = ctypes.CDLL(str(native.LIB_PATH))
    lib = native.load()
    for n in names:
        assert hasattr(raw, n), f"{n} declared in leansearch_ivf_build.h but not exported"
        assert getattr(lib, n).argtypes == native.IVF_BUILD_SYMBOLS[n][1], n  # load() bound it


def test_arguments_are_validated_before_any_device():
    lib = native.load()
    x = np.ones((4, 8), np.float32)
    c = np.ones((2, 8), np.float32)
    a = np.zeros(4, np.int32)
    m = np.zeros((2, 8), np.float64)
    h = ctypes.c_void_p()
    xp, cp, ap = x.ctypes.data, c.ctypes.data, a.ctypes.data
    create, assign = lib.ls_ivf_trainer_create, lib.ls_ivf_assign
    for nlist in (0, 8192, -1):
        assert create(ctypes.byref(h), xp, 4, 8, nlist, 0) == INVALID and not h.value
        assert b"nlist" in lib.ls_last_error()
        assert assign(xp, 4, 8, cp, nlist, ap, 0) == INVALID
        assert b"nlist" in lib.ls_last_error()
    for d in (0, 1025):
        assert create(ctypes.byref(h), xp, 4, d, 2, 0) == INVALID and not h.value
        assert assign(xp, 4, d, cp, 2, ap, 0) == INVALID
    assert create(ctypes.byref(h), xp, -1, 8, 2, 0) == INVALID
    assert assign(xp, -1, 8, cp, 2, ap, 0) == INVALID
    assert create(None, xp, 4, 8, 2, 0) == INVALID
    assert create(ctypes.byref(h), None, 4, 8, 2, 0) == INVALID and not h.value
    assert assign(None, 4, 8, cp, 2, ap, 0) == INVALID
    assert assign(xp, 4, 8, None, 2, ap, 0) == INVALID
    assert assign(xp, 4, 8, cp, 2, None, 0) == INVALID
    assert lib.ls_ivf_trainer_assign(None, cp, ap, None) == INVALID
    assert lib.ls_ivf_trainer_means(None, m.ctypes.data) == INVALID
    assert lib.ls_ivf_reconstruct(None, 0, 1, xp) == INVALID
    assert lib.ls_ivf_trainer_last_kernel_ms(None, None, None) == INVALID
    lib.ls_ivf_trainer_destroy(None)  # (a no-op)
    with pytest.raises(ValueError):
        IVFFlatIndex(8, 8192, build_on_device=True)
    with pytest.raises(ValueError):
        faiss_compat.IndexIVFFlat(None, 8, 8192, ivf=True, build_on_device=True)
    ix = IVFFlatIndex(8, 8192)  # (the host path has no such bound) ...
    with pytest.raises(ValueError):
        ix.train(np.ones((8192, 8), np.float32), on_device=True)  # ... the keyword does, before any device call
    ix = faiss_compat.IndexIVFFlat(None, 8, 4, ivf=True, build_on_device=True)
    assert isinstance(ix, IVFFlatIndex) and ix.build_on_device and ix._handle is None
    assert IVFFlatIndex(8, 4).build_on_device is False


def test_nothing_computes_without_a_device(gpu_available):
    if gpu_available:
        pytest.skip("a GPU is visible; the refusal path is for CPU-only hosts")
    lib = native.load()
    x = np.ones((4, 8), np.float32)
    c = np.ones((2, 8), np.float32)
    a = np.zeros(4, np.int32)
    h = ctypes.c_void_p()
    assert lib.ls_ivf_trainer_create(ctypes.byref(h), x.ctypes.data, 4, 8, 2, 0) == NO_DEVICE and not h.value
    assert b"no CPU path" in lib.ls_last_error()
    assert lib.ls_ivf_assign(x.ctypes.data, 4, 8, c.ctypes.data, 2, a.ctypes.data, 0) == NO_DEVICE
    assert lib.ls_ivf_assign(x.ctypes.data, 0, 8, c.ctypes.data, 2, None, 0) == NO_DEVICE  # (n == 0 too)
    ix = IVFFlatIndex(8, 2, build_on_device=True)
    with pytest.raises(native.LeanSearchError) as e:
        ix.train(x)
    assert e.value.code == NO_DEVICE


def test_host_plan_under_sanitizers(tmp_path):
    """csrc/ls_ivf_build_plan.h in a plain host program with its own main (tests/ivf_build_plan_check.cpp), built with
    AddressSanitizer and UndefinedBehaviorSanitizer: 8 geometries x 6 row counts x 5 list counts x 2 CU counts."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host check of ls_ivf_build_plan.h"
    exe = tmp_path / "ivf_build_plan_check"
    p = subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", str(CSRC),
                        str(ROOT / "tests" / "ivf_build_plan_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.strip() == f"OK {8 * 6 * 5 * 2} cases"


def test_kernel_resources(tmp_path):
    """The lightest (16 lanes x 1 chunk, 8 row groups) and the heaviest (64 x 4, 4 row groups) assignment kernel and
    the means kernel: no scratch, no spill, at most 256 VGPRs + AGPRs; the tile is read with 16-byte nontemporal
    loads and the means accumulate in float64."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    asm = tmp_path / "ivf_build.s"
    p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=fast",
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S",
                        str(CSRC / "ls_ivf_build.hip"), "-o", str(asm)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
        if m and name:
            usage[name][m.group(1)] = int(m.group(2))
    assign = {n: u for n, u in usage.items() if "ls_ivf_assign_kernel" in n}
    assert len(assign) == 8, sorted(usage)
    picked = [n for n in assign if re.search(r"ILi16ELi1ELi8EE|ILi64ELi4ELi4EE", n)]
    means = [n for n in usage if "ls_ivf_means_kernel" in n]
    assert len(picked) == 2 and len(means) == 1, sorted(usage)
    for n in picked + means:
        u = usage[n]
        assert u["ScratchSize [bytes/lane]"] == 0 and u.get("VGPRs Spill", 0) == 0, (n, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 256, (n, u)
    text = asm.read_text()
    assert re.search(r"global_load_dwordx4 .* nt", text)
    assert "v_add_f64" in text


# ------------------------------------------------------------------ the IwFl writer
def _lists_index(seed=5, n=300, d=24, nlist=7, nprobe=3, dtype="f32"):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d), dtype=np.float32)
    cent = rng.standard_normal((nlist, d), dtype=np.float32)
    a = rng.integers(0, nlist, n).astype(np.int32)
    a[a == 4] = 3  # (list 4 is empty)
    ix = IVFFlatIndex(d, nlist, dtype=dtype)
    ix.set_centroids(cent)
    ix.add(x[:100], assign=a[:100])
    ix.add(x[100:], assign=a[100:])
    ix.nprobe = nprobe
    return ix, x, a, cent


def test_writer_is_byte_identical_to_the_test_writer_and_round_trips(tmp_path):
    ix, x, a, cent = _lists_index()
    faiss_compat.write_index(ix, tmp_path / "ours.index")
    write_iwfl(tmp_path / "theirs.index", x, a, cent, 3)
    assert (tmp_path / "ours.index").read_bytes() == (tmp_path / "theirs.index").read_bytes()
    assert ix._handle is None  # nothing was built: rows and lists came from the buffers
    assert np.array_equal(ix.reconstruct_n(10, 5), x[10:15])
    back = faiss_compat.read_index(tmp_path / "ours.index", ivf=True)
    assert isinstance(back, IVFFlatIndex) and back.nprobe == 3 and back.nlist == 7 and back.ntotal == 300
    assert np.array_equal(back.centroids, cent)
    assert np.array_equal(np.concatenate(back._assign), a)
    assert np.array_equal(back.reconstruct_n(0, 300), x)
    flat = faiss_compat.read_index(tmp_path / "ours.index")  # the default reader still scatters the lists back
    assert np.array_equal(flat.host_corpus(), x)


def test_writer_of_an_empty_index(tmp_path):
    ix = IVFFlatIndex(8, 3)
    ix.set_centroids(np.eye(3, 8, dtype=np.float32))
    faiss_compat.write_index(ix, tmp_path / "e.index")
    write_iwfl(tmp_path / "t.index", np.zeros((0, 8), np.float32), np.zeros(0, np.int64), np.eye(3, 8, dtype=np.float32))
    assert (tmp_path / "e.index").read_bytes() == (tmp_path / "t.index").read_bytes()
    back = faiss_compat.read_index(tmp_path / "e.index", ivf=True)
    assert back.ntotal == 0 and back.nprobe == 1


def test_writer_refusals(tmp_path):
    with pytest.raises(ValueError, match="not trained"):
        faiss_compat.write_index(IVFFlatIndex(8, 3), tmp_path / "u.index")
    for dtype in ("f16", "sq8"):
        ix, *_ = _lists_index(dtype=dtype)
        with pytest.raises(ValueError, match="allow_lossy"):
            faiss_compat.write_index(ix, tmp_path / "l.index")
    assert not list(tmp_path.iterdir())
    ix, *_ = _lists_index()
    with pytest.raises(ValueError):
        ix.reconstruct_n(290, 20)
