"""The sq8 small-batch pass (csrc/ls_mq8.hip, ls_set_sq8_small_batch) without a GPU: the header and the binding, the
argument checks, and the kernel's build-time facts (no scratch, the register ceiling, the f32 MFMA and the 16-byte
nontemporal corpus loads in the emitted code)."""

import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from lean_explore_amd import faiss_compat, native
from lean_explore_amd.index import FlatIPIndex

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "leansearch_sq8_batch.h"


def test_header_declares_exactly_the_option_and_it_is_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ls_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(native.SQ8_BATCH_SYMBOLS) == ["ls_set_sq8_small_batch"]
    assert not set(native.SQ8_BATCH_SYMBOLS) & (set(native.SYMBOLS) | set(native.SQ8_SYMBOLS) | set(native.IVF_SYMBOLS))
    raw = ctypes.CDLL(str(native.LIB_PATH))
    assert hasattr(raw, "ls_set_sq8_small_batch"), "ls_set_sq8_small_batch is not exported"
    fn = native.load().ls_set_sq8_small_batch  # load() bound it
    assert fn.argtypes == [ctypes.c_void_p, ctypes.c_int32] and fn.restype == ctypes.c_int


def test_null_handle_is_an_argument_error():
    lib = native.load()
    assert lib.ls_set_sq8_small_batch(None, 1) == native.LS_ERR_INVALID_ARG
    assert b"ls_set_sq8_small_batch" in lib.ls_last_error()
    assert lib.ls_debug_counter(None, 36) == -1


def test_sq8_small_batch_needs_sq8_storage():
    for dtype in ("f32", "f16"):
        with pytest.raises(ValueError, match="sq8_small_batch"):
            FlatIPIndex(64, dtype=dtype, sq8_small_batch=True)
        ix = FlatIPIndex(64, dtype=dtype)
        with pytest.raises(ValueError, match="sq8_small_batch"):
            ix.set_sq8_small_batch(True)
        ix.set_sq8_small_batch(False)  # switching it off is always allowed
        assert ix.sq8_small_batch is False
    with pytest.raises(ValueError):
        FlatIPIndex(64, sq8_small_batch=True)  # (the default storage is fp32)
    assert FlatIPIndex(64, dtype="sq8", sq8_small_batch=True).sq8_small_batch is True


def test_keyword_is_kept_before_any_device_is_touched():
    ix = FlatIPIndex(64, dtype="sq8", sq8_small_batch=True)
    assert ix.sq8_small_batch is True and ix._handle is None
    assert FlatIPIndex(64, dtype="sq8").sq8_small_batch is False
    ix.set_sq8_small_batch(False)
    assert ix.sq8_small_batch is False and ix._handle is None
    ix.set_sq8_small_batch(True)
    assert ix.sq8_small_batch is True and ix._handle is None
    sq = faiss_compat.IndexScalarQuantizer(64, sq8_small_batch=True)
    assert sq.sq8_small_batch is True and sq._handle is None and sq.storage_dtype == "sq8"
    assert faiss_compat.IndexScalarQuantizer(64).sq8_small_batch is False


def test_engine_passes_the_option_through(tmp_path):
    from lean_explore_amd.search.engine import SearchEngine

    for dtype in ("f32", "f16"):
        with pytest.raises(ValueError, match="sq8_small_batch"):
            SearchEngine(index=object(), ids_map=[], lexical_retriever=False, storage_dtype=dtype, sq8_small_batch=True,
                         base_path=tmp_path, db_path=tmp_path / "x.db")
    e = SearchEngine(index=object(), ids_map=[], lexical_retriever=False, storage_dtype="sq8", sq8_small_batch=True,
                     base_path=tmp_path, db_path=tmp_path / "x.db")
    assert e._sq8_small_batch is True
    e = SearchEngine(index=object(), ids_map=[], lexical_retriever=False, storage_dtype="sq8",
                     base_path=tmp_path, db_path=tmp_path / "x.db")
    assert e._sq8_small_batch is False


@pytest.mark.parametrize("L, V", [(8, 3), (16, 4)])
def test_mq8_kernel_resources_and_matrix_instruction(tmp_path, L, V):
    """The shortest multi-round geometry (8 lanes x 3 chunks: d = 384) and the longest row served (16 x 4: d = 1024),
    the lightest (3 keys per lane) and the heaviest (8 keys) instantiation of each: no scratch, no spill, and at most
    256 VGPRs + AGPRs - the kernel is launched with two waves per SIMD in mind (__launch_bounds__(256, 2)). The
    emitted code carries the 16x16x4 f32 MFMA and 16-byte nontemporal corpus loads."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = ROOT / "lean-explore_amd" / "csrc" / "ls_mq8.hip"
    asm = tmp_path / f"mq8_{L}_{V}.s"
    p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=fast",
                        "-Rpass-analysis=kernel-resource-usage", "-DLS_MQ8_KERNEL_ONLY", f"-DLS_MQ8_ONLY_L={L}",
                        f"-DLS_MQ8_ONLY_V={V}", "--cuda-device-only", "-S", str(src), "-o", str(asm)],
                       capture_output=True, text=True, timeout=900)
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
    kernels = {n: u for n, u in usage.items() if f"ls_mq8_kernelILi{L}ELi{V}E" in n}
    assert len(kernels) == 2, sorted(usage)
    assert {re.search(r"ELi(\d+)EEv", n).group(1) for n in kernels} == {"3", "8"}
    for n, u in kernels.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u.get("VGPRs Spill", 0) == 0, (n, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 256, (n, u)
    text = asm.read_text()
    assert "v_mfma_f32_16x16x4_f32" in text
    assert re.search(r"global_load_dwordx4 .* nt", text)
