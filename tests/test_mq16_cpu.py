"""The fp16 small-batch pass (csrc/ls_mq16.hip, ls_set_f16_small_batch) without a GPU: the argument checks, the
binding, the header, and the kernel's build-time facts (no scratch, the register ceiling, the f16 MFMA in the
emitted code)."""

import re
import shutil
import subprocess
from pathlib import Path

import pytest

from lean_explore_amd import native
from lean_explore_amd.index import FlatIPIndex

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "leansearch.h"

# every function the public header declared before this option was added
EARLIER = ["ls_add", "ls_bm25_create", "ls_bm25_destroy", "ls_bm25_ntotal", "ls_bm25_search", "ls_check", "ls_create",
           "ls_create_from_device", "ls_create_replicated", "ls_create_sharded", "ls_create_sharded_from_device",
           "ls_destroy", "ls_device", "ls_device_count", "ls_dim", "ls_dtype", "ls_export_flags", "ls_last_error",
           "ls_merge_topk", "ls_merge_topk_strided", "ls_normalize_l2", "ls_ntotal", "ls_reconstruct", "ls_search",
           "ls_search_device", "ls_search_subset", "ls_set_base", "ls_shard_count", "ls_shard_exchange_info",
           "ls_shard_info", "ls_subset_create", "ls_subset_destroy", "ls_version"]


def test_f16_small_batch_needs_fp16_storage():
    with pytest.raises(ValueError):
        FlatIPIndex(64, dtype="f32", f16_small_batch=True)
    with pytest.raises(ValueError):
        FlatIPIndex(64, f16_small_batch=True)  # (the default storage is fp32)
    ix = FlatIPIndex(64, dtype="f32")
    with pytest.raises(ValueError):
        ix.set_f16_small_batch(True)
    ix.set_f16_small_batch(False)  # switching it off is always allowed
    assert ix.f16_small_batch is False


def test_keyword_is_kept_before_any_device_is_touched():
    ix = FlatIPIndex(64, dtype="f16", f16_small_batch=True)
    assert ix.f16_small_batch is True and ix._handle is None
    assert FlatIPIndex(64, dtype="f16").f16_small_batch is False
    ix.set_f16_small_batch(False)
    assert ix.f16_small_batch is False and ix._handle is None
    ix.set_f16_small_batch(True)
    assert ix.f16_small_batch is True and ix._handle is None


def test_engine_passes_the_option_through(tmp_path):
    from lean_explore_amd.search.engine import SearchEngine

    with pytest.raises(ValueError):
        SearchEngine(index=object(), ids_map=[], lexical_retriever=False, storage_dtype="f32", f16_small_batch=True,
                     base_path=tmp_path, db_path=tmp_path / "x.db")
    e = SearchEngine(index=object(), ids_map=[], lexical_retriever=False, storage_dtype="f16", f16_small_batch=True,
                     base_path=tmp_path, db_path=tmp_path / "x.db")
    assert e._f16_small_batch is True


def test_symbol_is_bound_and_the_header_keeps_every_earlier_function():
    assert "ls_set_f16_small_batch" in native.SYMBOLS
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    names = set(re.findall(r"\b(ls_[a-z0-9_]+)\s*\(", text))
    assert set(EARLIER) <= names, sorted(set(EARLIER) - names)
    assert names - set(EARLIER) == {"ls_set_f16_small_batch"}
    assert "or an fp16 index with the small-batch pass" in HEADER.read_text()


def test_mq16_kernel_resources_and_matrix_instruction(tmp_path):
    """d = 384 (48 chunks) and d = 2048 (256 chunks: the longest stored row), the lightest (3 keys, one B block) and
    the heaviest (8 keys, two B blocks) instantiation of each: no scratch, and at most 256 VGPRs - the kernel is
    launched with two waves per SIMD in mind (__launch_bounds__(256, 2): two four-wave workgroups per CU where the
    LDS allows). The scan part itself is designed for under 128; the count the compiler reports is that of the
    riding selection job (finalize_body), which shares the kernel. The emitted code carries the 16x16x32 f16 MFMA
    and 16-byte nontemporal corpus loads."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = ROOT / "lean-explore_amd" / "csrc" / "ls_mq16.hip"
    for ch in (48, 256):
        asm = tmp_path / f"mq16_{ch}.s"
        p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=fast",
                            "-Rpass-analysis=kernel-resource-usage", "-DLS_MQ16_KERNEL_ONLY", f"-DLS_MQ16_ONLY_CH={ch}",
                            "--cuda-device-only", "-S", str(src), "-o", str(asm)],
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
        kernels = {n: u for n, u in usage.items() if f"ls_mq16_kernelILi{ch}E" in n}
        assert len(kernels) == 2, sorted(usage)
        for n, u in kernels.items():
            assert u["ScratchSize [bytes/lane]"] == 0 and u.get("VGPRs Spill", 0) == 0, (n, u)
            assert u["VGPRs"] + u.get("AGPRs", 0) <= 256, (n, u)
        text = asm.read_text()
        assert "v_mfma_f32_16x16x32_f16" in text
        assert re.search(r"global_load_dwordx4 .* nt", text)
        assert "scratch_" not in text
