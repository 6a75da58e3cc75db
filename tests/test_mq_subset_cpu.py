"""The subset pass (csrc/ls_mq_subset.hip, ls_set_subset_small_batch) without a GPU: the header and the binding, the
argument checks, the kernel's build-time facts (no scratch, the register ceiling, the f32 MFMA and the 16-byte
nontemporal row loads in the emitted code), the host plan under sanitizers, and the key-list sizes the GPU test's k sweep
reaches."""

import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from lean_explore_amd import faiss_compat, native
from lean_explore_amd.index import FlatIPIndex
from tests import mq_subset_shapes as SH

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "lean-explore_amd" / "csrc"
HEADER = ROOT / "include" / "leansearch_subset_batch.h"


def test_header_declares_exactly_the_option_and_it_is_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ls_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(native.SUBSET_BATCH_SYMBOLS) == ["ls_set_subset_small_batch"]
    others = (set(native.SYMBOLS) | set(native.SQ8_SYMBOLS) | set(native.IVF_SYMBOLS) | set(native.SQ8_BATCH_SYMBOLS)
              | set(native.BM25_SUBSET_SYMBOLS) | set(native.IVF_SUBSET_SYMBOLS))
    assert not set(native.SUBSET_BATCH_SYMBOLS) & others
    raw = ctypes.CDLL(str(native.LIB_PATH))
    assert hasattr(raw, "ls_set_subset_small_batch"), "ls_set_subset_small_batch is not exported"
    fn = native.load().ls_set_subset_small_batch  # load() bound it
    assert fn.argtypes == [ctypes.c_void_p, ctypes.c_int32] and fn.restype == ctypes.c_int


def test_null_handle_is_an_argument_error():
    lib = native.load()
    for enable in (0, 1):
        assert lib.ls_set_subset_small_batch(None, enable) == native.LS_ERR_INVALID_ARG
        assert b"ls_set_subset_small_batch" in lib.ls_last_error()
    assert lib.ls_debug_counter(None, 37) == -1


def test_subset_small_batch_needs_fp32_rows_on_one_device():
    for dtype in ("f16", "sq8"):
        for cls in (FlatIPIndex, faiss_compat.IndexFlatIP):
            with pytest.raises(ValueError, match="subset_small_batch"):
                cls(64, dtype=dtype, subset_small_batch=True)
        ix = FlatIPIndex(64, dtype=dtype)
        with pytest.raises(ValueError, match="subset_small_batch"):
            ix.set_subset_small_batch(True)
        ix.set_subset_small_batch(False)  # switching it off is always allowed
        assert ix.subset_small_batch is False and ix._handle is None
    for replicate in (False, True):
        with pytest.raises(ValueError, match="subset_small_batch"):
            FlatIPIndex(64, devices=[0, 0], replicate=replicate, subset_small_batch=True)
        ix = FlatIPIndex(64, devices=[0, 0], replicate=replicate)
        with pytest.raises(ValueError, match="subset_small_batch"):
            ix.set_subset_small_batch(True)
        ix.set_subset_small_batch(False)
        assert ix.subset_small_batch is False and ix._handle is None


def test_keyword_is_kept_before_any_device_is_touched():
    ix = FlatIPIndex(64, subset_small_batch=True)
    assert ix.subset_small_batch is True and ix._handle is None
    assert FlatIPIndex(64).subset_small_batch is False
    ix.set_subset_small_batch(False)
    assert ix.subset_small_batch is False and ix._handle is None
    ix.set_subset_small_batch(True)
    assert ix.subset_small_batch is True and ix._handle is None
    fi = faiss_compat.IndexFlatIP(64, subset_small_batch=True)
    assert fi.subset_small_batch is True and fi._handle is None and fi.storage_dtype == "f32"
    assert faiss_compat.IndexFlatIP(64).subset_small_batch is False


@pytest.mark.parametrize("L, V", [(16, 3), (64, 4)])
def test_row_list_kernel_resources_and_matrix_instruction(tmp_path, L, V):
    """d = 384 (16 lanes x 3 chunks) and d = 1024 (64 x 4), the lightest (3 keys per lane) and the heaviest (8 keys)
    row-list instantiation of each: no scratch, no spill, and at most 256 VGPRs + AGPRs - the kernel is launched with
    two waves per SIMD in mind (__launch_bounds__(256, 2)). The emitted code carries the 16x16x4 f32 MFMA and 16-byte
    nontemporal row loads."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = CSRC / "ls_mq_subset.hip"
    asm = tmp_path / f"mqs_{L}_{V}.s"
    p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=fast",
                        "-Rpass-analysis=kernel-resource-usage", "-DLS_MQS_KERNEL_ONLY", f"-DLS_MQS_ONLY_L={L}",
                        f"-DLS_MQS_ONLY_V={V}", "--cuda-device-only", "-S", str(src), "-o", str(asm)],
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
    # <L, V, M, one B block, four waves, a row list (J PKj E: a pack of one const unsigned*)>
    kernels = {n: u for n, u in usage.items() if re.search(rf"ls_mq_kernelILi{L}ELi{V}ELi\d+ELi1ELi4EJPKjEE", n)}
    assert len(kernels) == 2, sorted(usage)
    assert {re.search(rf"ILi{L}ELi{V}ELi(\d+)E", n).group(1) for n in kernels} == {"3", "8"}
    for n, u in kernels.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u.get("VGPRs Spill", 0) == 0, (n, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 256, (n, u)
    text = asm.read_text()
    assert "v_mfma_f32_16x16x4_f32" in text
    assert re.search(r"global_load_dwordx4 .* nt", text)


def test_host_plan_under_sanitizers_and_the_restatement(tmp_path):
    """csrc/ls_mq_plan.h in a plain host program with its own main (tests/mq_plan_check.cpp), built with
    AddressSanitizer and UndefinedBehaviorSanitizer: its own sweep (kinds x sizes x k x CU counts x forced workgroups /
    k'), and the row-list plans of this file's restatement (tests/mq_subset_shapes.py) case for case."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host check of ls_mq_plan.h"
    exe = tmp_path / "mq_plan_check"
    p = subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", str(CSRC), str(ROOT / "tests" / "mq_plan_check.cpp"),
                        "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    m_half = int(SH.half_rows().size)
    cases = [(m, k, cu) for cu in (8, 256) for m in (1, 4095, 4096, 4097, 6000, m_half, SH.N, 200_000, 12_500_000)
             for k in (1, 10, 50, 150, 500, 1000, 2048)]
    args = [str(ROOT / "tests" / "mq_plan_parent.txt")] + [str(v) for c in cases for v in c]
    p = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    lines = [ln for ln in p.stdout.strip().splitlines() if not ln.startswith(("zeroed ", "defect "))]
    assert lines[-1].startswith("ok ") and len(lines) == len(cases) + 1
    for (m, k, cu), line in zip(cases, lines):
        got = tuple(int(x) for x in line.split())
        assert got == (m, k, cu) + SH.plan(m, k, cu), (got, SH.plan(m, k, cu))


def test_k_sweep_of_the_gpu_test_reaches_every_key_list_size():
    """On the GPU test's shape (a random half of 12 001 rows, 256 CUs) the k sweep selects 3, 5 and 8 keys per lane and
    declines one k: tests/test_mq_subset_gpu.py then runs every M instantiation of a geometry, and the declined route."""
    m = int(SH.half_rows().size)
    assert SH.MIN_ROWS < m < SH.N
    keys = [SH.plan(m, k)[2] for k in SH.K_SWEEP]
    assert keys == [3, 5, 8, 0], keys
    # the all-ones subset and a subset of exactly the threshold are served at the geometry sweep's k, one row fewer is not
    assert SH.plan(SH.N, 10)[2] == 3 and SH.plan(SH.MIN_ROWS, 10)[2] == 3 and SH.plan(SH.MIN_ROWS - 1, 10) == (0, 0, 0)
    # the integer-ties case asks for k = 500: a subset large enough for the key lists to take it
    assert SH.plan(int(SH.ties_rows().size), 500)[2] == 8
    assert [SH.groups(nq) for nq in (1, 2, 3, 15, 16, 17, 18, 32, 33, 40)] == [0, 1, 1, 1, 1, 1, 2, 2, 2, 3]
