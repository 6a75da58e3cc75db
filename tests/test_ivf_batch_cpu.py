"""The IVF small-batch pass (csrc/ls_ivf_batch.hip, ls_ivf_set_small_batch) without a GPU: the header and the binding,
the argument checks, the Python keywords, the host plan under sanitizers - held to every shape the GPU test launches -,
the numpy model of the union step, and the kernel's build-time facts."""

import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from lean_explore_amd import faiss_compat, native
from lean_explore_amd.ivf import IVFFlatIndex
from tests import ivf_batch_shapes as SH

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "lean-explore_amd" / "csrc"
HEADER = ROOT / "include" / "leansearch_ivf_batch.h"


def test_header_declares_exactly_the_two_calls_and_they_are_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ls_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(native.IVF_BATCH_SYMBOLS) == ["ls_ivf_last_passes", "ls_ivf_set_small_batch"]
    others = (set(native.SYMBOLS) | set(native.SQ8_SYMBOLS) | set(native.IVF_SYMBOLS) | set(native.SQ8_BATCH_SYMBOLS)
              | set(native.BM25_SUBSET_SYMBOLS) | set(native.IVF_SUBSET_SYMBOLS) | set(native.SUBSET_BATCH_SYMBOLS)
              | set(native.IVF_BUILD_SYMBOLS))
    assert not set(native.IVF_BATCH_SYMBOLS) & others
    raw = ctypes.CDLL(str(native.LIB_PATH))
    lib = native.load()
    for n in names:
        assert hasattr(raw, n), f"{n} declared in leansearch_ivf_batch.h but not exported"
        assert getattr(lib, n).argtypes == native.IVF_BATCH_SYMBOLS[n][1], n  # load() bound it


def test_null_handle_is_an_argument_error():
    lib = native.load()
    for enable in (0, 1):
        assert lib.ls_ivf_set_small_batch(None, enable) == native.LS_ERR_INVALID_ARG
        assert b"ls_ivf_set_small_batch" in lib.ls_last_error()
    p, r = ctypes.c_int32(), ctypes.c_int64()
    assert lib.ls_ivf_last_passes(None, ctypes.byref(p), ctypes.byref(r)) == native.LS_ERR_INVALID_ARG
    assert b"ls_ivf_last_passes" in lib.ls_last_error()


def test_small_batch_needs_fp32_rows_and_no_device_to_say_so(tmp_path):
    for dtype in ("f16", "sq8"):
        with pytest.raises(ValueError, match="small_batch"):
            IVFFlatIndex(64, 8, dtype=dtype, small_batch=True)
        with pytest.raises(ValueError, match="small_batch"):
            faiss_compat.IndexIVFFlat(None, 64, 8, dtype=dtype, ivf=True, ivf_small_batch=True)
        with pytest.raises(ValueError, match="ivf_small_batch"):
            faiss_compat.read_index(tmp_path / "absent.index", dtype=dtype, ivf=True, ivf_small_batch=True)
        ix = IVFFlatIndex(64, 8, dtype=dtype)
        with pytest.raises(ValueError, match="small_batch"):
            ix.set_small_batch(True)
        ix.set_small_batch(False)  # switching it off is always allowed
        assert ix.small_batch is False and ix._handle is None
    for make in (lambda: faiss_compat.IndexIVFFlat(None, 64, 8, ivf_small_batch=True),
                 lambda: faiss_compat.read_index(tmp_path / "absent.index", ivf_small_batch=True)):
        with pytest.raises(ValueError, match="ivf=True"):
            make()


def test_keyword_is_kept_before_any_device_is_touched():
    ix = IVFFlatIndex(64, 8, small_batch=True)
    assert ix.small_batch is True and ix._handle is None
    assert IVFFlatIndex(64, 8).small_batch is False
    ix.set_small_batch(False)
    assert ix.small_batch is False and ix._handle is None
    ix.set_small_batch(True)
    assert ix.small_batch is True and ix._handle is None
    fi = faiss_compat.IndexIVFFlat(None, 64, 8, ivf=True, ivf_small_batch=True)
    assert isinstance(fi, IVFFlatIndex) and fi.small_batch is True and fi._handle is None
    assert faiss_compat.IndexIVFFlat(None, 64, 8, ivf=True).small_batch is False


def test_groups_of_a_call():
    assert [SH.groups(nq) for nq in (1, 2, 3, 16, 17, 18, 32, 33, 34)] == [
        [], [2], [3], [16], [16], [16, 2], [16, 16], [16, 16], [16, 16, 2]]


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    """csrc/ls_mq_plan.h in a plain host program with its own main (tests/ivf_batch_plan_check.cpp), built with
    AddressSanitizer and UndefinedBehaviorSanitizer."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host check of ls_mq_plan.h"
    exe = tmp_path_factory.mktemp("ivfplan") / "ivf_batch_plan_check"
    p = subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", str(CSRC), str(ROOT / "tests" / "ivf_batch_plan_check.cpp"),
                        "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return exe


def run_plan(exe, cases):
    """cases: (ntotal, rows_q, k, nlist, group, n_cu) -> (served, blocks, kprime, keys) each; the program's own sweep
    runs first and must pass."""
    args = [str(v) for c in cases for v in c]
    p = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    lines = p.stdout.strip().splitlines()
    assert lines[-1].startswith("ok ") and len(lines) == len(cases) + 1
    out = []
    for c, line in zip(cases, lines):
        got = tuple(int(x) for x in line.split())
        assert got[:6] == tuple(c), (got, c)
        out.append(got[6:])
    return out


def test_host_plan_sweep_and_declines(plan_exe):
    """The program's sweep (served and declined shapes, every switch alone declines, the other kinds unmoved), and by
    hand: declined below 4096 rows of bound, past the nlist cap, for a k the key lists cannot take; the predicate does
    not look at the group size."""
    n = 200_000
    rq = 28_000  # (64 of 447 lists)
    cases = [(n, rq, 50, 447, g, 256) for g in (2, 3, 16)]
    cases += [(4095, 4095, 10, 8, 16, 256), (4096, 4096, 10, 8, 2, 256), (100_000, 2047, 10, 447, 16, 256),
              (100_000, 2048, 10, 447, 2, 256), (n, rq, 50, SH.MAX_NLIST, 2, 256), (n, rq, 50, SH.MAX_NLIST + 1, 2, 256),
              (n, rq, 2048, 447, 16, 256), (n, rq, 1000, 447, 16, 256), (n, 2800, 10, 447, 2, 256),
              (n, 2800, 10, 447, 16, 256)]
    got = run_plan(plan_exe, cases)
    assert [g[0] for g in got] == [1, 1, 1, 0, 1, 0, 1, 1, 0, 0, 1, 1, 1]
    assert all((g[3] > 0) == bool(g[0]) for g in got)
    assert got[5] == (0, 0, 0, 0), "a group of 16 whose two-query bound is below the threshold is not served"
    assert got[11][1] < got[12][1] <= 256, "16 queries probe more rows than 2: more workgroups, one per CU at most"
    assert got[2][1] <= 256 and got[10][3] == 8


def test_every_shape_of_the_gpu_tests_is_planned_as_the_tests_expect(plan_exe):
    """A declined plan must not turn a GPU test into a test of the per-query chains: every (corpus, k, nprobe, group)
    tests/test_ivf_batch_gpu.py launches is served at 256 CUs with keys > 0, and its two declining cases decline."""
    cases = SH.plan_cases()
    got = run_plan(plan_exe, [(n, rq, k, nlist, g, 256) for _, n, rq, k, nlist, g, _ in cases])
    for (name, n, rq, k, nlist, g, served), (ok, blocks, kprime, keys) in zip(cases, got):
        assert bool(ok) == served and (keys > 0) == served, (name, n, rq, k, g, ok, blocks, kprime, keys)
        if served:
            assert blocks >= 2, (name, blocks)  # more than one workgroup
    # the served-again case relies on three keys per lane: four adjacent best rows overflow one lane's list
    by_name = {c[0]: g for c, g in zip(cases, got)}
    assert by_name["axes nprobe=1"][3] == 3 and by_name["ties"][3] == 3


def test_union_model_against_a_brute_force_union():
    """The numpy model of the union step: list-major, storage order inside a list, every position's mask is its list's,
    the padding names no query; checked against sets built row by row."""
    rng = np.random.default_rng(5)
    nlist, n, g, nprobe = 23, 997, 5, 4
    assign = rng.integers(0, nlist, n).astype(np.int32)
    assign[assign == 7] = 8  # an empty list
    sizes, off, ids = SH.layout(assign, nlist)
    assert sizes[7] == 0 and np.array_equal(np.sort(ids), np.arange(n))
    probe = np.stack([rng.choice(nlist, nprobe, replace=False) for _ in range(g)])
    probe[0, 0], probe[1, 1] = 7, -1
    lmask, lpre, urow, uid, umask = SH.union_model(probe, off, ids)
    m = int(lpre[-1])
    want = sorted((int(assign[r]), r) for r in range(n) if any(assign[r] in probe[qi] for qi in range(g)))
    assert m == len(want) and [int(x) for x in uid[:m]] == [r for _, r in want]
    assert np.array_equal(ids[urow[:m]], uid[:m]) and (np.diff(urow[:m]) > 0).all()
    for p in range(m):
        qs = {qi for qi in range(g) if assign[uid[p]] in probe[qi]}
        assert umask[p] == sum(1 << qi for qi in qs) and qs
    assert urow.shape[0] % 16 == 0 and urow.shape[0] - m < 16 and not umask[m:].any()
    empty = SH.union_model(np.full((2, 3), -1), off, ids)
    assert int(empty[1][-1]) == 0 and empty[2].shape[0] == 16 and not empty[4].any()


def test_a_tile_of_the_masks_case_spans_a_list_boundary():
    sizes = SH.axes_sizes()
    assert (sizes % 16 != 0).all() and sizes[SH.AX_BIG] >= SH.MIN_ROWS
    _, _, assign = SH.axes()
    assert np.array_equal(np.bincount(assign, minlength=SH.AX_NLIST), sizes)
    _, off, ids = SH.layout(assign, SH.AX_NLIST)
    _, lpre, _, _, umask = SH.union_model(np.array([[0, 1], [2, 3]]), off, ids)
    tiles = umask.reshape(-1, 16)
    mixed = [t for t in range(tiles.shape[0]) if len(set(tiles[t][tiles[t] != 0])) > 1]
    assert mixed and int(lpre[2]) // 16 in mixed, "the boundary between query 0's lists and query 1's lies inside a tile"


@pytest.mark.parametrize("L, V", [(16, 3), (64, 4)])
def test_union_kernel_resources_and_matrix_instruction(tmp_path, L, V):
    """d = 384 (16 lanes x 3 chunks) and d = 1024 (64 x 4), the lightest (3 keys per lane) and the heaviest (8 keys)
    union instantiation of each: no scratch, no spill, at most 256 VGPRs + AGPRs (__launch_bounds__(256, 2)); the
    emitted code carries the 16x16x4 f32 MFMA and 16-byte nontemporal row loads."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = CSRC / "ls_ivf_batch.hip"
    asm = tmp_path / f"ivfb_{L}_{V}.s"
    p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=fast",
                        "-Rpass-analysis=kernel-resource-usage", "-DLS_IVFB_KERNEL_ONLY", f"-DLS_IVFB_ONLY_L={L}",
                        f"-DLS_IVFB_ONLY_V={V}", "--cuda-device-only", "-S", str(src), "-o", str(asm)],
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
    # <L, V, M, one B block, four waves, the union source>
    kernels = {n: u for n, u in usage.items() if re.search(rf"ls_mq_kernelILi{L}ELi{V}ELi\d+ELi1ELi4EJ12mq_union_srcEE", n)}
    assert len(kernels) == 2, sorted(usage)
    assert {re.search(rf"ILi{L}ELi{V}ELi(\d+)E", n).group(1) for n in kernels} == {"3", "8"}
    for n, u in kernels.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u.get("VGPRs Spill", 0) == 0, (n, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 256, (n, u)
    text = asm.read_text()
    assert "v_mfma_f32_16x16x4_f32" in text
    assert re.search(r"global_load_dwordx4 .* nt", text)
