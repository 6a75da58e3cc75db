"""The bf16 storage dtype without a GPU (include/leansearch_bf16.h): the ABI surface, the refusals that
come before any device check, the host restatement of the encoding (lean_explore_amd/bf16.py), the plain-C restatement
of a row's score (tests/bf16_ref.c) against float64, and what the gfx950 compile reports of the bf16 kernels beside the
fp16 kernels of the same shape."""

import ctypes
import re
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

from lean_explore_amd import bf16, faiss_compat, native
from lean_explore_amd import search as S
from lean_explore_amd.index import FlatIPIndex, switch_refusal
from lean_explore_amd.ivf import IVFFlatIndex
from oracle import oracle
from tests import helpers as H
from tests.test_geometry_cpu import GEOMS, geom_of
from tests.test_sq8_cpu import NEG, exact_topk

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "lean-explore_amd" / "csrc"
HEADER = ROOT / "include" / "leansearch.h"
BF16_HEADER = ROOT / "include" / "leansearch_bf16.h"
BF = native.LS_DTYPE_BF16


# ---- shared with tests/test_bf16_gpu.py ---------------------------------------------------------------------------------
def geom(d):
    """(chunks, L, V) of a bf16 row of d elements: the fp16 index's geometry."""
    L, V = geom_of("f16", d)
    return L * V, L, V


_ref_lib = None
_ref_dir = None


def ref_lib():
    """tests/bf16_ref.c, built once per process into a temporary directory (as test_sq8_cpu.py::ref_lib builds its own)."""
    global _ref_lib, _ref_dir
    if _ref_lib is None:
        _ref_dir = tempfile.TemporaryDirectory(prefix="bf16_ref_")
        so = Path(_ref_dir.name) / "libbf16_ref.so"
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", str(ROOT / "tests" / "bf16_ref.c"), "-o",
                        str(so), "-lm"], check=True)
        _ref_lib = ctypes.CDLL(str(so))
        _ref_lib.bf16_ref_scores.restype = None
        _ref_lib.bf16_ref_scores.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_void_p, ctypes.c_void_p]
    return _ref_lib


def padded_bits(bits, chunks):
    out = np.zeros((bits.shape[0], chunks * 8), np.uint16)
    out[:, :bits.shape[1]] = bits
    return out


def ref_scores(bits_padded, g, qn):
    """Scores [nq, n] of bf16_ref.c; qn [nq, d] float32: the queries as the kernels see them, padded here."""
    chunks, L, V = g
    lib = ref_lib()
    n = bits_padded.shape[0]
    qp = np.zeros((qn.shape[0], chunks * 8), np.float32)
    qp[:, :qn.shape[1]] = qn
    out = np.empty((qn.shape[0], n), np.float32)

    def one(i):
        lib.bf16_ref_scores(bits_padded.ctypes.data, n, chunks, L, V, qp[i].ctypes.data, out[i].ctypes.data)

    with ThreadPoolExecutor(max_workers=min(16, max(qn.shape[0], 1))) as ex:  # (ctypes releases the GIL)
        list(ex.map(one, range(qn.shape[0])))
    return out


def ref_of(corpus, qn):
    """bf16_ref.c's scores [nq, n] of bf16.encode(corpus) for the queries as the kernels see them."""
    g = geom(corpus.shape[1])
    return ref_scores(padded_bits(bf16.encode(corpus), g[0]), g, qn)


# the encoding, bit pattern by bit pattern: (float32 bits, bf16 bits)
ENCODE_TABLE = [
    (0x3F800000, 0x3F80),  # 1.0
    (0x3F808000, 0x3F80),  # an exact half: down to the even neighbour
    (0x3F818000, 0x3F82),  # an exact half: up to the even neighbour
    (0x3F808001, 0x3F81),  # just above the half
    (0x3F807FFF, 0x3F80),  # just below it
    (0xBF818000, 0xBF82),  # the sign does not change the direction
    (0x7F7FFFFF, 0x7F80),  # FLT_MAX lies above the largest bf16: +inf
    (0xFF7FFFFF, 0xFF80),
    (0x7F7F7FFF, 0x7F7F),  # the largest value that still rounds to the largest bf16
    (0x7F7F8000, 0x7F80),  # the half above it goes to even: inf
    (0x00000001, 0x0000),  # the smallest f32 subnormal
    (0x00008000, 0x0000),  # half of the smallest bf16 subnormal: to even, zero
    (0x00008001, 0x0001),
    (0x00010000, 0x0001),  # the smallest bf16 subnormal is kept
    (0x00018000, 0x0002),
    (0x007F0000, 0x007F),  # the largest bf16 subnormal
    (0x007FFFFF, 0x0080),  # the largest f32 subnormal rounds up into the normals
    (0x80000000, 0x8000),  # -0 is kept
    (0x80010000, 0x8001),
    (0x7F800000, 0x7F80),  # +-inf
    (0xFF800000, 0xFF80),
    (0x7FC00000, 0x7FC0),  # the default NaN
    (0x7F800001, 0x7FC0),  # a NaN whose payload sits in the low half only stays a NaN
    (0xFF80FFFF, 0xFFC0),
    (0x7FA50000, 0x7FE5),  # a signalling NaN is made quiet, its top payload bits kept
]


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def test_header_constant_and_symbols():
    m = re.search(r"#define\s+LS_DTYPE_BF16\s+(\d+)", HEADER.read_text())
    assert m and int(m.group(1)) == native.LS_DTYPE_BF16 == 3
    text = re.sub(r"/\*.*?\*/", "", BF16_HEADER.read_text(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ls_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(native.BF16_SYMBOLS) == ["ls_bf16_inexact", "ls_bf16_rows", "ls_ivf_bf16_inexact"]
    raw = ctypes.CDLL(str(native.LIB_PATH))
    lib = native.load()
    for n in names:
        assert hasattr(raw, n), f"{n} is not exported"
        assert getattr(lib, n).argtypes == native.BF16_SYMBOLS[n][1]
    assert FlatIPIndex(8, dtype="bf16").storage_dtype == FlatIPIndex(8, dtype="bfloat16").storage_dtype == "bf16"
    assert IVFFlatIndex(8, 4, dtype="bf16").storage_dtype == "bf16"


# ---- refusals, all before any device check (device 9999 exists nowhere) ---------------------------------------------------
@pytest.mark.parametrize("fn", ["ls_create_l2", "ls_create_l2_from_device"])
def test_l2_creates_refuse_bf16_before_any_device_check(fn):
    lib = native.load()
    x = np.ones((4, 8), np.float32)
    h = ctypes.c_void_p(1)
    assert getattr(lib, fn)(ctypes.byref(h), x.ctypes.data, 4, 8, BF, 9999) == native.LS_ERR_INVALID_ARG
    assert b"bf16" in lib.ls_last_error() and not h.value


def test_ivf_l2_create_refuses_bf16_before_any_device_check():
    lib = native.load()
    x = np.ones((4, 8), np.float32)
    cent = np.ones((2, 8), np.float32)
    h = ctypes.c_void_p(1)
    assert lib.ls_ivf_create_l2(ctypes.byref(h), x.ctypes.data, 4, 8, BF, cent.ctypes.data, 2, None,
                                9999) == native.LS_ERR_INVALID_ARG
    assert b"bf16" in lib.ls_last_error() and not h.value


@pytest.mark.parametrize("fn", ["ls_create_sharded", "ls_create_replicated"])
def test_sharded_and_replicated_creation_refuse_bf16_before_looking_for_devices(fn):
    lib = native.load()
    x = np.ones((4, 8), np.float32)
    ids = (ctypes.c_int32 * 2)(9998, 9999)
    h = ctypes.c_void_p()
    assert getattr(lib, fn)(ctypes.byref(h), x.ctypes.data, 4, 8, BF, ids, 2) == native.LS_ERR_INVALID_ARG
    assert b"bf16" in lib.ls_last_error()
    # ... also with no device list at all, where f32 and fp16 answer LS_ERR_NO_DEVICE
    assert getattr(lib, fn)(ctypes.byref(h), x.ctypes.data, 4, 8, BF, ids, 0) == native.LS_ERR_INVALID_ARG
    blocks = (ctypes.c_void_p * 2)(1, 1)
    rows = (ctypes.c_int64 * 2)(2, 2)
    assert lib.ls_create_sharded_from_device(ctypes.byref(h), blocks, rows, 8, BF, ids, 2) == native.LS_ERR_INVALID_ARG
    assert b"bf16" in lib.ls_last_error()


def test_no_device_without_a_gpu(gpu_available):
    """The creates that accept LS_DTYPE_BF16 get as far as the device check (an unknown dtype would not)."""
    if gpu_available:
        return  # (nothing to observe on a GPU box: tests/test_bf16_gpu.py runs there)
    lib = native.load()
    x = np.ones((4, 8), np.float32)
    h = ctypes.c_void_p()
    assert lib.ls_create(ctypes.byref(h), x.ctypes.data, 4, 8, BF, 0) == native.LS_ERR_NO_DEVICE
    assert lib.ls_create_from_device(ctypes.byref(h), x.ctypes.data, 4, 8, BF, 0) == native.LS_ERR_NO_DEVICE
    cent = np.ones((2, 8), np.float32)
    assert lib.ls_ivf_create(ctypes.byref(h), x.ctypes.data, 4, 8, BF, cent.ctypes.data, 2, None,
                             0) == native.LS_ERR_NO_DEVICE
    assert lib.ls_create(ctypes.byref(h), x.ctypes.data, 4, 2049, BF, 0) == native.LS_ERR_INVALID_ARG  # d <= 2048


# (switch, enable) -> the words of the refusal; None: LS_OK. The rule table of csrc/ls_switch_plan.h for a bf16 handle.
SWITCH_RULES = [
    ("LS_SW_F16", 1, "ls_set_f16_small_batch: the index stores bf16 rows"),
    ("LS_SW_F16", 0, "ls_set_f16_small_batch: the index stores bf16 rows"),  # (this switch's rule does not look at enable)
    ("LS_SW_SQ8", 1, "ls_set_sq8_small_batch: the index stores bf16 rows"),
    ("LS_SW_SQ8", 0, "ls_set_sq8_small_batch: the index stores bf16 rows"),  # (nor does this one's)
    ("LS_SW_SUBSET", 1, "ls_set_subset_small_batch: the index stores bf16 rows"),
    ("LS_SW_SUBSET", 0, None),
    ("LS_SW_L2", 1, "ls_set_l2_small_batch: not an L2 index"),
    ("LS_SW_L2", 0, "ls_set_l2_small_batch: not an L2 index"),
    ("LS_SW_IVF", 1, "ls_ivf_set_small_batch: the index stores bf16 rows"),
    ("LS_SW_IVF", 0, None),
]


def test_switch_rules_of_a_bf16_handle(tmp_path):
    """csrc/ls_switch_plan.h in a plain host program: what ls_switch_ask answers a single-device inner-product handle of
    bf16 rows, switch by switch, and that no answer for the other three dtypes mentions bf16."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host check of ls_switch_plan.h"
    src = tmp_path / "bf16_switch.cpp"
    src.write_text('#include <cstdio>\n#include "ls_switch_plan.h"\nint main() {\n'
                   '  for (int dt = 0; dt < 4; ++dt) for (int sw = 0; sw < LS_SW_COUNT; ++sw) for (int en = 0; en < 2; ++en) {\n'
                   '    const ls_switch_answer a = ls_switch_ask((ls_switch)sw, LS_METRIC_INNER_PRODUCT, dt, sw == LS_SW_IVF ? '
                   'LS_PLACE_NA : LS_PLACE_SINGLE, en);\n'
                   '    char msg[512] = "";\n    if (a.rc != LS_OK) snprintf(msg, sizeof msg, a.fmt, a.fill);\n'
                   '    printf("%d|%d|%d|%d|%s\\n", dt, sw, en, a.rc, msg);\n  }\n  return 0;\n}\n')
    exe = tmp_path / "bf16_switch"
    p = subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Wno-format-security", "-Wno-format-nonliteral",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(CSRC), str(src), "-o",
                        str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and not p.stderr.strip(), p.stderr[-2000:]
    order = ["LS_SW_F16", "LS_SW_SQ8", "LS_SW_SUBSET", "LS_SW_L2", "LS_SW_IVF"]
    got = {}
    for line in p.stdout.splitlines():
        dt, sw, en, rc, msg = line.split("|", 4)
        got[(int(dt), order[int(sw)], int(en))] = (int(rc), msg)
    assert len(got) == 4 * 5 * 2
    for sw, en, words in SWITCH_RULES:
        rc, msg = got[(BF, sw, en)]
        if words is None:
            assert rc == native.LS_OK, (sw, en, msg)
        else:
            assert rc == native.LS_ERR_INVALID_ARG and msg.startswith(words), (sw, en, msg)
            if "L2" not in sw:
                assert "bf16 rows" in msg
    assert not any("bf16" in msg for (dt, _, _), (_, msg) in got.items() if dt != BF)


def test_switch_setters_refuse_a_null_handle_and_python_mirrors_the_rules():
    for name in ("f16", "sq8", "subset", "ivf"):
        assert "bf16 rows" in switch_refusal(name, "ip", "bf16"), name
    assert switch_refusal("l2", "ip", "bf16").startswith("l2_small_batch needs metric='l2'")
    for kw in ("f16_small_batch", "sq8_small_batch", "subset_small_batch"):
        with pytest.raises(ValueError, match="bf16 rows"):
            FlatIPIndex(8, dtype="bf16", **{kw: True})
    ix = FlatIPIndex(8, dtype="bf16")
    for setter in (ix.set_f16_small_batch, ix.set_sq8_small_batch, ix.set_subset_small_batch):
        with pytest.raises(ValueError, match="bf16 rows"):
            setter(True)
        setter(False)  # (switching one off is never refused by the Python table)
    with pytest.raises(ValueError, match="bf16 rows"):
        IVFFlatIndex(8, 4, dtype="bf16", small_batch=True)
    IVFFlatIndex(8, 4, dtype="bf16").set_small_batch(False)


def test_python_refusals(tmp_path):
    with pytest.raises(ValueError, match="bf16"):
        FlatIPIndex(8, dtype="bf16", metric="l2")
    with pytest.raises(ValueError, match="bf16"):
        IVFFlatIndex(8, 4, dtype="bf16", metric="l2")
    with pytest.raises(ValueError, match="bf16"):
        faiss_compat.IndexFlatL2(8, dtype="bf16")
    with pytest.raises(ValueError, match="bf16"):
        FlatIPIndex(8, dtype="bf16", devices=[0, 1])
    with pytest.raises(ValueError, match="bf16"):
        FlatIPIndex.from_array(np.ones((4, 8), np.float32), dtype="bf16", devices=[0, 0], replicate=True)
    with pytest.raises(ValueError, match="bf16"):
        S.SearchEngine(index=object(), ids_map=[], lexical_retriever=False, storage_dtype="bf16", devices=[0, 1])
    with pytest.raises(ValueError, match="'bf16'"):  # the dtype error names the new dtype
        FlatIPIndex(8, dtype="int8")
    with pytest.raises(ValueError, match="bf16"):
        FlatIPIndex(8, dtype="f32").bf16_inexact
    with pytest.raises(ValueError, match="bf16"):
        FlatIPIndex(8, dtype="f16").bf16_rows()
    assert faiss_compat.IndexFlatIP(8, dtype="bf16").storage_dtype == "bf16"
    assert faiss_compat.IndexIVFFlat(None, 8, 4, ivf=True, dtype="bf16").storage_dtype == "bf16"
    from lean_explore_amd.sharded import ShardedFlatIPIndex

    with pytest.raises(ValueError, match="bf16"):
        ShardedFlatIPIndex.from_array(np.ones((4, 8), np.float32), dtype="bf16")


# ---- the encoding -------------------------------------------------------------------------------------------------------
def test_encode_on_hand_written_bit_patterns():
    u = np.array([a for a, _ in ENCODE_TABLE], np.uint32)
    want = np.array([b for _, b in ENCODE_TABLE], np.uint16)
    got = bf16.encode(u.view(np.float32))
    assert got.dtype == np.uint16 and [hex(v) for v in got] == [hex(v) for v in want]
    # what the table says in values
    x = u.view(np.float32)
    back = bf16.decode(got)
    assert np.isnan(back[np.isnan(x)]).all() and back[6] == np.inf and back[7] == -np.inf  # (FLT_MAX, -FLT_MAX)
    assert np.signbit(back[17]) and back[17] == 0.0  # (-0)
    assert bf16.inexact(x) == sum(1 for (a, b) in ENCODE_TABLE if (b << 16) != a and (a & 0x7FFFFFFF) <= 0x7F800000)


def test_decode_of_encode_is_the_identity_on_every_bf16_value():
    bits = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)  # every bf16 bit pattern
    x = bf16.decode(bits)
    assert x.dtype == np.float32 and np.array_equal(x.view(np.uint32), bits.astype(np.uint32) << 16)
    again = bf16.encode(x)
    nan = np.isnan(x)
    assert np.array_equal(again[~nan], bits[~nan])  # every x that is already bf16-valued is kept, bit for bit
    assert (again[nan] == (bits[nan] | 0x0040)).all()  # a NaN is kept as a NaN (made quiet)
    assert np.array_equal(bf16.decode(again)[~nan].view(np.uint32), x[~nan].view(np.uint32))
    assert bf16.inexact(x) == 0
    # and encode rounds to the NEAREST value: never further than half a bf16 step of the operand's binade
    y = H.gauss(3, 64, 257, normalize=False)
    err = np.abs(bf16.decode(bf16.encode(y)).astype(np.float64) - y)
    assert (err <= np.abs(y) * 2.0 ** -8).all() and bf16.inexact(y) > 0


# ---- tests/bf16_ref.c alone, against float64 -------------------------------------------------------------------------------
REF_DIMS = [128, 250, 384, 500, 768, 1024, 1500, 2048, 100, 1001]  # one per geometry, and two ragged ones


def test_restatement_dimensions_are_one_per_geometry():
    assert sorted(geom_of("f16", d) for d in REF_DIMS[:8]) == sorted(GEOMS["f16"])
    assert all(d % 8 for d in REF_DIMS[8:])


@pytest.mark.parametrize("d", REF_DIMS)
def test_c_restatement_against_float64(d):
    """bf16_ref.c at each of the eight geometries against the float64 product of the decoded rows, unit-norm Gaussian
    rows and queries: scores within the project's 1e-5 bar, and the top-50 equal except where the float64 scores lie
    within 2e-6 - the reference alone stays inside the bars the project already uses."""
    n, k = 500, 50
    corpus = H.gauss(d, n, d)
    q = H.gauss(d + 1, 4, d)
    got = ref_of(corpus, q)
    dec = bf16.decode(bf16.encode(corpus))
    want = q.astype(np.float64) @ dec.astype(np.float64).T
    assert got.shape == want.shape == (4, n)
    print(f"d={d}: max |bf16_ref.c - float64| = {np.abs(got - want).max():.3e}")
    assert np.abs(got - want).max() <= 1e-5
    for i in range(4):
        _, I = exact_topk(got[i], k)
        Ir = np.lexsort((np.arange(n), -want[i]))[:k]
        for a, b in zip(I, Ir):
            assert a == b or abs(want[i][a] - want[i][b]) <= 2e-6, (d, i, a, b)


def test_c_restatement_is_exact_on_integer_rows():
    """Integer-valued rows and queries (|values| <= 64) are exact in bf16 and in any summation order."""
    d, n = 250, 300
    corpus = H.int_corpus(5, n, d, -64, 65)
    q = H.int_corpus(6, 3, d, -64, 65)
    assert bf16.inexact(corpus) == 0
    want = q.astype(np.int64) @ corpus.astype(np.int64).T
    assert np.abs(want).max() < 2 ** 24 and np.array_equal(ref_of(corpus, q).astype(np.int64), want)


# ---- what the compiler reports --------------------------------------------------------------------------------------------
def resource_usage(name, tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=fast",
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S", str(CSRC / name), "-o",
                        str(tmp_path / (name + ".s"))], capture_output=True, text=True, timeout=1800)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, fn = {}, None
    for line in p.stderr.splitlines():  # (the remarks only)
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            fn = m.group(1)
            usage[fn] = {}
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|"
                      r"Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and fn:
            usage[fn][m.group(1)] = int(m.group(2))
    return usage


def keyed(usage, tag):
    """{(kernel, L, V, SMALL, list): usage} of the single-query instantiations whose pack ends in `tag` ('' : the plain
    fp16 kernels, F16 = true). Itanium names: ls_scan_kernel<F16, L, V, U, NQ, SMALL, pack...>, ls_ivf_scan_kernel<F16,
    L, V, U, pack...>; `PKj` is the row list, `11ls_bf16_arg` the tag."""
    out = {}
    for fn, u in usage.items():
        m = re.match(r"_Z14ls_scan_kernelILb([01])ELi(\d+)ELi(\d+)ELi\d+ELi1ELb([01])EJ(.*?)EEv", fn)
        if m:
            key = ("scan", int(m.group(2)), int(m.group(3)), m.group(4) == "1")
        else:
            m = re.match(r"_Z18ls_ivf_scan_kernelILb([01])ELi(\d+)ELi(\d+)ELi\d+EJ(.*?)EEv", fn)
            if not m:
                continue
            key = ("ivf", int(m.group(2)), int(m.group(3)), False)
        pack = m.groups()[-1]
        f16 = m.group(1) == "1"
        rest = pack.replace("PKj", "", 1) if pack.startswith("PKj") else pack
        if (tag and rest == tag and not f16) or (not tag and rest == "" and f16):
            out[key + (pack.startswith("PKj"),)] = u
    return out


def test_bf16_kernels_spill_no_more_than_the_fp16_kernels_beside_them(tmp_path):
    """ls_bf16_scan.hip and ls_bf16_ivf.hip compiled for gfx950 beside ls_scan.hip, ls_ivf.hip and ls_ivf_subset.hip: every
    bf16 instantiation reports scratch, VGPR spills and SGPR spills no greater than the fp16 instantiation of the same
    (L, V, SMALL, list). The bound is the parent's own kernels', whatever they are. DESIGN.md 4.13 holds the table this
    prints."""
    with ThreadPoolExecutor(max_workers=5) as ex:
        reports = list(ex.map(lambda n: resource_usage(n, tmp_path),
                              ["ls_bf16_scan.hip", "ls_bf16_ivf.hip", "ls_scan.hip", "ls_ivf.hip", "ls_ivf_subset.hip"]))
    bf = {**keyed(reports[0], "11ls_bf16_arg"), **keyed(reports[1], "11ls_bf16_arg")}
    fp = {**keyed(reports[2], ""), **keyed(reports[3], ""), **keyed(reports[4], "")}
    want = {(kern, L, V, small, lst) for kern in ("scan", "ivf") for (L, V) in GEOMS["f16"]
            for small in ((False, True) if kern == "scan" else (False,)) for lst in (False, True)}
    assert set(bf) == want and set(fp) >= want, (sorted(want - set(bf)), sorted(want - set(fp)))
    fields = ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill")
    print("kernel L V SMALL list | bf16: VGPRs AGPRs scratch vgpr-spill sgpr-spill occupancy | fp16: the same")
    worse = []
    for key in sorted(want):
        b, f = bf[key], fp[key]
        row = lambda u: " ".join(str(u.get(x, 0)) for x in ("VGPRs", "AGPRs") + fields + ("Occupancy [waves/SIMD]",))
        print(*key, "|", row(b), "|", row(f))
        worse += [(key, x, b.get(x, 0), f.get(x, 0)) for x in fields if b.get(x, 0) > f.get(x, 0)]
    assert not worse, worse
