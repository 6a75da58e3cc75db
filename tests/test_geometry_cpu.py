"""Row geometries (L, V) of the scan kernels without a GPU, and everything tests/test_geometry_gpu.py shares: the
dimensions it sweeps, the host restatement of the SMALL launch rule, the plan of launches per case, and the host-only
references (no library search call inside any of them).

A stored row is `chunks` 16-byte chunks; L lanes share a row and each takes V chunks (ls_pick_geom, csrc/ls_prep.hip).
Every (L, V) is one instantiation of the scan template per path (plain scan, row-list scan, IVF probed-list scan), and
the plain and row-list scans have a SMALL and a non-SMALL variant each. The tables below must reach all of them: the
coverage tests here fail when a change to the geometry table or to a dimension list drops one."""

import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from lean_explore_amd import native, sq8
from oracle import oracle
from tests import helpers as H
from tests.test_sq8_cpu import NEG, exact_topk, geom, padded_codes, ref_scores

N = 3001  # odd: no multiple of any tile
NQ = 4    # queries 0, 1 run with normalize=True, queries 2, 3 without

DIMS = {
    "sq8": [1, 17, 128, 129, 250, 256, 257, 384, 385, 500, 512, 513, 760, 768, 769, 1000, 1024, 1025, 1530, 1536, 1537,
            2000, 2048, 2049, 3000, 3072, 3073, 4090, 4096],
    "f32": [1, 3, 64, 65, 100, 128, 129, 190, 192, 193, 256, 257, 384, 385, 500, 512, 513, 768, 769, 1000, 1024],
    "f16": [1, 8, 128, 129, 256, 257, 384, 385, 512, 513, 768, 769, 1024, 1025, 1536, 1537, 2048],
}
SHARED_GEOMS = [(16, 1), (16, 2), (16, 3), (16, 4), (32, 3), (32, 4), (64, 3), (64, 4)]
GEOMS = {"sq8": [(8, 1), (8, 3)] + SHARED_GEOMS, "f32": SHARED_GEOMS, "f16": SHARED_GEOMS}
PER_CHUNK = {"sq8": 16, "f16": 8, "f32": 4}   # elements of a 16-byte chunk
MAX_D = {"sq8": 4096, "f16": 2048, "f32": 1024}  # a stored row is at most 4096 bytes
# The coarse quantiser of an IVF index is an f32 index of the centroids, so an IVF index exists for d <= 1024 only
# (ls_ivf_create refuses a larger d whatever the rows' dtype): the probed-list kernels of the geometries that begin
# past d = 1024 cannot be launched through the library.
IVF_MAX_D = MAX_D["f32"]


def geom_of(dtype, d):
    """(L, V) of a stored row: ls_sq8_geom for sq8, the oracle's table for f32; an f16 row of d elements has the chunks
    of an f32 row of ceil(d / 2)."""
    if dtype == "sq8":
        rc, g = geom(d)
        assert rc == native.LS_OK, d
        return g[1], g[2]
    return oracle.geom_f32(d if dtype == "f32" else (d + 1) // 2)


# ---- the launch rule (csrc/ls_scan_plan.h: ls_scan_small_unroll, ls_scan_tile_rows, ls_scan_is_small and
# ls_scan_blocks_lv, which ls_scan_launch of csrc/ls_scan_launch.h and ls_scan_blocks apply), restated;
# test_restated_launch_rule_is_the_code_s_own below holds the restatement to that header ----------------------------------
#   U = 4 for V >= 3, else 8 row groups in flight; TR = U * 64 / L rows per tile;
#   SMALL  <=>  one query per launch  and  ceil(ceil(rows / TR) / (4 * blocks)) * TR <= 64  and  blocks <= 256;
#   blocks = debug option 7 when set, else ceil(ceil(rows / TR) / 16) (at least 4 tiles per wave; far below the cap of
#   two workgroups per CU at the sizes used here);
#   the SMALL row-list kernel of sq8 rows with V == 4 is built with U = 2 and the rule uses that TR.
def tile_rows(L, V, sq8_rowlist=False):
    U = 2 if (sq8_rowlist and V == 4) else (4 if V >= 3 else 8)
    return U * (64 // L)


def default_blocks(rows, L, V):
    tiles = -(-rows // tile_rows(L, V))
    return max(1, -(-tiles // 16))


def is_small(rows, blocks, L, V, sq8_rowlist=False):
    TR = tile_rows(L, V, sq8_rowlist)
    tiles_per_wave = -(-(-(-rows // TR)) // (4 * blocks))
    return tiles_per_wave * TR <= 64 and blocks <= 256


# ---- the plan of a flat / subset case: (path, selection, debug option 7) ------------------------------------------------
# At n = 3001 option 7 = 4 gives every geometry 12 tiles or more per wave (non-SMALL) and option 7 = 256 gives every
# one a single tile per wave (SMALL). A 10 % mask (about 300 rows) is SMALL at 4 workgroups for every geometry, so
# the row-list scan also runs at 1 workgroup, where it is not.
PLAIN_OPTS = (0, 4, 256)
SUBSET_RUNS = (("mask10", 0), ("mask10", 1), ("mask10", 4), ("mask10", 256), ("forty", 0), ("one", 0), ("ones", 0),
               ("ones", 4))
PLAIN_K = (1, 10, 2048)
SUBSET_K = (1, 50, 2048)


def selections(n=N):
    rng = np.random.default_rng(31)
    return {"mask10": np.flatnonzero(rng.random(n) < 0.10), "forty": np.sort(rng.choice(n, 40, replace=False)),
            "one": np.array([1234]), "ones": np.arange(n)}


def variants_reached(dtype, d):
    """{(path, SMALL?)} the plan above launches for one (dtype, d), by the restated rule."""
    L, V = geom_of(dtype, d)
    out = set()
    for opt in PLAIN_OPTS:
        out.add(("plain", is_small(N, opt or default_blocks(N, L, V), L, V)))
    sel = selections()
    for name, opt in SUBSET_RUNS:
        m = sel[name].size
        out.add(("rowlist", is_small(m, opt or default_blocks(m, L, V), L, V, sq8_rowlist=dtype == "sq8")))
    return out


def ivf_dims(dtype):
    """One full and one ragged d per geometry an IVF index can have, taken from DIMS."""
    per, out = PER_CHUNK[dtype], []
    for g in GEOMS[dtype]:
        ds = [d for d in DIMS[dtype] if d <= IVF_MAX_D and geom_of(dtype, d) == g]
        full = [d for d in ds if d % per == 0]
        ragged = [d for d in ds if d % per]
        if full and ragged:
            out += [max(full), max(ragged)]
    return out


def ivf_unreachable(dtype):
    return [g for g in GEOMS[dtype] if all(geom_of(dtype, d) != g for d in range(1, IVF_MAX_D + 1))]


# ---- references -----------------------------------------------------------------------------------------------------------
class Flat:
    """Host reference of one corpus and dtype over any ascending row list. qn: the queries as the kernels see them
    (normalised already where the call normalises: oracle.c_normalize_l2 sums the squares in the kernels' order).
      f32: oracle.c_search(order="scan") - the scan kernels' own summation order, bit for bit;
      f16: oracle.c_search(f16=True) - bit for bit on integer-valued data, the project's bars otherwise;
      sq8: tests/sq8_ref.c at the geometry ls_sq8_geom names, then exact_topk.
    step: the sq8 step to encode with (a handle that was mutated keeps the step it was built with); default: trained
    on `corpus`."""

    def __init__(self, corpus, dtype, step=None):
        self.corpus, self.dtype, self.d = corpus, dtype, corpus.shape[1]
        self._scores = {}
        if dtype == "sq8":
            self.step = sq8.train_step(corpus) if step is None else np.asarray(step, np.float32)
            self.codes = sq8.encode(corpus, self.step)
            rc, self.g = geom(self.d)
            assert rc == native.LS_OK
            self.cp = padded_codes(self.codes, self.g[0])

    def sq8_scores(self, qn):
        key = qn.tobytes()
        if key not in self._scores:
            self._scores[key] = ref_scores(self.cp, self.g, qn * self.step)  # float32: the second rounded multiply
        return self._scores[key]

    def topk(self, rows, qn, k):
        nq = qn.shape[0]
        if rows.size == 0:
            return np.full((nq, k), NEG, np.float32), np.full((nq, k), -1, np.int64)
        if self.dtype == "sq8":
            S = self.sq8_scores(qn)[:, rows]
            out = [exact_topk(S[i], k, rows) for i in range(nq)]
            return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
        if self.dtype == "f16":
            D, I = oracle.c_search(self.corpus[rows], qn, k, f16=True)
        else:
            D, I = oracle.c_search(self.corpus[rows], qn, k, order="scan")
        return D, np.where(I >= 0, rows[np.maximum(I, 0)], -1)


def seen_queries(q, normalize):
    return oracle.c_normalize_l2(q) if normalize else np.ascontiguousarray(q, np.float32)


def ivf_reference(corpus, cent, assign, q, k, nprobe, normalize, dtype, flat=None):
    """The definition of include/leansearch_ivf.h on the host: the probed lists of a query are the top
    min(nprobe, nlist) centroids under the f32 scan order (the centroids are always an f32 index), the rows are those
    of the probed lists, the result is the dtype's flat reference over them. Returns (D, I, rows of every query).
    flat: a Flat of (corpus, dtype) to reuse."""
    flat = flat or Flat(corpus, dtype)
    qn = seen_queries(q, normalize)
    _, P = oracle.c_search(cent, qn, min(nprobe, cent.shape[0]), order="scan")
    D = np.empty((q.shape[0], k), np.float32)
    I = np.empty((q.shape[0], k), np.int64)
    rows_of = []
    for i in range(q.shape[0]):
        rows = np.flatnonzero(np.isin(assign, P[i][P[i] >= 0]))
        D[i], I[i] = (a[0] for a in flat.topk(rows, qn[i:i + 1], k))
        rows_of.append(rows)
    return D, I, rows_of


def assert_bars(D, I, corpus, rows, qn, k, f16):
    """The project's bars against the float64 twin over corpus[rows]: scores within 1e-5, an index may differ only
    where the twin's own scores are within 2e-6, recall 1.0. I holds original rows."""
    if rows.size == 0:
        assert (I == -1).all() and (D == NEG).all()
        return
    Dr, Ir, Sr = oracle.np_search(corpus[rows], qn, k, f16=f16)
    ok = I >= 0
    assert np.isin(I[ok], rows).all(), "a returned row is not among the searched rows"
    pos = np.where(ok, np.searchsorted(rows, np.maximum(I, 0)), -1)
    rep = oracle.compare_topk(D, pos, Dr, Ir, Sr, score_tol=1e-5, tie_eps=2e-6)
    assert rep["recall"] == 1.0, rep


def uneven_assignment(n=N, nlist=37, seed=5):
    """Lists 0 and 20 empty, list 36 one row, list 7 a third of the rows, the rest spread over the other lists."""
    rng = np.random.default_rng(seed)
    others = np.setdiff1d(np.arange(nlist), [0, 7, 20, 36])
    assign = others[rng.integers(0, others.size, n)].astype(np.int32)
    pick = rng.choice(n, n // 3 + 1, replace=False)
    assign[pick[:-1]] = 7
    assign[pick[-1]] = 36
    return assign


# ---- the geometry table ---------------------------------------------------------------------------------------------------
BOUNDARIES = [(128, (8, 8, 1)), (129, (16, 16, 1)), (256, (16, 16, 1)), (257, (24, 8, 3)), (384, (24, 8, 3)),
              (385, (32, 16, 2)), (512, (32, 16, 2)), (513, (48, 16, 3)), (768, (48, 16, 3)), (769, (64, 16, 4)),
              (1024, (64, 16, 4)), (1025, (96, 32, 3)), (1536, (96, 32, 3)), (1537, (128, 32, 4)),
              (2048, (128, 32, 4)), (2049, (192, 64, 3)), (3072, (192, 64, 3)), (3073, (256, 64, 4)), (1, (8, 8, 1)),
              (4096, (256, 64, 4))]


@pytest.mark.parametrize("d, want", BOUNDARIES)
def test_sq8_geometry_on_both_sides_of_every_boundary(d, want):
    assert geom(d) == (native.LS_OK, want)
    assert want[0] == want[1] * want[2] and want[0] * 16 >= d


@pytest.mark.parametrize("dtype", ["sq8", "f32", "f16"])
def test_the_library_has_exactly_these_geometries(dtype):
    """Every d a row can have maps to one of GEOMS[dtype], and every one of them occurs: a change to the table of
    ls_pick_geom (or of the oracle's twin) fails here instead of dropping coverage silently."""
    seen = {geom_of(dtype, d) for d in range(1, MAX_D[dtype] + 1)}
    assert seen == set(GEOMS[dtype])
    if dtype == "sq8":
        assert geom(MAX_D[dtype] + 1)[0] == native.LS_ERR_INVALID_ARG
    else:
        with pytest.raises(ValueError):
            geom_of(dtype, MAX_D[dtype] + 1)


def test_f32_and_sq8_tables_agree_where_they_overlap():
    """The oracle's f32 table (oracle/flat_ip_ref.c) and the library's (ls_sq8_geom) are two copies of one table: where
    the chunk counts coincide and the library does not pick an 8-lane geometry, they name the same (L, V)."""
    for d in range(1, MAX_D["f32"] + 1):
        rc, (chunks, L, V) = geom(4 * d)  # 4 d codes fill the chunks of d floats
        if L != 8:
            assert oracle.geom_f32(d) == (L, V), d


@pytest.mark.parametrize("dtype", ["sq8", "f32", "f16"])
def test_swept_dimensions_cover_every_geometry_and_both_variants(dtype):
    reached = {}
    for d in DIMS[dtype]:
        assert 1 <= d <= MAX_D[dtype]
        reached.setdefault(geom_of(dtype, d), set()).update(variants_reached(dtype, d))
    assert set(reached) == set(GEOMS[dtype])
    for g, v in reached.items():
        assert v == {("plain", True), ("plain", False), ("rowlist", True), ("rowlist", False)}, (dtype, g, v)
    # a full and a ragged last chunk, and both sides of the boundary, for every geometry
    per = PER_CHUNK[dtype]
    for g in GEOMS[dtype]:
        ds = [d for d in DIMS[dtype] if geom_of(dtype, d) == g]
        assert any(d % per == 0 for d in ds) and any(d % per for d in ds), (dtype, g, ds)
        hi = max(d for d in range(1, MAX_D[dtype] + 1) if geom_of(dtype, d) == g)
        assert hi in ds and (hi == MAX_D[dtype] or hi + 1 in DIMS[dtype]), (dtype, g, hi)


@pytest.mark.parametrize("d", sorted({d for ds in DIMS.values() for d in ds}))
def test_option_7_selects_the_variant_for_every_geometry(d):
    """The claim the GPU tests rest on: at n = 3001 debug option 7 = 4 is non-SMALL and = 256 is SMALL, whatever the
    geometry; a 40-row list is SMALL by size; a 10 % list is SMALL at 4 workgroups and not at 1."""
    sel = selections()
    assert 250 <= sel["mask10"].size <= 350
    for dtype in DIMS:
        if d > MAX_D[dtype]:
            continue
        L, V = geom_of(dtype, d)
        assert not is_small(N, 4, L, V) and is_small(N, 256, L, V)
        rl = dtype == "sq8"
        m = sel["mask10"].size
        assert is_small(40, default_blocks(40, L, V), L, V, rl)
        assert is_small(m, 4, L, V, rl) and is_small(m, 256, L, V, rl) and not is_small(m, 1, L, V, rl)
        assert not is_small(N, 4, L, V, rl)


@pytest.mark.parametrize("dtype", ["sq8", "f32", "f16"])
def test_ivf_dimensions_cover_every_geometry_an_ivf_index_can_have(dtype):
    dims = ivf_dims(dtype)
    got = {geom_of(dtype, d) for d in dims}
    assert got | set(ivf_unreachable(dtype)) == set(GEOMS[dtype]) and not got & set(ivf_unreachable(dtype))
    assert len(dims) == 2 * len(got) and all(d <= IVF_MAX_D for d in dims)
    assert ivf_unreachable(dtype) == {"f32": [], "f16": [(64, 3), (64, 4)],
                                      "sq8": [(32, 3), (32, 4), (64, 3), (64, 4)]}[dtype]


# ---- the restatements against float64 -------------------------------------------------------------------------------------
SQ8_REF_DIMS = [100, 200, 384, 500, 760, 1000, 1530, 2000, 3000, 4090]  # one per geometry


def test_sq8_restatement_dimensions_are_one_per_geometry():
    assert sorted(geom_of("sq8", d) for d in SQ8_REF_DIMS) == sorted(GEOMS["sq8"])


@pytest.mark.parametrize("d", SQ8_REF_DIMS)
def test_sq8_restatement_at_each_geometry_against_float64(d):
    """tests/sq8_ref.c at each of the ten geometries (part[64] holds L = 64) against the float64 product of the decoded
    rows: the bound of test_sq8_cpu.py::test_c_restatement_against_float64."""
    n = 500
    corpus = H.gauss(d, n, d)
    q = H.gauss(d + 1, 4, d)
    flat = Flat(corpus, "sq8")
    got = flat.sq8_scores(q)
    want = q.astype(np.float64) @ sq8.decode(flat.codes, flat.step).astype(np.float64).T
    assert got.shape == want.shape == (4, n)
    assert np.abs(got - want).max() <= 1e-5


@pytest.mark.parametrize("dtype, d", [("f32", 100), ("f16", 100), ("sq8", 100)])
def test_ivf_reference_alone_against_float64(dtype, d):
    """ivf_reference on one small shape against a float64 brute force over the same probed rows, under the project's
    bars - a reference that returned nonsense (or nothing) does not pass: the probed rows are recomputed here from
    float64 centroid scores, and every query must return min(k, rows) real rows."""
    n, nlist, k, nprobe = 600, 37, 30, 5
    corpus = H.gauss(1, n, d)
    cent = H.gauss(2, nlist, d)
    assign = uneven_assignment(n, nlist)
    q = H.gauss(3, NQ, d, normalize=False) * np.float32(2.5)
    assert np.bincount(assign, minlength=nlist)[[0, 20, 36]].tolist() == [0, 0, 1]
    for normalize in (False, True):
        D, I, rows_of = ivf_reference(corpus, cent, assign, q, k, nprobe, normalize, dtype)
        qn = seen_queries(q, normalize)
        Sc = qn.astype(np.float64) @ cent.astype(np.float64).T
        step = sq8.train_step(corpus)
        searched = sq8.decode(sq8.encode(corpus, step), step) if dtype == "sq8" else corpus
        for i in range(NQ):
            probed = np.argsort(-Sc[i], kind="stable")[:nprobe]
            rows = np.flatnonzero(np.isin(assign, probed))
            assert np.array_equal(rows, rows_of[i]) and 0 < rows.size < n
            assert (I[i] >= 0).sum() == min(k, rows.size)
            assert_bars(D[i:i + 1], I[i:i + 1], searched, rows, qn[i:i + 1], k, f16=dtype == "f16")
    # every list probed: the flat reference over all rows
    Da, Ia, _ = ivf_reference(corpus, cent, assign, q, k, nlist, True, dtype)
    Df, If = Flat(corpus, dtype).topk(np.arange(n), seen_queries(q, True), k)
    assert np.array_equal(Da, Df) and np.array_equal(Ia, If)


# ---- the restated launch rule against csrc/ls_scan_plan.h -------------------------------------------------------------------
ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "lean-explore_amd" / "csrc"
PLAN_ROWS = (1, 40, 63, 64, 65, 300, 301, 3001)
PLAN_BLOCKS = (1, 4, 256, 257)


def kprime(blocks, keff, kp_max):
    """k' of a scan launch (ls_kprime): lambda + 5 sqrt(lambda) + 3 of lambda = keff / blocks, at least 2, below
    kp_max, and at most 8192 (LS_FINAL_CAP) emitted keys in all."""
    lam = keff / blocks
    kp = min(max(int(lam + 5.0 * math.sqrt(lam) + 3.0), 2), kp_max - 1)
    while kp > 1 and blocks * kp > 8192:
        kp -= 1
    return kp


def test_restated_launch_rule_is_the_code_s_own(tmp_path):
    """csrc/ls_scan_plan.h in a plain host program with its own main (tests/scan_plan_check.cpp), built with
    AddressSanitizer and UndefinedBehaviorSanitizer: tile_rows, default_blocks and is_small above against the header's
    functions case for case, ls_scan_blocks' large-shard branch at the value its comment documents, and the clamped k'
    against kprime above. The coverage tests of this file rest on the restatement; this is what ties it to the code."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host check of ls_scan_plan.h"
    exe = tmp_path / "scan_plan_check"
    p = subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", str(CSRC), str(ROOT / "tests" / "scan_plan_check.cpp"),
                        "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    cases, want = [], []
    for L, V in GEOMS["sq8"]:
        for rl in (False, True):
            for rows in PLAN_ROWS:
                for blocks in PLAN_BLOCKS:
                    cases.append(f"S {L} {V} {int(rl)} {rows} {blocks}")
                    want.append(f"S {tile_rows(L, V, rl)} {default_blocks(rows, L, V)} "
                                f"{int(is_small(rows, blocks, L, V, rl))}")
    # 25 000 tiles; counts 512 ... 384 in steps of 8; the fullest last round is 13.95, at 448
    cases.append("B 200000 32 3 256")
    want.append("B 448")
    for blocks in (1, 8, 72, 241, 448, 512):
        for keff in (1, 10, 50, 1000, 2048):
            for kp_max in (16, 24):
                cases.append(f"K {blocks} {keff} {kp_max}")
                lam = keff / blocks
                want.append(f"K {kprime(blocks, keff, kp_max)} {int(lam + 5.0 * math.sqrt(lam) + 3.0)}")
    p = subprocess.run([str(exe)], input="\n".join(cases) + "\n", capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr.strip(), (p.stdout[-2000:], p.stderr[-2000:])
    got = p.stdout.split("\n")
    assert got[len(cases):] == [f"OK {len(cases)} cases", ""]
    for c, g, w in zip(cases, got, want):
        assert g == w, (c, g, w)
