"""The selection catalogue (tests/selection_cases.py) before any GPU sees it: its reference agrees with the CPU
oracle on every case, and - by the numpy restatement of lds_topk's path choice - its merge cases reach every path of
lds_topk at 256 threads. A path that no case reaches fails by name."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from oracle import oracle
from tests import selection_cases as C


@pytest.fixture(autouse=True)
def _ieee_denormals():
    with C.ieee_denormals():
        assert C.denormals_are_seen()
        yield


N_DENSE = 4096
D_DENSE = 64
KS_DENSE = (1, 50, 257, 2048)
QUERY_SCALES = (1.0, -1.0, 0.5)


@functools.lru_cache(maxsize=None)
def merge_inputs(case_id: str):
    case = next(c for c in C.merge_cases() if c["id"] == case_id)
    return C.build_merge_case(case)


MERGE_IDS = [c["id"] for c in C.merge_cases()]


@pytest.mark.parametrize("case_id", MERGE_IDS)
def test_ref_topk_equals_oracle_merge(case_id):
    S, R = merge_inputs(case_id)
    n_lists, nq, k = S.shape
    # in contract: sorted lists, padding at the tails only, rows distinct, scores valid
    for qi in range(nq):
        real = R[:, qi] >= 0
        assert (np.diff(real.astype(np.int8), axis=1) <= 0).all(), "padding inside a list"
        keys = C.make_keys(S[:, qi], R[:, qi])
        for l in range(n_lists):
            kl = keys[l][real[l]]
            assert (kl[:-1] > kl[1:]).all(), "a list is not sorted by the total order"
        rows = R[:, qi][real]
        assert np.unique(rows).size == rows.size and rows.max(initial=0) < 2 ** 32 - 1
        assert C.valid_pairs(S[:, qi][real], rows).all()
        assert not np.signbit(S[:, qi][real][S[:, qi][real] == 0]).any()
    Do, Io = oracle.c_merge(S, R)
    Dr, Ir = _ref_merge(S, R)
    assert C.bits_equal(Dr, Ir, Do, Io), C.first_difference(Dr, Ir, Do, Io)


def _ref_merge(S, R):
    n_lists, nq, k = S.shape
    out = [C.ref_topk(S[:, qi].reshape(-1), R[:, qi].reshape(-1), k) for qi in range(nq)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@functools.lru_cache(maxsize=None)
def dense_vectors(n):
    """Every score vector of the catalogue at n rows, with the k-dependent variants the GPU tests use."""
    out = {name: C.score_vector(name, n, 5) for name in C.SCORES}
    out["gauss_f16"] = C.score_vector("gauss_f16", n, 5)
    for k in (50, 2048):
        for where in C.TWO_VALUES_AT:
            out[f"two_values-{where}-k{k}"] = C.two_values_for_k(n, 5, k, where)
        for m in (0, k - 1, k, k + 1):
            out[f"invalid-{m}valid-k{k}"] = C.invalid(n, 5, valid=m)
    return out


@pytest.mark.parametrize("name", sorted(dense_vectors(8)))
def test_ref_topk_equals_oracle_search_of_one_hot_corpus(name):
    s = dense_vectors(N_DENSE)[name]
    corpus = np.zeros((N_DENSE, D_DENSE), np.float32)
    corpus[:, 0] = s
    q = np.zeros((len(QUERY_SCALES), D_DENSE), np.float32)
    q[:, 0] = QUERY_SCALES
    with np.errstate(invalid="ignore", over="ignore"):
        scores = q[:, :1] * s[None, :]  # float32: the only product of a row that is not 0 * 0
    rows = np.arange(N_DENSE)
    kmax = max(KS_DENSE)  # one search per order: the top k of a smaller k is a prefix, padding included
    Dr, Ir = C.ref_topk_batch(scores, rows, kmax)
    for order in ("strict", "scan", "fma"):
        Do, Io = oracle.c_search(corpus, q, kmax, order=order)
        for k in KS_DENSE:
            assert C.bits_equal(Dr[:, :k], Ir[:, :k], Do[:, :k], Io[:, :k]), \
                (k, order, C.first_difference(Dr[:, :k], Ir[:, :k], Do[:, :k], Io[:, :k]))


def test_denormals_are_seen_and_in_the_catalogue():
    """Whatever ran earlier in the session (the -ffast-math oracle build sets flush-to-zero on the thread that loads
    it; this test loads it if nothing has), the tests of this module see denormals - the autouse fixture - and
    `straddle` carries them in both signs."""
    oracle.c_search(np.ones((4, 4), np.float32), np.ones((1, 4), np.float32), 1, fast=True)
    with C.ieee_denormals():  # (a first load just now has switched this thread to flush-to-zero)
        assert C.denormals_are_seen()
        bits = C.straddle(N_DENSE, 5).view(np.uint32)
        for pattern in (0x00000001, 0x80000001, 0x00000002, 0x80000002, 0x80000000, 0x7F800000, 0x7F7FFFFF):
            assert (bits == pattern).any(), hex(pattern)
        D, I = C.ref_topk(np.array([1, 2, 0], np.uint32).view(np.float32), np.arange(3), 3)
        assert I.tolist() == [1, 0, 2] and D.view(np.uint32).tolist() == [2, 1, 0]


def test_ref_topk_definition():
    s = np.array([1.0, np.nan, -np.inf, C.NEG_FLT_MAX, -0.0, 0.0, np.inf, 1.0, 5.0], np.float32)
    r = np.array([7, 1, 2, 3, 4, 5, 6, 0, -1], np.int64)
    D, I = C.ref_topk(s, r, 7)
    assert I.tolist() == [6, 0, 7, 4, 5, -1, -1]
    assert D.view(np.uint32).tolist() == np.array([np.inf, 1, 1, 0.0, 0.0, C.NEG_FLT_MAX, C.NEG_FLT_MAX],
                                                   np.float32).view(np.uint32).tolist()
    x = np.array([0.0, -0.0, 1e-45, -1e-45, 1.5, -1.5, np.inf, C.FLT_MAX, C.NEG_FLT_MAX], np.float32)
    o = C.ord_u32(x)
    assert np.array_equal(C.unord_u32(o).view(np.uint32), (x + np.float32(0)).view(np.uint32))
    assert o[0] == o[1] and o[3] < o[0] < o[2] < o[4] < o[7] < o[6] and o[8] < o[5] < o[3]


@functools.lru_cache(maxsize=None)
def merge_paths(nt=256):
    """{case id: [lds_topk_path of each query]} at `nt` threads, the keys in ls_merge_kernel's order (list-major)."""
    out = {}
    for cid in MERGE_IDS:
        S, R = merge_inputs(cid)
        n_lists, nq, k = S.shape
        out[cid] = [C.lds_topk_path(C.make_keys(S[:, qi].reshape(-1), R[:, qi].reshape(-1)), k, nt) for qi in range(nq)]
    return out


WANTED = {
    "count, 4 threads per key": lambda p: p["main"] == "count" and p["G"] == 4,
    "count, 1 thread per key": lambda p: p["main"] == "count" and p["G"] == 1,
    "splitter": lambda p: p["main"] == "splitter",
    "splitter_fallthrough": lambda p: p["main"] == "splitter_fallthrough",
    "radix with cnt > 4096": lambda p: p["main"] == "radix" and p["cnt"] > 4096,
    **{f"{n} score passes": (lambda n: lambda p: p.get("score_passes") == n)(n) for n in range(5)},
    "a short top digit": lambda p: p.get("short_top_digit") is True,
    "hb == 31": lambda p: p.get("hb") == 31,
    **{f"{n} row-half passes": (lambda n: lambda p: p.get("row_passes") == n)(n) for n in range(1, 5)},
    "lhb == 31": lambda p: p.get("lhb") == 31,
    **{f"survivors ordered by {o}": (lambda o: lambda p: p.get("order") == o)(o)
       for o in ("count", "bucketed", "network")},
}


@pytest.mark.parametrize("path", sorted(WANTED))
def test_merge_catalogue_reaches(path):
    hits = [cid for cid, ps in merge_paths().items() if any(WANTED[path](p) for p in ps)]
    assert hits, f"no merge case of the catalogue reaches: {path}"


def test_shapes_take_the_main_path_they_are_listed_under():
    """Full lists of distinct Gaussian scores, blocked (no resonance with the sample stride)."""
    for shapes, want in ((C.SHAPES_COUNT, "count"), (C.SHAPES_SPLITTER, "splitter"), (C.SHAPES_RADIX, "radix")):
        for n_lists, k in shapes:
            m = n_lists * k
            S, R = C.make_lists(C.gauss(m, 3), np.arange(m), n_lists, k, "blocked")
            p = C.lds_topk_path(C.make_keys(S.reshape(-1), R.reshape(-1)), k, 256)
            assert p["main"] == want, (n_lists, k, p)


def test_interleaved_16x256_gaussian_falls_through():
    """Row-interleaved shards: the sample positions land in clumps of n_lists neighbouring ranks, one splitter bucket
    holds several hundred keys, and the splitter code hands over to the radix code."""
    for seed in range(3):
        m = 16 * 256
        S, R = C.make_lists(C.gauss(m, seed), np.arange(m), 16, 256, "interleaved")
        p = C.lds_topk_path(C.make_keys(S.reshape(-1), R.reshape(-1)), 256, 256)
        assert p["main"] == "splitter_fallthrough" and p["longest_bucket"] > 256, p
        b = C.lds_topk_path(C.make_keys(*[a.reshape(-1) for a in C.make_lists(C.gauss(m, seed), np.arange(m), 16, 256,
                                                                                 "blocked")]), 256, 256)
        assert b["main"] == "splitter", b


def test_restatement_agrees_with_a_sort():
    """The passes the restatement walks end at the k-th key: its bookkeeping is checked against np.sort."""
    rng = np.random.default_rng(9)
    for hb in (3, 7, 12, 24, 31):
        vals = rng.integers(0, 2 ** (hb + 1), 3000, dtype=np.uint64).astype(np.uint32)
        vals[0] |= np.uint32(1 << hb)
        vals[1] &= ~np.uint32(1 << hb)
        for k in (1, 100, 2999, 3000):
            run, krem, neq, first = C._radix_passes(vals, hb, k)
            kth = np.sort(vals)[::-1][k - 1]
            assert 1 <= run <= (hb + 8) // 8 and 1 <= krem <= neq
            assert int(first.sum()) == k
            if run == (hb + 8) // 8:  # every digit resolved: the bin is one value
                assert neq == int((vals == kth).sum()) and krem == k - int((vals > kth).sum())
