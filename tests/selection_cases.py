"""Inputs for the tests of the selection step (csrc/ls_select_dev.h), chosen instead of met by accident.

Pure numpy, importable without a device. Four parts:

* ``ref_topk``: the definition every GPU result is compared with, bit for bit.
* the score-vector catalogue ``SCORES``: named generators ``(n, seed) -> float32[n]``, each aimed at one branch of
  ``lds_topk`` / ``general_select`` / ``finalize_body``.
* the merge-list catalogue: ``make_lists`` (layouts), ``ROW_MAPS`` and ``merge_cases`` - inputs of ``ls_merge_topk`` that
  stay inside its documented contract (include/leansearch.h).
* ``lds_topk_path``: a numpy restatement of ``lds_topk``'s path choice, so that tests/test_selection_cpu.py can show
  that the catalogue reaches every path. It proves nothing about the kernel.

The three injectors that feed these numbers to the kernels are in tests/test_selection_gpu.py (testing).
"""

from __future__ import annotations

import contextlib
import ctypes
import ctypes.util

import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)
NEG_FLT_MAX = np.float32(-3.4028234663852886e38)
LS_SS_MAX_KEYS = 4096   # csrc/ls_common.h
LS_SS_SAMPLE = 128      # csrc/ls_select_dev.h
LS_FINAL_CAP = 8192     # csrc/ls_scan_plan.h
LS_MAX_K = 2048         # include/leansearch.h


# ---------------------------------------------------------------------------------------------- denormals on the host
@contextlib.contextmanager
def ieee_denormals():
    """Default IEEE floating-point environment on the calling thread for the duration, the previous one put back after.
    A library built with -ffast-math (oracle/_build/liboracle_fast.so, once anything in the session has loaded it)
    switches the loading thread to flush-to-zero / denormals-are-zero: numpy then reads 1e-45 as 0 and the references
    computed here would no longer see the denormals the GPU sees. Both selection test modules run every test inside
    this context (an autouse fixture), so the catalogue and ref_topk do not depend on what ran before them."""
    # (glibc: FE_DFL_ENV is the pointer value -1 and fenv_t is 32 bytes on x86-64, 8 on aarch64 - the buffer is
    # generous. Where this does nothing, denormals_are_seen() says so: both modules' fixtures assert it.)
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fegetenv.argtypes = libm.fesetenv.argtypes = [ctypes.c_void_p]
    saved = ctypes.create_string_buffer(256)  # (fenv_t: 32 bytes on x86-64)
    libm.fegetenv(saved)
    libm.fesetenv(ctypes.c_void_p(-1))  # FE_DFL_ENV
    try:
        yield
    finally:
        libm.fesetenv(saved)


def denormals_are_seen() -> bool:
    one = np.array([1], np.uint32).view(np.float32)  # the smallest denormal, from its bit pattern
    return int((one + np.float32(0.0)).view(np.uint32)[0]) == 1 and float(one[0]) * 2.0 ** 149 == 1.0


# ---------------------------------------------------------------------------------------------- keys and the reference
def ord_u32(s: np.ndarray) -> np.ndarray:
    """ls_ord (csrc/ls_common.h): float32 -> uint32 whose unsigned order is the float order; -0.0 folds into +0.0."""
    with np.errstate(invalid="ignore"):
        u = (np.asarray(s, np.float32) + np.float32(0.0)).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unord_u32(k: np.ndarray) -> np.ndarray:
    """ls_unord: the inverse of ord_u32."""
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def valid_pairs(scores: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """A pair is a result iff row >= 0 and score > -FLT_MAX (NaN, -inf and -FLT_MAX never are: make_key's rule,
    oracle/flat_ip_ref.c)."""
    with np.errstate(invalid="ignore"):
        return (np.asarray(rows) >= 0) & (np.asarray(scores, np.float32) > NEG_FLT_MAX)


def make_keys(scores: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """ls_make_key as ls_merge_kernel applies it: uint64 (ord(score) << 32) | (2^32 - 1 - row); 0 = no result."""
    ok = valid_pairs(scores, rows)
    r = np.where(ok, rows, 0).astype(np.uint64)
    key = (ord_u32(scores).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - r)
    return np.where(ok, key, np.uint64(0))


def ref_topk(scores: np.ndarray, rows: np.ndarray, k: int) -> tuple[np.ndarray, np.ndarray]:
    """The k best valid pairs under (score descending, row ascending), compared in float64 with integer rows.
    Returns (float32[k], int64[k]); scores come back as score + 0.0f (the key folds -0.0 into +0.0); the tail is
    padded with (-FLT_MAX, -1)."""
    scores = np.asarray(scores, np.float32).reshape(-1)
    rows = np.asarray(rows, np.int64).reshape(-1)
    idx = np.flatnonzero(valid_pairs(scores, rows))
    order = idx[np.lexsort((rows[idx], -scores[idx].astype(np.float64)))][:k]
    D = np.full(k, NEG_FLT_MAX, np.float32)
    I = np.full(k, -1, np.int64)
    D[: order.size] = scores[order] + np.float32(0.0)
    I[: order.size] = rows[order]
    return D, I


def ref_topk_batch(S: np.ndarray, rows: np.ndarray, k: int) -> tuple[np.ndarray, np.ndarray]:
    out = [ref_topk(s, rows, k) for s in S]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def bits_equal(D, I, Dr, Ir) -> bool:
    """Scores on their bit patterns (so that -0.0 != +0.0 and NaN == NaN), rows exactly."""
    return (np.array_equal(np.ascontiguousarray(D, np.float32).view(np.uint32),
                           np.ascontiguousarray(Dr, np.float32).view(np.uint32))
            and np.array_equal(np.asarray(I, np.int64), np.asarray(Ir, np.int64)))


def first_difference(D, I, Dr, Ir) -> str:
    D, Dr = np.ascontiguousarray(D, np.float32), np.ascontiguousarray(Dr, np.float32)
    bad = np.argwhere((D.view(np.uint32) != Dr.view(np.uint32)) | (np.asarray(I) != np.asarray(Ir)))
    if not bad.size:
        return "equal"
    at = tuple(bad[0])
    return (f"{bad.shape[0]} of {D.size} slots differ, first at {at}: got (row {I[at]}, score {D[at]!r}) "
            f"want (row {Ir[at]}, score {Dr[at]!r})")


# ---------------------------------------------------------------------------------------------- score vectors
def _rng(seed: int, salt: int) -> np.random.Generator:
    return np.random.default_rng([salt, seed])


def gauss(n: int, seed: int) -> np.ndarray:
    return _rng(seed, 1).standard_normal(n, dtype=np.float32)


def gauss_f16(n: int, seed: int) -> np.ndarray:
    return gauss(n, seed).astype(np.float16).astype(np.float32)


def all_equal(n: int, seed: int) -> np.ndarray:
    return np.full(n, np.float32(0.75 + 0.25 * (seed % 3)), np.float32)


def two_values(n: int, seed: int, upper: int | None = None) -> np.ndarray:
    """`upper` rows (scattered) hold 1.5, the rest 0.25."""
    upper = n // 3 if upper is None else max(0, min(n, upper))
    s = np.full(n, np.float32(0.25), np.float32)
    s[_rng(seed, 2).permutation(n)[:upper]] = np.float32(1.5)
    return s


# where the k-th result falls: (name, size of the upper class as a function of k)
TWO_VALUES_AT = {"last_upper": lambda k: k, "first_lower": lambda k: k - 1, "inside_lower": lambda k: k // 2}


def two_values_for_k(n: int, seed: int, k: int, where: str) -> np.ndarray:
    return two_values(n, seed, TWO_VALUES_AT[where](min(k, n)))


def seven_values(n: int, seed: int) -> np.ndarray:
    vals = np.array([0.0, 1.25, 2.5, 3.75, 5.0, 6.5, 8.0], np.float32)
    return vals[_rng(seed, 3).integers(0, 7, n)]


def straddle(n: int, seed: int) -> np.ndarray:
    """About 1 % positives, 1 % zeros and denormals of both signs, FLT_MAX and +inf, the rest negative: the top k
    crosses zero for any k above n / 100, and the ordered keys differ in bit 31."""
    rng = _rng(seed, 4)
    s = -np.abs(rng.standard_normal(n, dtype=np.float32)) - np.float32(1e-3)
    perm = rng.permutation(n)
    npos = max(1, n // 100)
    s[perm[:npos]] = np.abs(rng.standard_normal(npos, dtype=np.float32)) + np.float32(1e-3)
    # +0, -0, +-1e-45, +0, -0, +-3e-45 (denormals), FLT_MAX, +inf - from their bit patterns
    special = np.array([0, 0x80000000, 1, 0x80000001, 0, 0x80000000, 2, 0x80000002, 0x7F7FFFFF, 0x7F800000],
                       np.uint32).view(np.float32)
    reps = max(1, n // 800)
    spots = perm[npos: npos + min(special.size * reps, max(0, n - npos - 1))]
    s[spots] = np.tile(special, reps)[: spots.size]
    return s


def ulps(n: int, seed: int) -> np.ndarray:
    chain = [np.float32(1.0)]
    for _ in range(15):
        chain.append(np.nextafter(chain[-1], np.float32(2.0)))
    return np.array(chain, np.float32)[_rng(seed, 5).integers(0, 16, n)]


def hb_bits(b: int):
    """Scores whose ordered keys share every bit above b and differ in bit b and below. Half of the rows draw
    from 48 patterns (tie classes, so that all score passes and the row half run), half are free."""
    def gen(n: int, seed: int) -> np.ndarray:
        rng = _rng(seed, 100 + b)
        base = np.uint32(0xBF800000) & ~np.uint32((1 << (b + 1)) - 1)  # ord(1.0) with the low b+1 bits cleared
        pool = rng.integers(0, 1 << (b + 1), 48, dtype=np.uint32)
        low = np.where(rng.random(n) < 0.5, pool[rng.integers(0, 48, n)], rng.integers(0, 1 << (b + 1), n, dtype=np.uint32))
        if n >= 2:  # bit b itself differs
            low[0] |= np.uint32(1 << b)
            low[n - 1] &= ~np.uint32(1 << b)
        return unord_u32(base | low.astype(np.uint32))
    gen.__name__ = f"hb_{b}"
    return gen


def ascending(n: int, seed: int) -> np.ndarray:
    return (np.arange(n, dtype=np.float64) * 2.0 ** -14 - 0.5 + (seed % 3)).astype(np.float32)


def descending(n: int, seed: int) -> np.ndarray:
    return ascending(n, seed)[::-1].copy()


_BAD = np.array([np.nan, -np.inf, NEG_FLT_MAX], np.float32)


def invalid(n: int, seed: int, valid: int | None = None) -> np.ndarray:
    """gauss with NaN, -inf and -FLT_MAX at row 0, at the last row, over one whole 64-row stretch and at 5 % of the
    rows at random; `valid` = m leaves exactly m valid rows instead."""
    rng = _rng(seed, 6)
    s = gauss(n, seed)
    if valid is None:
        bad = rng.random(n) < 0.05
        bad[0] = bad[n - 1] = True
        if n >= 192:
            j = 64 * ((n // 64) // 2)
            bad[j: j + 64] = True
    else:
        bad = np.ones(n, bool)
        bad[rng.permutation(n)[: max(0, min(n, valid))]] = False
    at = np.flatnonzero(bad)
    s[at] = _BAD[(at + seed) % 3]
    return s


# name -> (generator, the branch it aims at)
SCORES = {
    "gauss": (gauss, "control: distinct scores, the k-th never tied"),
    "all_equal": (all_equal, "hb = -1: no score pass, the row half decides everything"),
    "two_values": (two_values, "one score pass of one bit; the k-th inside or at the edge of a tie class"),
    "seven_values": (seven_values, "BM25-like: a few discrete non-negative scores, long first-digit buckets"),
    "straddle": (straddle, "hb == 31: pref and pmask take their special values; +-0, denormals, FLT_MAX, +inf"),
    "ulps": (ulps, "hb < 7: a single short digit"),
    **{f"hb_{b}": (hb_bits(b), f"hb == {b}: {(b + 8) // 8} score passes, last digit {b % 8 + 1} bits wide")
       for b in (7, 8, 15, 16, 23, 24)},
    "ascending": (ascending, "distinct, best rows last: every later row beats the running threshold"),
    "descending": (descending, "distinct, best rows first"),
    "invalid": (invalid, "NaN, -inf and -FLT_MAX among the candidates"),
}
F16_EXACT = ("gauss_f16", "seven_values", "all_equal", "two_values")  # exact in binary16, and so are a * s for a = +-2^-j
MERGE_SCORES = tuple(s for s in SCORES if s != "invalid")  # the merge contract excludes invalid scores on real rows


def score_vector(name: str, n: int, seed: int) -> np.ndarray:
    if name == "gauss_f16":
        return gauss_f16(n, seed)
    return SCORES[name][0](n, seed)


# ---------------------------------------------------------------------------------------------- merge lists
ROW_MAPS = {
    "identity": lambda r: r,
    "bit16": lambda r: r + (2 ** 16 - 3),         # tied rows differ up to bit 16 of the row half: three row passes
    "bit24": lambda r: r + (2 ** 24 - 3),         # ... bit 24: the fourth row pass
    "bit31": lambda r: r + (2 ** 31 - 3),         # ... bit 31: lhb == 31
    "top": None,                                  # the m highest legal rows, ending at 2^32 - 2
    "stride256": lambda r: r * 256,               # tied rows differ in one byte of the row half only
    "stride65536": lambda r: r * 65536,
}


def map_rows(name: str, m: int) -> np.ndarray:
    r = np.arange(m, dtype=np.int64)
    if name == "top":
        return r + (2 ** 32 - 1 - m)
    return ROW_MAPS[name](r)


LAYOUTS = ("interleaved", "blocked", "random", "ragged")


def make_lists(keys_scores: np.ndarray, keys_rows: np.ndarray, n_lists: int, k: int, layout: str, seed: int = 0
               ) -> tuple[np.ndarray, np.ndarray]:
    """Deal a pool of (score, row) pairs (at most n_lists * k, rows distinct) to n_lists sorted lists of k slots:
    (float32 [n_lists, k], int64 [n_lists, k]) inside ls_merge_topk's contract - every list sorted by the total
    order, -1 padding at list tails only (score -FLT_MAX there), scores of real rows valid and with -0.0 folded into
    +0.0 (merge inputs are search results, which never carry -0.0), rows distinct across lists.
      interleaved: rank i goes to list i mod n_lists;  blocked: list l holds ranks [l k, (l + 1) k);
      random: every rank to a random list with room;   ragged: lists of different real lengths, some empty."""
    s = np.asarray(keys_scores, np.float32) + np.float32(0.0)
    r = np.asarray(keys_rows, np.int64)
    assert s.shape == r.shape and s.size <= n_lists * k
    assert valid_pairs(s, r).all() and np.unique(r).size == r.size and r.max(initial=0) < 2 ** 32 - 1
    order = np.lexsort((r, -s.astype(np.float64)))
    s, r = s[order], r[order]
    m = s.size
    rng = _rng(seed, 7)
    if layout == "interleaved":
        owner = np.arange(m) % n_lists
    elif layout == "blocked":
        owner = np.arange(m) // k
    elif layout == "random":
        owner = rng.permutation(np.repeat(np.arange(n_lists), k))[:m]
    elif layout == "ragged":
        lens = rng.integers(0, k + 1, n_lists)
        lens[rng.random(n_lists) < 0.25] = 0
        if n_lists > 1:
            lens[rng.integers(0, n_lists)] = k  # one full list, so that the shape's k is reachable
        else:
            lens[0] = k
        slots = rng.permutation(np.repeat(np.arange(n_lists), lens))
        m = min(m, slots.size)
        pick = np.sort(rng.permutation(s.size)[:m])  # a subset of the pool, still in rank order
        s, r, owner = s[pick], r[pick], slots[:m]
    else:
        raise ValueError(layout)
    S = np.full((n_lists, k), NEG_FLT_MAX, np.float32)
    R = np.full((n_lists, k), -1, np.int64)
    for l in range(n_lists):
        mine = np.flatnonzero(owner == l)  # ascending rank: sorted by the total order
        S[l, : mine.size] = s[mine]
        R[l, : mine.size] = r[mine]
    return S, R


# (n_lists, k) of the issue, by the main path their full lists take at 256 threads
SHAPES_COUNT = ((2, 3), (4, 16), (3, 64), (2, 128), (256, 1))
SHAPES_SPLITTER = ((2, 129), (3, 1000), (2, 2048), (16, 256), (64, 64), (4096, 1))
SHAPES_RADIX = ((8, 1000), (3, 2048), (4, 2048), (32, 256), (8192, 1))
SHAPES = SHAPES_COUNT + SHAPES_SPLITTER + SHAPES_RADIX
NQ = 3  # queries per launch, all different


def _case(n_lists, k, scores, layout, rowmap, seed):
    return {"id": f"{n_lists}x{k}-{scores}-{layout}-{rowmap}", "n_lists": n_lists, "k": k, "scores": scores,
            "layout": layout, "rowmap": rowmap, "seed": seed}


def merge_cases() -> list[dict]:
    """The thinned cross product: every shape with four (scores, layout, row map) triples that between them use every
    layout; the long shapes, where the radix code and its row half run, with every score vector and row map; and the
    tie cases aimed at single branches."""
    cases = []
    base = (("gauss", "interleaved", "identity"), ("all_equal", "random", "bit24"),
            ("two_values", "ragged", "bit31"), ("seven_values", "blocked", "stride256"))
    for n_lists, k in SHAPES:
        for sc, lay, rm in base:
            cases.append(_case(n_lists, k, sc, lay, rm, 11))
    maps = tuple(ROW_MAPS)
    for si, (n_lists, k) in enumerate(((8, 1000), (4, 2048), (16, 256), (32, 256), (3, 1000), (8192, 1))):
        for ci, sc in enumerate(MERGE_SCORES):
            cases.append(_case(n_lists, k, sc, LAYOUTS[(ci + si) % 2 * 2], maps[(ci + si) % len(maps)], 23))
    # ties: every row map under all-equal and two-valued scores where the row half decides
    for rm in maps:
        cases.append(_case(8, 1000, "all_equal", "interleaved", rm, 31))
        cases.append(_case(32, 256, "two_values", "random", rm, 31))
        cases.append(_case(4, 2048, "hb_24", "interleaved", rm, 31))
    seen, out = set(), []
    for c in cases:
        if c["id"] not in seen:
            seen.add(c["id"])
            out.append(c)
    return out


def build_merge_case(case: dict) -> tuple[np.ndarray, np.ndarray]:
    """(float32 [n_lists, NQ, k], int64 [n_lists, NQ, k]): NQ different queries (seeds) of one case."""
    n_lists, k = case["n_lists"], case["k"]
    m = n_lists * k
    S = np.empty((n_lists, NQ, k), np.float32)
    R = np.empty((n_lists, NQ, k), np.int64)
    for qi in range(NQ):
        seed = case["seed"] + qi
        if case["scores"] == "two_values":  # the k-th at the end of the upper class, at the start of and inside the lower
            s = two_values_for_k(m, seed, k, tuple(TWO_VALUES_AT)[qi % 3])
        else:
            s = score_vector(case["scores"], m, seed)
        rows = map_rows(case["rowmap"], m)[_rng(seed, 8).permutation(m)]
        S[:, qi], R[:, qi] = make_lists(s, rows, n_lists, k, case["layout"], seed)
    return S, R


# ---------------------------------------------------------------------------------------------- lds_topk's path choice
def _radix_passes(vals: np.ndarray, hb: int, krem: int):
    """The 8-bit passes of lds_topk from bit hb down over uint32 `vals` (all of which share the bits above hb):
    (passes run, krem left, population of the last selected bin, first pass's per-bin survivor counts)."""
    npass = (hb + 8) // 8
    run, neq, first = 0, vals.size, None
    for p in range(npass):
        top = hb - 8 * p
        shift = top - 7 if top >= 7 else 0
        dmask = 255 if top >= 7 else (2 << top) - 1
        dig = (vals >> np.uint32(shift)) & np.uint32(dmask)
        hist = np.bincount(dig, minlength=256)
        above = np.cumsum(hist[::-1])[::-1] - hist          # keys in higher bins
        b = int(np.flatnonzero((above < krem) & (krem <= above + hist))[0])
        if p == 0:
            first = np.where(np.arange(256) > b, hist, 0)
            first[b] = krem - above[b]
        krem -= int(above[b])
        neq = int(hist[b])
        vals = vals[dig == b]
        run += 1
        if neq == krem:
            break
    return run, krem, neq, first


def lds_topk_path(keys: np.ndarray, k: int, nt: int) -> dict:
    """Which way lds_topk (csrc/ls_select_dev.h) takes for `keys` (uint64, in list order, 0 = no result):
      main: "count" (l. 346-368; "G" = threads per key), "splitter" (l. 369-495), "splitter_fallthrough" (l. 442, 496)
            or "radix" (l. 498-747; cnt > LS_SS_MAX_KEYS, or a workgroup size the splitter code does not serve);
      for the radix code (fall-through included): "hb" (l. 534), "score_passes" run (l. 543-564), "short_top_digit"
      (0 <= hb < 7), "row_passes" run (0 = the row half did not run; l. 568-628), "lhb" (l. 600), "order": "count"
      (kk <= 256, l. 697), "bucketed" (l. 643-674, 713) or "network" (l. 738)."""
    keys = np.asarray(keys, np.uint64)
    cnt = keys.size
    k = min(k, cnt)
    out = {"cnt": cnt, "k": k}
    if k <= 0:
        return {**out, "main": "empty"}
    if cnt <= 256 and cnt <= nt:
        return {**out, "main": "count", "G": 4 if cnt * 4 <= nt else 1}
    nz = keys[keys != 0]
    main = "radix"
    if cnt <= LS_SS_MAX_KEYS and nt in (256, 512, 1024):
        t = np.arange(LS_SS_SAMPLE)
        sample = keys[(t * cnt) // LS_SS_SAMPLE]
        sample = np.where(sample != 0, sample, (t + 1).astype(np.uint64))
        ssort = np.sort(sample)[::-1]
        split = ssort[1::2][:63]                                   # splitter j = ssort[2 j + 1], j = 0 .. 62
        bucket = (split[None, :] > nz[:, None]).sum(axis=1) if nz.size else np.zeros(0, int)
        bcnt = np.bincount(bucket, minlength=64)
        start = np.cumsum(bcnt) - bcnt
        kq = min(k, int(nz.size))
        if kq == 0:
            return {**out, "main": "empty"}
        big = int(bcnt[start < kq].max())
        if big <= 256:
            return {**out, "main": "splitter", "longest_bucket": big}
        main = "splitter_fallthrough"
        out["longest_bucket"] = big
    kk = min(k, int(nz.size))
    if kk == 0:
        return {**out, "main": "empty"}
    hi = (nz >> np.uint64(32)).astype(np.uint32)
    lo = (nz & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    diff = int(hi.max() ^ hi.min())
    hb = diff.bit_length() - 1
    run, krem, neq, first = (0, kk, int(nz.size), None) if hb < 0 else _radix_passes(hi, hb, kk)
    out.update(main=main, hb=hb, score_passes=run, short_top_digit=0 <= hb < 7, row_passes=0, lhb=None)
    if neq > krem:
        # the k-th score: the pattern the passes selected, i.e. the krem-th largest of the tie class' score
        kth = np.sort(hi)[::-1][kk - 1]
        tl = lo[hi == kth]
        ldiff = int(tl.max() ^ tl.min())
        lhb = ldiff.bit_length() - 1
        out["lhb"] = lhb
        out["row_passes"] = _radix_passes(tl, lhb, krem)[0]
    if kk <= 256:
        out["order"] = "count"
    elif hb >= 0 and int(first.max()) <= 192:
        out["order"] = "bucketed"
    else:
        out["order"] = "network"
    return out
