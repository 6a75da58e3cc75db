"""What tests/test_mq_subset_cpu.py and tests/test_mq_subset_gpu.py share: the GPU test's shape, and a restatement in
Python of how csrc/ls_mq_plan.h plans a subset pass (workgroups, k', keys per lane) - the CPU test holds the
restatement to the header (tests/mq_plan_check.cpp) and uses it to show that the GPU test's k sweep reaches every
key-list size."""

import math

import numpy as np

N = 12_001          # n % 16 == 1: the all-ones subset has a ragged last tile
N_CU = 256          # compute units of an MI355X
MAX_BLOCKS = 4 * N_CU
MIN_ROWS = 4096     # LS_MQ_MIN_ROWS
K_SWEEP = (10, 50, 150, 1000)   # keys per lane on the half subset: 3, 5, 8, declined


def half_rows(n: int = N, seed: int = 77) -> np.ndarray:
    """A random half of the rows, ascending (m ~ 6000)."""
    return np.nonzero(np.random.default_rng(seed).random(n) < 0.5)[0]


TIES_N = 50_000     # the integer corpus with duplicated rows: k = 500 needs ~1000 waves to be served by a pass


def ties_rows(n: int = TIES_N) -> np.ndarray:
    """Four rows of every five (m = 40 000)."""
    r = np.arange(n)
    return r[r % 5 != 4]


def mq_blocks(m: int, n_cu: int = N_CU, wpb: int = 4) -> int:
    nt = (m + 15) // 16
    b = (nt + wpb * 2 - 1) // (wpb * 2)
    if b <= n_cu:
        return max(b, 1)
    best, best_fill = n_cu, -1.0
    c = n_cu
    while c >= n_cu * 92 // 100:
        rounds = nt / (c * wpb)
        fill = rounds - int(rounds)
        if fill == 0.0:
            fill = 1.0
        if fill > best_fill + 0.02:
            best_fill, best = fill, c
        c -= 1
    return best


def lane_keys(blocks: int, keff: int, wpb: int = 4) -> int:
    """ls_mq_plan_lane_keys: the smallest of 3, 5, 8 keys for which a wave holding more of a query's top-k (a Poisson(k /
    waves) number) is rarer than 2e-3 per query over the launch's waves; 0: declined."""
    waves = float(wpb * blocks)
    mu = keff / waves
    for m in (3, 5, 8):
        term = math.exp(-mu)
        tail = 1.0 - term
        for j in range(1, m + 1):
            term *= mu / j
            tail -= term
        tail = max(tail, 0.0)
        if tail * waves < 2e-3:
            return m
    return 0


def kprime_of(blocks: int, keff: int, kp_max: int = 24) -> int:
    lam = keff / blocks
    kp = min(max(int(lam + 5.0 * math.sqrt(lam) + 3.0), 2), kp_max - 1)
    while kp > 1 and blocks * kp > 8192:
        kp -= 1
    return kp


def plan(m: int, k: int, n_cu: int = N_CU, wpb: int = 4, forced_blocks: int = 0):
    """(blocks, kprime, keys) of ls_mq_make_plan (LS_MQ_ROWLIST) with the option on (forced_blocks: debug option 7); (0, 0, 0):
    declined"""
    if m < MIN_ROWS:
        return (0, 0, 0)
    max_blocks = 4 * n_cu
    keff = max(min(k, m), 1)
    blocks = min(forced_blocks if forced_blocks > 0 else mq_blocks(m, n_cu, wpb), max_blocks)
    keys = lane_keys(blocks, keff, wpb)
    if keys == 0 and forced_blocks <= 0:  # one workgroup per CU, down to one tile per wave, before the plan declines
        wide = min(n_cu, max_blocks, ((m + 15) // 16 + wpb - 1) // wpb)
        if wide > blocks:
            blocks = wide
            keys = lane_keys(blocks, keff, wpb)
    kp = kprime_of(blocks, keff)
    while 0 < keys < 8 and kp + 1 > wpb * keys:
        keys = 5 if keys == 3 else 8
    if keys > 0:
        kp = min(kp, wpb * keys - 1)
    kp = min(kp, max_blocks * 16 // blocks)
    if keys == 0 or kp < 1:
        return (0, 0, 0)
    return (blocks, kp, keys)


def groups(nq: int) -> int:
    """passes a call of nq queries takes: groups of min(left, 16) while two or more are left"""
    g, left = 0, nq
    while left >= 2:
        left -= min(left, 16)
        g += 1
    return g
