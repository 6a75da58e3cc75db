"""The mutation scripts and their host model without a GPU (tests/mutation_scripts.py):
  - the conditions the script set must meet - they are what makes tests/test_mutation_scripts_gpu.py worth running, so
    an edit that hollows a script out fails here;
  - the model against a naive restatement (a Python list of (token, row, list) tuples and list comprehensions), and its
    expected search results on the tied script against a float64 brute force ordered by (score, current row);
  - the host-buffered half of IVFFlatIndex (add / remove_ids before the device object exists) over sequences of ops;
  - csrc/ls_ivf_add_plan.h and csrc/ls_ivf_remove_plan.h chained over random histories under sanitizers
    (tests/mutation_chain_check.cpp)."""

import functools
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from lean_explore_amd import sq8
from lean_explore_amd.ivf import IVFFlatIndex
from tests import mutation_scripts as M

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "lean-explore_amd" / "csrc"
FLOOR = M.FLOOR
TIES_K = (10, 100)  # the k of the tied script's condition (k = 1 is searched too: the best score may be one row's alone)


@functools.lru_cache(maxsize=None)
def trace(name, ivf=True):
    d = 100
    return M.trace(M.SCRIPTS[name], d, M.centroids(d) if ivf else None)


def mutations(tr):
    """[(index, "add" | "remove", live subset keys)] of the ops that changed a built handle's rows."""
    return [(i, s["op"][0], tuple(sorted(s["subsets"]))) for i, s in enumerate(tr)
            if s["built"] and s["op"][0] in ("add", "remove") and s["moved"] > 0]


# ---- 1. the conditions ----------------------------------------------------------------------------------------------------
def test_required_scripts_exist_and_random_ones_have_twelve_ops():
    for name in ("update_cycles", "empty_and_refill", "across_the_floor", "late_build", "late_build_default_lists", "ties",
                 "edges", "louder_adds", "random_206", "random_213", "random_215"):
        assert name in M.SCRIPTS, name
    for name, s in M.SCRIPTS.items():
        assert s.ops.count(("build",)) == 1 and s.ops[0][0] == "add", name
        if name.startswith("random_"):
            assert len(s.ops) == 2 + 12 and s == M.random_script(s.seed), name  # (seeded: the same script every time)
    assert M.SCRIPTS["late_build"].ops == M.SCRIPTS["late_build_default_lists"].ops
    assert M.SCRIPTS["late_build"].named and not M.SCRIPTS["late_build_default_lists"].named
    assert M.SCRIPTS["late_build"].ivf_only and M.SCRIPTS["ties"].data == "int"


def test_every_op_kind_removal_kind_and_add_size_occurs():
    ops = [op for s in M.SCRIPTS.values() for op in s.ops]
    assert {op[0] for op in ops} == set(M.OP_KINDS)
    assert {op[1] for op in ops if op[0] == "remove"} == set(M.REMOVE_KINDS)
    assert {op[2] for op in ops if op[0] == "add"} == set(M.ADD_HOWS)
    sizes = {op[1] for op in ops if op[0] == "add"}
    assert {0, 1, 63} <= sizes and any(s is not None and 200 <= s <= 900 for s in sizes)
    # ... and does what it says: every removal kind takes rows from a built handle at least once, but the two that
    # by definition take none
    took = {s["op"][1] for name in M.SCRIPTS for s in trace(name) if s["op"][0] == "remove" and s["built"] and s["moved"] > 0}
    none = {s["op"][1] for name in M.SCRIPTS for s in trace(name) if s["op"][0] == "remove" and s["built"] and s["moved"] == 0}
    assert took == set(M.REMOVE_KINDS) - {"nothing", "out_of_range"} and {"nothing", "out_of_range"} <= none
    dup = [s for name in M.SCRIPTS for s in trace(name) if s["op"] == ("remove", "duplicated", None)]
    assert dup and all(s["moved"] == 3 for s in dup)


def test_update_cycles_has_six_rounds_and_two_subsets_of_different_age():
    tr = trace("update_cycles")
    muts = mutations(tr)  # (the initial add precedes the build: not among them)
    assert [m[1] for m in muts] == ["remove", "add"] * 6
    made = [i for i, s in enumerate(tr) if s["op"][0] == "subset_new"]
    assert len(made) == 2
    assert made[0] < muts[0][0], "one subset is made before round 1"
    assert muts[5][0] < made[1] < muts[6][0], "one subset is made between rounds 3 and 4"
    assert all(len(m[2]) == 1 for m in muts[:6]) and all(len(m[2]) == 2 for m in muts[6:])
    assert all(s["subsets"][k] > 0 for s in tr[made[1]:] for k in (0, 1)), "both are searched after every later round"


def test_a_subset_lives_through_remove_add_remove():
    found = False
    for name in M.SCRIPTS:
        muts = mutations(trace(name))
        for key in {k for m in muts for k in m[2]}:
            kinds = [m[1] for m in muts if key in m[2]]
            for a in range(len(kinds)):
                if kinds[a] == "remove" and "add" in kinds[a + 1:]:
                    b = a + 1 + kinds[a + 1:].index("add")
                    found |= "remove" in kinds[b + 1:] and len(kinds) >= 3
    assert found


def test_two_subsets_of_different_age_are_live_during_a_removal():
    hits = [name for name in M.SCRIPTS for m in mutations(trace(name)) if m[1] == "remove" and len(m[2]) >= 2]
    assert "update_cycles" in hits and "across_the_floor" in hits


def test_empty_and_refill_empties_a_list_under_a_subset_and_refills_it():
    tr = trace("empty_and_refill")
    p = M.Player(M.SCRIPTS["empty_and_refill"], 100, M.centroids(100))
    seen = []
    for st in p.steps():
        seen.append((st, p.model.list_sizes(), {k: p.model.list_sizes(k) for k in p.model.subsets}))
    emptied = next(i for i, (st, _, _) in enumerate(seen) if st.op[:2] == ("remove", "list"))
    l = int(np.flatnonzero((seen[emptied - 1][1] > 0) & (seen[emptied][1] == 0))[0])
    assert seen[emptied - 1][2][0][l] > 0 and seen[emptied][2][0][l] == 0, "subset 0 held rows of the list"
    refill = emptied + 1
    assert seen[refill][0].op[0] == "add" and seen[refill][1][l] == seen[emptied - 1][1][l] > 0, "refilled by an add"
    assert seen[refill][2][0][l] == 0, "rows added later never join a subset"
    assert seen[refill + 1][0].op[0] == "subset_new" and seen[refill + 1][2][1][l] > 0, "subset 1 covers the refilled list"
    ns = [s["n"] for s in tr[refill + 2:]]
    kinds = [s["op"][0] for s in tr[refill + 2:]]
    assert kinds == ["remove", "add", "remove"] and ns[0] == 0 and ns[1] > ns[2] > 0, "ntotal -> 0 -> add -> remove"
    assert all(tr[i]["built"] for i in range(emptied, len(tr)))


def test_a_list_and_the_whole_index_go_to_zero_and_recover():
    for ivf in (True, False):
        tr = trace("empty_and_refill", ivf)
        built = [s for s in tr if s["built"]]
        ns = [s["n"] for s in built]
        z = ns.index(0)
        assert z > 0 and max(ns[z + 1:]) > 0
        sizes = np.stack([s["sizes"] for s in built])
        assert any((sizes[a, l] > 0 and sizes[b, l] == 0 and sizes[c, l] > 0)
                   for l in range(M.NLIST) for a in range(len(built)) for b in range(a + 1, len(built))
                   for c in range(b + 1, len(built)))


@pytest.mark.parametrize("ivf", [True, False])
def test_across_the_floor_crosses_4096_both_ways_with_the_option_on(ivf):
    tr = [s for s in trace("across_the_floor", ivf) if s["built"]]
    assert all(s["small_batch"] for s in tr)
    ns = [s["n"] for s in tr if s["op"][0] in ("add", "remove", "build")]
    assert ns[0] >= FLOOR + 1500 and ns[1] <= FLOOR - 800 and ns[2] >= FLOOR + 2500 and FLOOR + 500 <= ns[3] <= FLOOR + 1500, ns
    # A subset never grows, so "both ways" is two subsets on one handle: subset 0 is served above the floor, falls
    # below it, and subset 1 - made of the regrown index - is served above it again, then falls below it too.
    rows = [(s["subsets"].get(0), s["subsets"].get(1)) for s in tr if s["subsets"]]
    assert rows[0][0] >= FLOOR and rows[1][0] < FLOOR, rows
    made = next(i for i, r in enumerate(rows) if r[1] is not None)
    assert made > 1 and rows[made][1] >= FLOOR and rows[made][0] < FLOOR and 0 < rows[-1][1] < FLOOR, rows


def test_late_build_mutates_the_buffers_four_times_and_the_handle_three_times():
    for name in ("late_build", "late_build_default_lists"):
        tr = trace(name)
        b = next(i for i, s in enumerate(tr) if s["op"] == ("build",))
        assert [s["op"][0] for s in tr[:b]] == ["add", "remove", "add", "remove"] and all(s["moved"] > 0 for s in tr[:b])
        assert [m[1] for m in mutations(tr)] == ["add", "remove", "add"]
        assert 4500 <= tr[b]["n"] <= 9000


def test_sizes_stay_between_4500_and_9000_rows_at_the_build_and_the_sq8_step_survives():
    for name, s in M.SCRIPTS.items():
        for d in (20, 384):
            p = M.Player(s, d)
            step = None
            for st in p.steps():
                assert p.model.n <= 9000, name
                if st.op == ("build",):
                    assert 4500 <= p.model.n <= 9000, name
                    step = sq8.train_step(p.model.rows)
            if name == "louder_adds":
                # the opposite: from the first loud add on, a step trained on the live rows is not the build's, so a
                # handle that retrained during a mutation stores other codes than the model's (and the GPU test
                # compares no fresh IVF sq8 handle on this script: it would train that other step)
                loud = [i for i, op in enumerate(s.ops) if op[0] == "add" and op[2] == "loud"]
                assert len(loud) == 3 and s.ops.index(("build",)) < loud[0]
                q = M.Player(s, d)
                for st in q.steps():
                    if st.index >= loud[0]:
                        other = sq8.train_step(q.model.rows)
                        assert (other > step * np.float32(1.5)).all(), (name, st.index)
                        assert (sq8.encode(q.model.rows, other) != sq8.encode(q.model.rows, step)).mean() > 0.5
            elif s.data == "gauss":
                # the fresh handle the GPU test builds at the end trains the step the mutated one was built with
                assert p.model.n >= 300 and np.array_equal(sq8.train_step(p.model.rows), step), name
                assert np.array_equal(step, np.full(d, np.float32(M.CLIP) / np.float32(127.0), np.float32))


def test_edges_switches_the_option_off_and_on_under_a_subset_above_the_floor():
    """Flat handles: with the option off and a live subset of at least 4096 rows the subset pass must stay away, and
    come back with the option - both inside one hand-written script, not left to the generated ones."""
    tr = [s for s in trace("edges", False) if s["built"]]
    big = [(s["small_batch"], max(s["subsets"].values(), default=0) >= FLOOR) for s in tr]
    off = big.index((False, True))
    assert (True, True) in big[off + 1:] and (False, True) in big[off + 2:]
    assert all(s["n"] >= FLOOR for s in tr[:off + 3]), "the f16 / sq8 passes see the toggles above their floor too"


@pytest.mark.parametrize("d, named", [(100, True), (100, False), (384, True)])
def test_ties_every_kth_score_is_shared_after_every_mutation(d, named):
    """Computed from the model alone (integer data: float64 products are exact): after every mutation, for each of the
    16 queries and k in TIES_K, at least two live rows hold the k-th best score - over all rows, over the rows of the
    subset, and inside the single best list of the query (what nprobe = 1 searches). named=False: the rows filed under
    their default lists, as the build_on_device handle files them."""
    s = M.SCRIPTS["ties"]
    cent = M.centroids(d)
    q = M.queries(s, d, "int")[:16].astype(np.float64)
    p = M.Player(s, d, cent, named=named)
    checked = 0
    dup_ranks_after = 0
    for st in p.steps():
        if not (p.built and st.op[0] in ("add", "remove", "build")):
            continue
        m = p.model
        S = q @ m.rows.astype(np.float64).T
        best = np.argmax(q @ cent.astype(np.float64).T, axis=1)
        pools = [np.ones(m.n, bool)] + [np.isin(m.tokens, t) for t in m.subsets.values()]
        for i in range(16):
            # (default lists are uneven - a query's best list may hold a hundred rows -, so the one-list pool, which goes
            # beyond the condition as stated, is held where the lists are drawn evenly)
            for pool in pools + ([m.lists == best[i]] if named else []):
                sc = np.sort(S[i, pool])[::-1]
                for k in TIES_K:
                    if sc.size >= k:
                        assert (sc == sc[k - 1]).sum() >= 2, (st.index, i, k)
                        checked += 1
        if st.op[:3:2] == ("add", "dup"):
            # an exact copy of a live row sits behind its original: same score, larger row number
            x0 = st.x[0]
            twins = np.flatnonzero((m.rows == x0).all(axis=1))
            assert twins.size >= 2 and twins[-1] >= m.n - st.x.shape[0]
            dup_ranks_after += 1
    assert checked >= 400 and dup_ranks_after >= 3
    # removals take some, but not all, rows of tied groups: the best score's group of query 0 before / after a removal
    p = M.Player(s, d, cent, named=named)
    partly, before = 0, None
    for st in p.steps():
        m = p.model
        if st.op[0] == "remove" and p.built and st.removed:
            tokens, scores = before
            alive = np.isin(tokens, m.tokens)
            for v in np.unique(scores)[::-1][:5]:  # the five best score groups of query 0
                group = scores == v
                if group.sum() >= 2 and 0 < alive[group].sum() < group.sum():
                    partly += 1
                    break
        before = (m.tokens.copy(), q[0] @ m.rows.astype(np.float64).T)
    assert partly >= 3, "every removal of the script splits one of the best tied groups"


# ---- 2. the model against a naive restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(M.SCRIPTS))
def test_model_against_a_naive_restatement(name):
    s = M.SCRIPTS[name]
    d = 8
    p = M.Player(s, d, None if s.named else M.centroids(d))
    state, subsets, issued = [], {}, 0  # [(token, row, list)], {key: set of tokens}
    for st in p.steps():
        kind = st.op[0]
        if kind == "add":
            state = state + [(issued + j, st.x[j].copy(), int(st.lists[j])) for j in range(st.x.shape[0])]
            issued += st.x.shape[0]
        elif kind == "remove":
            sel = st.sel
            if sel.dtype == bool:
                gone = {i for i, b in enumerate(sel.tolist()) if b}
            else:
                gone = {int(r) for r in sel.tolist() if 0 <= int(r) < len(state)}
            assert st.removed == len(gone), (st.index, st.op)
            state = [t for i, t in enumerate(state) if i not in gone]
        elif kind == "subset_new":
            subsets[st.key] = {state[i][0] for i, b in enumerate(st.sel.tolist()) if b}
        elif kind == "subset_close":
            del subsets[st.key]
        m = p.model
        assert m.n == len(state), (st.index, st.op)
        assert m.tokens.tolist() == [t[0] for t in state], (st.index, st.op)
        assert m.lists.tolist() == [t[2] for t in state], (st.index, st.op)
        assert np.array_equal(m.rows, np.array([t[1] for t in state], np.float32).reshape(-1, d)), (st.index, st.op)
        assert sorted(m.subsets) == sorted(subsets)
        for key, toks in subsets.items():
            assert m.subset_rows(key).tolist() == [i for i, t in enumerate(state) if t[0] in toks], (st.index, key)
            want = [sum(1 for t in state if t[0] in toks and t[2] == l) for l in range(M.NLIST)]
            assert m.list_sizes(key).tolist() == want
        assert m.list_sizes().tolist() == [sum(1 for t in state if t[2] == l) for l in range(M.NLIST)]


def brute(rows, pos, q, k):
    """float64 scores of rows[pos]; best first under (score descending, current row ascending)."""
    D, I = M.Model.padding(q.shape[0], k)
    for i in range(q.shape[0]):
        sc = rows[pos].astype(np.float64) @ q[i].astype(np.float64)
        order = sorted(range(len(pos)), key=lambda j: (-sc[j], pos[j]))[:k]
        D[i, :len(order)] = sc[order]
        I[i, :len(order)] = [pos[j] for j in order]
    return D, I


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_model_search_on_the_tied_script_against_brute_force(dtype):
    """Integer data: every product is exact, so the references the model calls must equal a float64 brute force whose
    only tie rule is the current row number - flat, through a subset, and through probed lists. Also holds the one
    shortcut the GPU test takes: the best 10 of a query are the first 10 of its best 100."""
    s, d, k = M.SCRIPTS["ties"], 100, 100
    cent = M.centroids(d)
    q = M.queries(s, d, "int")[:3]
    p = M.Player(s, d, cent)
    for st in p.steps():
        if not (p.built and st.op[0] in ("add", "remove")):
            continue
        m = p.model
        rows = m.stored(dtype)
        D, I = m.search(q, k, dtype)
        Db, Ib = brute(rows, list(range(m.n)), q, k)
        assert np.array_equal(I, Ib) and np.array_equal(D, Db), st.index
        D10, I10 = m.search(q, 10, dtype)
        assert np.array_equal(I10, I[:, :10]) and np.array_equal(D10, D[:, :10])
        probed = np.argsort(-(q.astype(np.float64) @ cent.astype(np.float64).T), axis=1, kind="stable")
        for key in [None] + list(m.subsets):
            member = np.ones(m.n, bool) if key is None else np.isin(m.tokens, m.subsets[key])
            if key is not None:
                D, I = m.search(q, k, dtype, key=key)
                Db, Ib = brute(rows, np.flatnonzero(member).tolist(), q, k)
                assert np.array_equal(I, Ib) and np.array_equal(D, Db), (st.index, key)
            for nprobe in (1, 4):
                D, I = m.search_ivf(cent, q, k, nprobe, dtype, key=key)
                for i in range(q.shape[0]):
                    pos = np.flatnonzero(member & np.isin(m.lists, probed[i, :nprobe])).tolist()
                    Db, Ib = brute(rows, pos, q[i:i + 1], k)
                    assert np.array_equal(I[i], Ib[0]) and np.array_equal(D[i], Db[0]), (st.index, key, nprobe, i)


# ---- 3. the host-buffered half of IVFFlatIndex ----------------------------------------------------------------------------------
def buffered_cases():
    out = [(name, False) for name, s in sorted(M.SCRIPTS.items())]
    return out + [("late_build", True), ("late_build_default_lists", True)]


@pytest.mark.parametrize("name, whole", buffered_cases())
def test_host_buffered_ivf_index_follows_the_model(name, whole):
    """The ops before the script's build (whole: the build deleted, every add / remove / toggle of the script) on an
    IVFFlatIndex that has no handle: ntotal, the buffered rows and the buffered lists equal the model's after every op."""
    s, d = M.SCRIPTS[name], 20
    cent = M.centroids(d)
    p = M.Player(s, d, cent)
    ix = IVFFlatIndex(d, M.NLIST, small_batch=True)
    ix.set_centroids(cent)
    ran = 0
    for st in p.steps():
        kind = st.op[0]
        if kind == "build":
            if whole:
                continue
            break
        if kind == "add":
            ix.add(st.x, assign=st.lists if s.named else None)
        elif kind == "remove":
            assert ix.remove_ids(st.sel) == st.removed, (st.index, st.op)
        elif kind == "toggle":
            ix.set_small_batch(p.small_batch)
        else:
            continue  # (a subset needs the device object)
        ran += 1
        m = p.model
        assert ix._handle is None, "no handle is created"
        assert ix.ntotal == m.n, (st.index, st.op)
        assert np.array_equal(ix.reconstruct_n(), m.rows), (st.index, st.op)
        if m.n:
            assert np.array_equal(ix.reconstruct_n(m.n - 1, 1), m.rows[-1:])
        if s.named and m.n:
            assert np.array_equal(np.concatenate(ix._assign), m.lists), (st.index, st.op)
        elif not s.named:
            assert ix._assign is None
        assert ix.small_batch == p.small_batch
    assert ran >= (7 if whole else 1)


# ---- 4. the plans, chained ----------------------------------------------------------------------------------------------------
def test_chained_plans_under_sanitizers(tmp_path):
    """tests/mutation_chain_check.cpp: csrc/ls_ivf_add_plan.h and csrc/ls_ivf_remove_plan.h (with the subset kernels'
    deal) chained over 200 random histories of 12 steps in a plain host program with its own main, built with
    AddressSanitizer and UndefinedBehaviorSanitizer."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host check of the chained plans"
    exe = tmp_path / "mutation_chain_check"
    p = subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", str(CSRC),
                        str(ROOT / "tests" / "mutation_chain_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.strip() == "OK 200 histories 2400 steps"
