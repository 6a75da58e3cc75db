"""Scripted histories of add / remove / subset calls on a built index, and the host model they are held to. Shared by
tests/test_mutation_scripts_cpu.py and tests/test_mutation_scripts_gpu.py; nothing here touches a GPU or a library
handle.

The MODEL holds, per live row, a unique token (a running counter over every row ever added), the row's float32 values
as given and its list. A row's current number is its position in the live order; ``add`` appends, ``remove`` drops the
selected positions, and a subset is the SET OF TOKENS selected when it was made: its current rows are the positions of
its live tokens, ascending, and rows added later never join it. There is no renumbering arithmetic in the model: nothing
it computes can share a mistake with csrc/ls_ivf_remove_plan.h, csrc/ls_ivf_add_plan.h or csrc/ls_remove.hip.

Expected search results come from the host references of tests/test_geometry_cpu.py only: ``Flat.topk`` over a row list
(flat and flat-subset search) and ``ivf_reference`` (IVF search; for a subset the same function with the rows outside
the subset given no list, which leaves ``rows of the probed lists`` & ``subset rows``). An index whose adds name no lists
files a row under ``oracle.c_search(cent, x, 1, order="scan")``. Stored values: f32 as is, f16 ``astype(float16)``, sq8
``sq8.encode`` / ``decode`` with the step of the corpus the handle was BUILT from (a mutated handle never retrains).

A SCRIPT is named, seeded, plain data: a tuple of ops
    ("add", m, how)        how: "fresh" rows | "dup" exact copies of live rows | "back" the rows the last removal took |
                           "loud" fresh rows of 4 times the scale (an sq8 handle that retrained its step would show)
    ("remove", kind, arg)  kind: one of REMOVE_KINDS
    ("subset_new", share)  a random `share` of the live rows
    ("subset_close", i)    the i-th subset the script made
    ("toggle", option)     flips the handle's small-batch option (a handle is made with it ON where its kind has one)
    ("build",)             the first point at which the device handle exists
and a ``Player`` turns it into concrete rows, lists and selections from the script's seed, moving the model along."""

from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from lean_explore_amd import sq8
from oracle import oracle
from tests import helpers as H
from tests.test_geometry_cpu import Flat, ivf_reference
from tests.test_sq8_cpu import NEG

NLIST = 16
FLOOR = 4096  # LS_MQ_MIN_ROWS (csrc/ls_mq_plan.h): below it the small-batch passes decline
NQ = 40       # queries made per script (the first 16 serve every check but the 40-query call of the flat f32 handle)
CLIP = 2.0    # Gaussian rows are clipped to +-CLIP: any few hundred of them train the same sq8 step, CLIP / 127
TIE_COLUMNS = 24  # integer queries are zero past this column: scores are sums of 24 values of {-1, 0, 1}
REMOVE_KINDS = ("share", "head", "tail", "list", "all_but_one", "everything", "nothing", "out_of_range", "duplicated")
ADD_HOWS = ("fresh", "dup", "back", "loud")
LOUD = 4.0    # "loud" rows are fresh rows times LOUD: an sq8 step trained on them is LOUD times the one of the build
OP_KINDS = ("add", "remove", "subset_new", "subset_close", "toggle", "build")


# ---- the model ------------------------------------------------------------------------------------------------------------
class Model:
    def __init__(self, d):
        self.d = int(d)
        self.tokens = np.zeros(0, np.int64)
        self.rows = np.zeros((0, self.d), np.float32)
        self.lists = np.zeros(0, np.int32)
        self.issued = 0       # tokens handed out so far
        self.subsets = {}     # key -> the tokens selected when the subset was made
        self.made = 0         # subsets made so far (the next key)
        self._flat = {}

    @property
    def n(self):
        return self.tokens.shape[0]

    def add(self, x, lists):
        x = np.ascontiguousarray(x, np.float32).reshape(-1, self.d)
        lists = np.asarray(lists, np.int32).reshape(-1)
        assert lists.shape[0] == x.shape[0]
        self.tokens = np.concatenate([self.tokens, np.arange(self.issued, self.issued + x.shape[0], dtype=np.int64)])
        self.rows = np.concatenate([self.rows, x])
        self.lists = np.concatenate([self.lists, lists])
        self.issued += x.shape[0]
        self._flat.clear()

    def selected(self, sel):
        """The positions a selection names: a bool mask [n], or row ids (repeats count once, ids outside [0, n) name
        nothing)."""
        sel = np.asarray(sel)
        if sel.dtype == bool:
            assert sel.shape == (self.n,)
            return sel.copy()
        gone = np.zeros(self.n, bool)
        for r in sel.tolist():
            if 0 <= r < self.n:
                gone[r] = True
        return gone

    def remove(self, sel):
        gone = self.selected(sel)
        keep = ~gone
        self.tokens, self.rows, self.lists = self.tokens[keep], self.rows[keep], self.lists[keep]
        self._flat.clear()
        return int(gone.sum())

    def subset_new(self, mask):
        key, self.made = self.made, self.made + 1
        self.subsets[key] = self.tokens[np.asarray(mask, bool)].copy()
        return key

    def subset_close(self, key):
        del self.subsets[key]

    def subset_rows(self, key):
        return np.flatnonzero(np.isin(self.tokens, self.subsets[key]))

    def list_sizes(self, key=None):
        lists = self.lists if key is None else self.lists[self.subset_rows(key)]
        return np.bincount(lists, minlength=NLIST).astype(np.int64)

    # ---- what a handle of `dtype` stores and answers
    def stored(self, dtype, step=None):
        if dtype == "f16":
            return self.rows.astype(np.float16).astype(np.float32)
        if dtype == "sq8":
            return sq8.decode(sq8.encode(self.rows, step), step)
        return self.rows.copy()

    def flat(self, dtype, step=None):
        if dtype not in self._flat:
            self._flat[dtype] = Flat(self.rows, dtype, step=step)
        return self._flat[dtype]

    @staticmethod
    def padding(nq, k):
        return np.full((nq, k), NEG, np.float32), np.full((nq, k), -1, np.int64)

    def search(self, q, k, dtype, step=None, key=None):
        """Flat search of the live rows, or of the subset `key`: Flat.topk over the row list."""
        rows = np.arange(self.n) if key is None else self.subset_rows(key)
        if rows.size == 0:
            return self.padding(q.shape[0], k)
        return self.flat(dtype, step).topk(rows, np.ascontiguousarray(q, np.float32), k)

    def search_ivf(self, cent, q, k, nprobe, dtype, step=None, key=None):
        """ivf_reference over the live rows; for a subset the rows outside it are given no list (-1 is no centroid's
        number), so a query's rows are those of its probed lists that the subset holds."""
        if self.n == 0:
            return self.padding(q.shape[0], k)
        lists = self.lists
        if key is not None:
            lists = np.where(np.isin(self.tokens, self.subsets[key]), self.lists, -1)
        D, I, _ = ivf_reference(self.rows, cent, lists, q, k, nprobe, False, dtype, flat=self.flat(dtype, step))
        return D, I


def default_lists(cent, x):
    """The list of every row of an index whose adds name none: the largest inner product with the centroids in the scan
    kernels' summation order, the lowest list among equals."""
    if x.shape[0] == 0:
        return np.zeros(0, np.int32)
    _, I = oracle.c_search(cent, x, 1, order="scan")
    return np.maximum(I[:, 0], 0).astype(np.int32)


# ---- scripts --------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Script:
    name: str
    seed: int
    ops: tuple
    data: str = "gauss"    # "gauss": clipped Gaussian rows; "int": rows and queries of {-1, 0, 1} (H.int_corpus)
    ivf_only: bool = False
    named: bool = True     # on IVF handles: every add names its lists; False: none does


def update_cycles(rounds=6, name="update_cycles"):
    """`rounds` rounds of "remove 10 %, add 10 %"; one subset made before round 1 and one between rounds 3 and 4."""
    ops = [("add", 5000, "fresh"), ("build",), ("subset_new", 0.5)]
    for r in range(1, rounds + 1):
        ops += [("remove", "share", 0.10), ("add", 500, "fresh")]
        if r == 3:
            ops.append(("subset_new", 0.4))
    return Script(name, 101, tuple(ops))


def random_script(seed, nops=12):
    """An initial corpus, the build and `nops` ops drawn from the seed. Where fewer than 500 rows are left the next op
    is an add of several hundred, so a history recovers from "everything" and the corpus at the end still trains the
    sq8 step it began with."""
    rng = np.random.default_rng(seed)
    ops = [("add", int(rng.integers(4500, 7000)), "fresh"), ("build",)]
    made, live = 0, []
    n = ops[0][1]  # (a rough count: shares are expectations)
    for i in range(nops):
        r = rng.random()
        if n < 500:  # nearly empty: the next op is an add of several hundred fresh rows
            m = int(rng.integers(600, 900))
            ops.append(("add", m, "fresh"))
            n += m
        elif r < 0.30:
            m = int(rng.choice([0, 1, 63, int(rng.integers(200, 900))]))
            ops.append(("add", m, str(rng.choice(["fresh", "fresh", "dup", "back"]))))
            n += m
        elif r < 0.65:
            kind = str(rng.choice(REMOVE_KINDS, p=[0.45, 0.1, 0.1, 0.1, 0.05, 0.05, 0.05, 0.05, 0.05]))
            arg = {"share": round(float(rng.uniform(0.05, 0.4)), 2), "head": int(rng.integers(1, 400)),
                   "tail": int(rng.integers(1, 400))}.get(kind)
            ops.append(("remove", kind, arg))
            n = {"share": int(n * (1 - arg)) if kind == "share" else n, "head": max(n - (arg or 0), 0),
                 "tail": max(n - (arg or 0), 0), "list": n - n // NLIST, "all_but_one": min(n, 1),
                 "everything": 0}.get(kind, n)
        elif r < 0.82 or not live:
            ops.append(("subset_new", round(float(rng.uniform(0.1, 0.9)), 2)))
            live.append(made)
            made += 1
        elif r < 0.92:
            ops.append(("subset_close", live.pop(int(rng.integers(len(live))))))
        else:
            ops.append(("toggle", "small_batch"))
    return Script(f"random_{seed}", seed, tuple(ops))


SCRIPTS = {s.name: s for s in (
    update_cycles(),
    # list 3 (the largest: the player picks it) is emptied while subset 0 holds rows of it, refilled by the rows that
    # were taken, covered by subset 1; then ntotal -> 0 -> add -> remove
    Script("empty_and_refill", 102, (
        ("add", 4800, "fresh"), ("build",), ("subset_new", 0.5), ("remove", "list", None), ("add", None, "back"),
        ("subset_new", 0.6), ("remove", "everything", None), ("add", 700, "fresh"), ("remove", "share", 0.3))),
    # small-batch option on; ntotal 6000 -> 3000 -> 7000 -> 5000. Subset 0 (4500 rows) falls below the floor with the
    # first removal; subset 1 is made above it (4900 rows of the regrown index) and falls below it with the second
    Script("across_the_floor", 103, (
        ("add", 6000, "fresh"), ("build",), ("subset_new", 0.75), ("remove", "share", 0.5),
        ("add", 4000, "fresh"), ("subset_new", 0.7), ("remove", "share", 0.2857))),
    # IVF only: four mutations of the host buffers, the build, three mutations of the handle
    Script("late_build", 104, (
        ("add", 3000, "fresh"), ("remove", "share", 0.2), ("add", 2500, "fresh"), ("remove", "head", 300), ("build",),
        ("subset_new", 0.5), ("add", 500, "fresh"), ("remove", "share", 0.1), ("add", 63, "dup")), ivf_only=True),
    Script("late_build_default_lists", 104, (
        ("add", 3000, "fresh"), ("remove", "share", 0.2), ("add", 2500, "fresh"), ("remove", "head", 300), ("build",),
        ("subset_new", 0.5), ("add", 500, "fresh"), ("remove", "share", 0.1), ("add", 63, "dup")), ivf_only=True,
        named=False),
    # integer rows and queries: removals take some rows of every tied group, adds duplicate live rows exactly (the copy
    # ties with its original and must rank after it)
    Script("ties", 105, (
        ("add", 5000, "fresh"), ("build",), ("subset_new", 0.5), ("remove", "share", 0.3), ("add", 300, "dup"),
        ("remove", "share", 0.1), ("add", 63, "dup"), ("add", 400, "fresh"), ("remove", "list", None),
        ("add", 1, "dup")), data="int"),
    # every add size and every removal kind the other hand-written scripts leave out
    Script("edges", 106, (
        ("add", 4600, "fresh"), ("build",), ("subset_new", 0.5), ("add", 0, "fresh"), ("add", 1, "fresh"),
        ("add", 63, "fresh"), ("remove", "nothing", None), ("remove", "out_of_range", None),
        ("remove", "duplicated", None), ("remove", "head", 100), ("remove", "tail", 100), ("toggle", "small_batch"),
        ("subset_new", 0.95), ("toggle", "small_batch"), ("toggle", "small_batch"),  # (off: a subset above the floor)
        ("subset_close", 0), ("subset_new", 0.3), ("remove", "all_but_one", None), ("add", 600, "fresh"),
        ("remove", "share", 0.2))),
    # adds of another scale than the corpus the handle was built from: an sq8 handle keeps the step of the build (the
    # louder values saturate at code 127), so a handle that retrained on a mutation stores other codes for every row
    Script("louder_adds", 107, (
        ("add", 4600, "fresh"), ("build",), ("subset_new", 0.5), ("add", 500, "loud"), ("remove", "share", 0.2),
        ("add", 300, "loud"), ("remove", "head", 200), ("add", 63, "loud"))),
    random_script(206), random_script(213), random_script(215),
)}


def centroids(d):
    return np.random.default_rng(7700 + d).standard_normal((NLIST, d), dtype=np.float32)


def make_rows(rng, m, d, data):
    if data == "int":
        return H.int_corpus(int(rng.integers(1 << 30)), m, d, -1, 2)
    return np.clip(rng.standard_normal((m, d), dtype=np.float32), -CLIP, CLIP)


def queries(script, d, data):
    """NQ queries of the data kind the rows have; the tied script's are zero past TIE_COLUMNS (few distinct scores)."""
    rng = np.random.default_rng(script.seed * 7919 + d)
    if data == "int":
        q = H.int_corpus(int(rng.integers(1 << 30)), NQ, d, -1, 2)
        if script.data == "int":
            q[:, TIE_COLUMNS:] = 0
        return q
    return rng.standard_normal((NQ, d), dtype=np.float32)


class Step(NamedTuple):
    index: int
    op: tuple
    x: np.ndarray | None = None        # add: the rows ...
    lists: np.ndarray | None = None    # ... and their lists (what the model files them under)
    sel: np.ndarray | None = None      # remove: the selection (mask or ids); subset_new: the mask
    removed: int = 0                   # remove: rows the model dropped
    key: int | None = None             # subset_new / subset_close: the model's key of the subset


class Player:
    """Plays a script on a fresh model. `cent`: the centroids of an IVF handle (None: a flat handle; its rows still
    carry drawn lists, so "one whole list" means the same rows for every kind of handle). `data` overrides the
    script's (f16 handles run every script on integer rows, where the f16 reference is exact), `named` the script's
    (False: no add names its lists, whatever the script says)."""

    def __init__(self, script, d, cent=None, data=None, named=None):
        self.script, self.d, self.cent = script, int(d), cent
        self.data = data or script.data
        self.named = (script.named if named is None else named) or cent is None
        self.rng = np.random.default_rng(script.seed)
        self.model = Model(d)
        self.built = False
        self.small_batch = True
        self.keys = []           # the model's key of every subset the script made, in order
        self.last_removed = None  # (rows, lists) of the most recent removal that took any

    def _lists_of(self, x, drawn):
        return drawn if self.named else default_lists(self.cent, x)

    def steps(self):
        for i, op in enumerate(self.script.ops):
            yield self.apply(i, op)

    def apply(self, i, op):
        m, rng = self.model, self.rng
        kind = op[0]
        if kind == "add":
            count, how = op[1], op[2]
            if how == "back" and self.last_removed is not None:
                x, lists = self.last_removed
                count = x.shape[0] if count is None else min(count, x.shape[0])
                x, lists = x[:count].copy(), lists[:count].copy()
            elif how == "dup" and m.n > 0:
                pick = rng.integers(0, m.n, int(count))
                x, lists = m.rows[pick].copy(), m.lists[pick].copy()
            else:
                count = 300 if count is None else int(count)
                x = make_rows(rng, count, self.d, self.data)
                if how == "loud":
                    x *= np.float32(LOUD)
                lists = rng.integers(0, NLIST, count).astype(np.int32)
            lists = self._lists_of(x, lists)
            m.add(x, lists)
            return Step(i, op, x=x, lists=lists)
        if kind == "remove":
            what, arg, n = op[1], op[2], m.n
            if what == "share":
                sel = rng.random(n) < arg
            elif what == "head":
                sel = np.arange(min(arg, n), dtype=np.int64)
            elif what == "tail":
                sel = np.arange(n) >= n - arg
            elif what == "list":
                sizes = m.list_sizes()
                sel = np.flatnonzero(m.lists == (int(np.argmax(sizes)) if arg is None else arg)).astype(np.int64)
            elif what == "all_but_one":
                sel = np.arange(n) != n // 3
            elif what == "everything":
                sel = np.ones(n, bool)
            elif what == "nothing":
                sel = np.zeros(n, bool)
            elif what == "out_of_range":
                sel = np.array([n, n + 7, -1, 10 ** 9], np.int64)
            elif what == "duplicated":
                sel = np.array([5, 5, 17, n - 1, n - 1, 5, n + 3], np.int64)
            else:
                raise ValueError(op)
            gone = m.selected(sel)
            if gone.any():
                self.last_removed = (m.rows[gone].copy(), m.lists[gone].copy())
            return Step(i, op, sel=sel, removed=m.remove(sel))
        if kind == "subset_new":
            mask = rng.random(m.n) < op[1]
            key = m.subset_new(mask)
            self.keys.append(key)
            return Step(i, op, sel=mask, key=key)
        if kind == "subset_close":
            key = self.keys[op[1]]
            m.subset_close(key)
            return Step(i, op, key=key)
        if kind == "toggle":
            self.small_batch = not self.small_batch
            return Step(i, op)
        if kind == "build":
            self.built = True
            return Step(i, op)
        raise ValueError(op)


def trace(script, d=100, cent=None, data=None):
    """The script played on the model alone: after every op (op, rows, list sizes, {subset key: rows}, built?,
    small-batch option, rows the op added or removed)."""
    p = Player(script, d, cent, data)
    out = []
    for st in p.steps():
        moved = st.x.shape[0] if st.op[0] == "add" else st.removed
        out.append({"op": st.op, "n": p.model.n, "sizes": p.model.list_sizes(),
                    "subsets": {k: int(p.model.subset_rows(k).size) for k in p.model.subsets}, "built": p.built,
                    "small_batch": p.small_batch, "moved": moved})
    return out
