"""Scripted histories of add / remove_ids / subset calls on built handles on the MI355X, held to the host model of
tests/mutation_scripts.py after EVERY op (include/leansearch_ivf_add.h, leansearch_ivf_remove.h, leansearch_remove.h:
"the handle is, in everything observable, the handle built from scratch from the resulting rows").

Nothing here compares the library with itself but the one check at the end of a script (a fresh handle of the model's
rows): stored rows, lists, subsets and every search result are np.array_equal to what the model says - expected search
results from Flat.topk / ivf_reference of tests/test_geometry_cpu.py, never from a second handle. f16 handles run every
script on integer rows (the f16 reference is exact there); the tied script is integer-valued for f32 too.

The expected results of a step are computed once, for 16 queries and k = 100; a call of fewer queries or a smaller k is
held to the leading queries / ranks of that result (the order is total: score descending, row ascending -
test_mutation_scripts_cpu.py holds the shortcut to the reference itself)."""

import numpy as np
import pytest

from lean_explore_amd import faiss_compat as fc
from lean_explore_amd import native, sq8
from lean_explore_amd.id_selectors import SearchParameters, SearchParametersIVF
from lean_explore_amd.index import FlatIPIndex
from lean_explore_amd.ivf import IVFFlatIndex
from oracle import oracle
from tests import mutation_scripts as M

pytestmark = pytest.mark.gpu

NLIST, FLOOR = M.NLIST, M.FLOOR
NQS, KS, NPROBES = (1, 5, 16), (1, 10, 100), (1, 4, M.NLIST)
SUB_NQS, SUB_KS = (1, 5), (10, 100)

# kind -> (ivf?, dtype, d, constructor keywords, the setter of its small-batch option or None)
KINDS = {
    "ivf_f32_small_batch": (True, "f32", 384, {"small_batch": True}, "set_small_batch"),
    "ivf_f32_build_on_device": (True, "f32", 100, {"build_on_device": True}, None),
    "ivf_f16": (True, "f16", 384, {}, None),
    "ivf_sq8": (True, "sq8", 384, {}, None),
    "flat_f32": (False, "f32", 100, {"subset_small_batch": True}, "set_subset_small_batch"),
    "flat_f16": (False, "f16", 384, {"f16_small_batch": True}, "set_f16_small_batch"),
    "flat_sq8": (False, "sq8", 20, {"sq8_small_batch": True}, "set_sq8_small_batch"),
    "flat_f32_sharded": (False, "f32", 100, {"devices": [0, 0, 0]}, None),
}
# the debug counter that counts the launches of a flat kind's small-batch pass over the whole index (as
# tests/test_mq16_gpu.py and tests/test_mq8_gpu.py use them); flat_f32's option concerns subsets (counter 37, below)
PASS_COUNTER = {"flat_f16": 34, "flat_sq8": 36}
# also through a file and back. (No sq8 case: the file holds the decoded rows, and an sq8 index read from it trains a
# step of its own on them - other codes than the model's.)
WRITTEN = {("update_cycles", "ivf_f32_small_batch"), ("update_cycles", "flat_f32"), ("update_cycles", "flat_f16")}
F16_STATE = [(name, kind) for name in ("update_cycles", "empty_and_refill", "louder_adds")
             for kind in ("ivf_f16", "flat_f16")]


def cases():
    out = []
    for name, s in M.SCRIPTS.items():
        for kind, (ivf, dtype, _, _, _) in KINDS.items():
            if s.ivf_only and not ivf:
                continue
            if s.data == "int" and dtype == "sq8":
                continue  # (the tied script runs as f32 and as f16)
            if kind == "ivf_f32_build_on_device" and not s.named:
                continue  # (this kind runs every script without named lists: it would repeat "late_build")
            out.append((name, kind))
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Subject:
    """The handle under test of one kind, the player of one script, and every check of one step."""

    def __init__(self, script, kind, data=None):
        self.ivf, self.dtype, self.d, self.kw, self.setter = KINDS[kind]
        self.kind = kind
        self.loud = any(op[0] == "add" and op[2] == "loud" for op in script.ops)
        self.data = data or ("int" if self.dtype == "f16" else script.data)
        self.cent = M.centroids(self.d)
        self.named = script.named and kind != "ivf_f32_build_on_device"
        self.p = M.Player(script, self.d, self.cent if self.ivf else None, data=self.data, named=self.named)
        self.q = M.queries(script, self.d, self.data)
        self.ix = self.make()
        self.subs = {}    # the model's key -> the library's subset object
        self.step = None  # the sq8 step the handle was built with

    def make(self, **over):
        kw = dict(self.kw, **over)
        if self.ivf:
            ix = IVFFlatIndex(self.d, NLIST, dtype=self.dtype, **kw)
            ix.set_centroids(self.cent)
            return ix
        return FlatIPIndex(self.d, dtype=self.dtype, **kw)

    @property
    def m(self):
        return self.p.model

    def close(self):
        self.ix.close()

    # ---- one op on the handle
    def apply(self, st):
        kind, ix = st.op[0], self.ix
        if kind == "add":
            if self.ivf:
                ix.add(st.x, assign=st.lists if self.named else None)
            else:
                ix.add(st.x)
        elif kind == "remove":
            assert ix.remove_ids(st.sel) == st.removed, "rows the removal reports"
        elif kind == "subset_new":
            self.subs[st.key] = ix.subset(st.sel)
        elif kind == "subset_close":
            self.subs.pop(st.key).close()
        elif kind == "toggle":
            if self.setter:
                getattr(ix, self.setter)(self.p.small_batch)
        elif kind == "build":
            if self.dtype == "sq8":
                self.step = sq8.train_step(self.m.rows)
            ix._ensure_built()

    # ---- state
    def check_state(self, ix=None):
        ix, m = ix or self.ix, self.m
        assert ix.ntotal == m.n
        if not self.p.built:  # the rows are buffered on the host: nothing below may build the handle
            assert ix._handle is None
            got = ix.reconstruct_n() if self.ivf else ix.host_corpus()
            assert np.array_equal(bits(got), bits(m.rows))
            return
        stored = m.stored(self.dtype, self.step)
        if self.ivf:
            assert native.load().ls_ivf_ntotal(ix._ensure_built()) == m.n
            assert np.array_equal(ix.list_sizes(), m.list_sizes())
            assert np.array_equal(ix.assignment(), m.lists)
            assert np.array_equal(bits(ix.reconstruct_n()), bits(stored))
        else:
            assert native.load().ls_ntotal(ix._ensure_built()) == m.n
            assert np.array_equal(bits(ix.host_corpus()), bits(stored))
            if self.dtype == "sq8":
                assert np.array_equal(ix.sq8_step, self.step)
                assert np.array_equal(ix.codes(), sq8.encode(m.rows, self.step))
            sh = ix.shards()
            assert len(sh) == (3 if "devices" in self.kw else 0)
            if sh:
                assert sum(r for _, _, r in sh) == m.n
                assert [r0 for _, r0, _ in sh] == [0, sh[0][2], sh[0][2] + sh[1][2]], "contiguous bases"

    # ---- searches
    def held(self, got, want, nq, k, what):
        (D, I), (Dw, Iw) = got, want
        assert np.array_equal(I, Iw[:nq, :k]), (what, np.argwhere(I != Iw[:nq, :k])[:5].tolist())
        assert np.array_equal(bits(D), bits(Dw[:nq, :k])), what

    def check_plain(self, ix=None):
        ix, m, q = ix or self.ix, self.m, self.q
        counter = PASS_COUNTER.get(self.kind)
        if self.ivf:
            for nprobe in NPROBES:
                want = m.search_ivf(self.cent, q[:16], 100, nprobe, self.dtype, self.step)
                for nq in NQS:
                    for k in KS:
                        got = ix.search(q[:nq], k, params=SearchParametersIVF(nprobe=nprobe))
                        self.held(got, want, nq, k, ("plain", nq, k, nprobe))
                        if (nq, k, nprobe) == (5, 10, NLIST) and self.dtype == "f32":
                            # the union pass serves the call where the option is on and the index holds the floor's
                            # rows (the bound of a two-query group probing every list is ntotal), the chains elsewhere
                            served = bool(self.kw.get("small_batch")) and self.p.small_batch and m.n >= FLOOR
                            passes = ix.last_passes()[0]
                            assert (passes >= 1) if served else (passes == 0), (passes, m.n, self.p.small_batch)
            return
        want = m.search(q[:16], 100, self.dtype, self.step)
        for nq in NQS:
            for k in KS:
                before = ix.debug_counter(counter) if counter else 0
                self.held(ix.search(q[:nq], k), want, nq, k, ("plain", nq, k))
                if counter and (nq, k) == (5, 10):
                    # the f16 / sq8 small-batch pass serves the call exactly where the option is on and the index
                    # holds the floor's rows; elsewhere the scan groups do and the counter stands still
                    served = self.p.small_batch and m.n >= FLOOR
                    rose = ix.debug_counter(counter) > before
                    assert rose == served, (counter, m.n, self.p.small_batch)
        if self.kind == "flat_f32":
            # 40 queries: past the scan path's 23, where the summation order is the batched pass's ("fma") or, for a
            # query served again by the scan path, "scan": oracle.compare_kernel_order admits exactly these
            D, I = ix.search(q, 10)
            if m.n:
                oracle.compare_kernel_order(D, I, m.rows, q, 10)
            else:
                self.held((D, I), M.Model.padding(q.shape[0], 10), q.shape[0], 10, "40 queries, no rows")

    def check_subsets(self, searches=True):
        ix, m, q = self.ix, self.m, self.q
        assert sorted(self.subs) == sorted(m.subsets)
        for key, sub in self.subs.items():
            rows = m.subset_rows(key)
            assert sub.valid and sub.rows == rows.size, (key, sub.rows, rows.size)
            if self.ivf:
                assert np.array_equal(sub.list_sizes(), m.list_sizes(key)), key
            if not searches:
                continue
            if self.ivf:
                for nprobe in NPROBES:
                    want = m.search_ivf(self.cent, q[:5], 100, nprobe, self.dtype, self.step, key=key)
                    for nq in SUB_NQS:
                        for k in SUB_KS:
                            got = ix.search(q[:nq], k, params=SearchParametersIVF(nprobe=nprobe, sel=sub))
                            self.held(got, want, nq, k, ("subset", key, nq, k, nprobe))
                            if rows.size == 0:
                                assert (got[1] == -1).all() and (got[0] == M.NEG).all()
                continue
            want = m.search(q[:5], 100, self.dtype, self.step, key=key)
            for nq in SUB_NQS:
                for k in SUB_KS:
                    c37 = ix.debug_counter(37)
                    got = ix.search(q[:nq], k, params=SearchParameters(sel=sub))
                    self.held(got, want, nq, k, ("subset", key, nq, k))
                    if rows.size == 0:
                        assert (got[1] == -1).all() and (got[0] == M.NEG).all()
                    if self.kind == "flat_f32" and (nq, k) == (5, 10):
                        # the subset pass serves the call where the option is on and the subset holds the floor's rows
                        served = self.p.small_batch and rows.size >= FLOOR
                        rose = ix.debug_counter(37) > c37
                        assert rose == served, (key, rows.size, self.p.small_batch)

    # ---- once, at the end of the script
    def check_against_a_fresh_handle(self):
        m = self.m
        if self.ivf:
            fresh = self.make(**({"small_batch": self.p.small_batch} if self.setter else {}))
            try:
                fresh.add(m.rows, assign=m.lists if self.named else None)
                fresh._ensure_built()
                assert np.array_equal(fresh.list_sizes(), self.ix.list_sizes())
                assert np.array_equal(fresh.assignment(), self.ix.assignment())
                if not (self.dtype == "sq8" and self.loud):
                    # (a fresh sq8 handle trains its step on the rows it is given: after a loud add that is another
                    # step than the mutated handle's, which keeps the one of its build - other codes, by definition)
                    assert np.array_equal(bits(fresh.reconstruct_n()), bits(self.ix.reconstruct_n()))
                if self.setter and m.n:
                    par = SearchParametersIVF(nprobe=NLIST)
                    a, b = self.ix.search(self.q[:5], 10, params=par), fresh.search(self.q[:5], 10, params=par)
                    assert np.array_equal(a[1], b[1]) and np.array_equal(bits(a[0]), bits(b[0]))
                    assert fresh.last_passes() == self.ix.last_passes()
            finally:
                fresh.close()
            return
        kw = dict(self.kw)
        if self.dtype == "sq8":
            kw["sq8_step"] = self.step
        fresh = FlatIPIndex.from_array(m.rows, dtype=self.dtype, **kw)
        try:
            assert fresh.ntotal == self.ix.ntotal
            assert np.array_equal(bits(fresh.host_corpus()), bits(self.ix.host_corpus()))
            if self.dtype == "sq8":
                assert np.array_equal(fresh.codes(), self.ix.codes())
        finally:
            fresh.close()

    def check_through_a_file(self, path):
        """write_index / read_index: the reloaded index holds the model's state and answers as the model says."""
        fc.write_index(self.ix, path, allow_lossy=self.dtype == "f16")  # (f16: the file holds the rounded rows)
        if self.ivf:
            back = fc.read_index(path, ivf=True, ivf_small_batch=self.p.small_batch)
        elif self.dtype == "f16":
            back = fc.read_index(path, dtype="f16", f16_small_batch=self.p.small_batch)
        else:
            back = fc.read_index(path)
        try:
            self.check_state(back)
            self.check_plain(back)
        finally:
            back.close()


@pytest.mark.parametrize("name, kind", cases())
def test_script(name, kind, tmp_path):
    s = Subject(M.SCRIPTS[name], kind)
    try:
        for st in s.p.steps():
            try:
                s.apply(st)
                s.check_state()
                if s.p.built:
                    s.check_plain()
                    s.check_subsets()
            except AssertionError as e:
                raise AssertionError(f"{name} on {kind}: op {st.index} {st.op}: {e}") from e
        assert s.p.built
        s.check_against_a_fresh_handle()
        if (name, kind) in WRITTEN:
            s.check_through_a_file(tmp_path / "mutated.index")
    finally:
        s.close()


@pytest.mark.parametrize("name, kind", F16_STATE)
def test_f16_rows_with_real_mantissas_survive_the_moves(name, kind):
    """The f16 cases above run on integer rows, where the search reference is exact but `astype(float16)` is the
    identity. Here the same scripts move Gaussian rows: after every op the stored rows equal the model's rows rounded
    to f16 bit for bit, and the state of every subset follows. No search is checked (no exact f16 reference exists
    for such rows)."""
    s = Subject(M.SCRIPTS[name], kind, data="gauss")
    try:
        for st in s.p.steps():
            try:
                s.apply(st)
                s.check_state()
                if s.p.built:
                    s.check_subsets(searches=False)
            except AssertionError as e:
                raise AssertionError(f"{name} on {kind}: op {st.index} {st.op}: {e}") from e
        stored = s.m.stored("f16")
        assert s.p.built and s.m.n > 0 and (stored != s.m.rows).mean() > 0.9, "the rounding is not the identity"
        s.check_against_a_fresh_handle()
    finally:
        s.close()


def test_the_cases_reach_every_kind_and_script():
    cs = cases()
    assert {k for _, k in cs} == set(KINDS) and {n for n, _ in cs} == set(M.SCRIPTS)
    assert WRITTEN <= set(cs)
    for name in ("update_cycles", "empty_and_refill", "across_the_floor", "edges", "louder_adds", "random_206",
                 "random_213", "random_215"):
        assert {k for n, k in cs if n == name} == set(KINDS)
    assert {k for n, k in cs if n == "ties"} == {k for k, v in KINDS.items() if v[1] != "sq8"}
    assert {k for n, k in cs if n.startswith("late_build")} == {k for k, v in KINDS.items() if v[0]}


# ---- HBM after many updates ---------------------------------------------------------------------------------------------
def test_hbm_after_22_update_rounds(capsys):
    """update_cycles for 22 rounds on an IVF f32 handle with two live subsets: free device memory after round 2 and
    after round 22, beside a control that builds a fresh handle of the same rows (and the same subsets) in every round
    and closes it. The mutated handle may not lose more than the control plus one d_ids array (4 n bytes) - asserted
    only where the control itself drifts by less than that: the allocator's granule is not known here.
    Measured on an MI355X: see DESIGN.md section 2."""
    import torch

    script = M.update_cycles(22, "update_cycles_22")
    d, cent = 100, M.centroids(100)
    q = M.queries(script, d, "gauss")[:5]
    par = SearchParametersIVF(nprobe=4)

    def free():
        torch.cuda.synchronize()
        return int(torch.cuda.mem_get_info()[0])

    def fresh_index():
        ix = IVFFlatIndex(d, NLIST, small_batch=True)
        ix.set_centroids(cent)
        return ix

    def rounds(mutate):
        p = M.Player(script, d, cent)
        ix, subs, seen, done = (fresh_index() if mutate else None), {}, {}, 0
        try:
            for st in p.steps():
                kind = st.op[0]
                if mutate:
                    if kind == "add":
                        ix.add(st.x, assign=st.lists)
                    elif kind == "remove":
                        assert ix.remove_ids(st.sel) == st.removed
                    elif kind == "subset_new":
                        subs[st.key] = ix.subset(st.sel)
                    elif kind == "build":
                        ix._ensure_built()
                if not (kind == "add" and p.built):
                    continue
                done += 1  # the end of a round
                if not mutate:  # the control: a fresh handle of the model's rows and subsets, the last one closed
                    if ix is not None:
                        ix.close()
                    ix = fresh_index()
                    ix.add(p.model.rows, assign=p.model.lists)
                    ix._ensure_built()
                    subs = {k: ix.subset(p.model.subset_rows(k)) for k in p.model.subsets}
                ix.search(q, 10, params=par)
                for sub in subs.values():
                    ix.search(q, 10, params=SearchParametersIVF(nprobe=4, sel=sub))
                if done in (2, 22):
                    seen[done] = (free(), p.model.n)
            assert done == 22 and len(subs) == len(p.model.subsets) == 2
            assert ix.ntotal == p.model.n and np.array_equal(ix.assignment(), p.model.lists)
        finally:
            if ix is not None:
                ix.close()
        return seen

    free()  # (the context exists before the first reading)
    control = rounds(False)
    mutated = rounds(True)
    n = mutated[22][1]
    drift_c = control[2][0] - control[22][0]
    drift_m = mutated[2][0] - mutated[22][0]
    with capsys.disabled():
        print(f"\n[hbm] rows {mutated[2][1]} -> {n}; free-memory drift over rounds 2..22: mutated {drift_m} bytes, "
              f"control {drift_c} bytes; one d_ids array {4 * n} bytes")
    if abs(drift_c) < 4 * n:
        assert drift_m <= drift_c + 4 * n, (drift_m, drift_c, 4 * n)
