"""BM25 over a document subset (include/leansearch_bm25_subset.h) without a GPU: the header and
the binding, the argument checks, the row deal of the score kernel on the host, the engine's lexical package prefilter
on an oracle-backed retriever, and the list-driven kernel's build-time facts."""

import asyncio
import ctypes
import re
import shutil
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from lean_explore_amd import loader, native
from lean_explore_amd import search as S
from lean_explore_amd.search.tokenization import tokenize_raw, tokenize_spaced
from oracle import bm25_ref as R
from tests import helpers as H
from tests.test_subset_cpu import FakeEmbed, ParamsOracleIndex, _make_db

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "leansearch_bm25_subset.h"
CSRC = ROOT / "lean-explore_amd" / "csrc"
NAMES = ["ls_bm25_search_subset", "ls_bm25_subset_create", "ls_bm25_subset_destroy"]
FLT_MAX = np.float32(3.4028234663852886e38)


def ref_subset(ref, query_tokens, rows, k):
    """The host reference of a subset search: the oracle's scores of EVERY document (global statistics), the selected
    documents `rows` (ascending) ordered by (score descending, document ascending), padded with (-1, -FLT_MAX)."""
    s = R.scores(ref, R.token_ids(ref, query_tokens))
    rows = np.asarray(rows, dtype=np.int64)
    order = np.lexsort((rows, -s[rows].astype(np.float64)))[:k]
    docs = np.full(k, -1, dtype=np.int64)
    out = np.full(k, -FLT_MAX, dtype=np.float32)
    docs[: order.size] = rows[order]
    out[: order.size] = s[rows[order]]
    return docs, out


def test_header_declares_exactly_the_three_functions_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ls_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(native.BM25_SUBSET_SYMBOLS) == NAMES
    assert not set(native.BM25_SUBSET_SYMBOLS) & set(native.SYMBOLS)
    raw = ctypes.CDLL(str(native.LIB_PATH))
    lib = native.load()
    for n in names:
        assert hasattr(raw, n), f"{n} declared in leansearch_bm25_subset.h but not exported"
        fn = getattr(lib, n)  # load() bound it
        assert fn.restype == native.BM25_SUBSET_SYMBOLS[n][0] and fn.argtypes == native.BM25_SUBSET_SYMBOLS[n][1], n


def test_argument_validation_needs_no_gpu():
    lib = native.load()
    sid, docs = ctypes.c_int32(), ctypes.c_int64()
    bm = (ctypes.c_uint8 * 1)(0xFF)
    tok = (ctypes.c_int32 * 1)(0)
    out_s, out_d = (ctypes.c_float * 4)(), (ctypes.c_int64 * 4)()
    assert lib.ls_bm25_subset_create(None, bm, 1, ctypes.byref(sid), ctypes.byref(docs)) == native.LS_ERR_INVALID_ARG
    assert b"ls_bm25_subset_create" in lib.ls_last_error()
    assert lib.ls_bm25_subset_destroy(None, 1) == native.LS_ERR_INVALID_ARG
    assert b"ls_bm25_subset_destroy" in lib.ls_last_error()
    assert lib.ls_bm25_search_subset(None, 1, tok, 1, 4, out_s, out_d) == native.LS_ERR_INVALID_ARG
    assert b"ls_bm25_search_subset" in lib.ls_last_error()
    assert lib.ls_bm25_search_subset(None, 1, tok, 1, 4, None, None) == native.LS_ERR_INVALID_ARG


def test_every_position_is_dealt_exactly_once(tmp_path):
    """csrc/ls_bm25_deal.h in a plain host program: for every m and workgroup count the kernel's enumeration visits
    each position of [0, m) once, and a lane the kernel masks off never names a position below m."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host check of ls_bm25_deal.h"
    exe = tmp_path / "bm25_deal_check"
    p = subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-I", str(CSRC), str(ROOT / "tests" / "bm25_deal_check.cpp"),
                        "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:]
    assert p.stdout.strip() == f"OK {(70 + 10) * 10} cases"


# ------------------------------------------------------------------ engine glue
BIG = [f"Big.addComm{i}" for i in range(40)]
SMALL = [f"Small.Sub.Deep.addComm{i}Extra" for i in range(10)]
QUERY, BM25_K = "add comm", 5


class RefRetriever:
    """Stand-in for NameRetriever on the CPU oracle: `ids`, `subset(mask)` and `__call__(query, k, subset=None)`."""

    def __init__(self, ids, names):
        self.ids = list(ids)
        self.refs = [(R.build([list(dict.fromkeys(tok(n))) for n in names]), tok)
                     for tok in (tokenize_spaced, tokenize_raw)]
        self.n = len(names)
        self.calls, self.masks = [], []

    def subset(self, mask):
        mask = np.asarray(mask)
        assert mask.dtype == bool and mask.shape == (self.n,)
        self.masks.append(mask.copy())
        rows = np.nonzero(mask)[0]
        return SimpleNamespace(rows=rows, docs=rows.size)

    def __call__(self, *args, **kwargs):
        self.calls.append((args, dict(kwargs)))
        return self._run(*args, **kwargs)

    def _run(self, query, bm25_k, subset=None):
        rows = np.arange(self.n) if subset is None else subset.rows
        k = min(bm25_k, max(1, rows.size))
        out = {}
        for ref, tok in self.refs:
            docs, sc = ref_subset(ref, tok(query), rows, k)
            for d, s in zip(docs.tolist(), sc.tolist()):
                if d >= 0:
                    out[self.ids[d]] = max(out.get(self.ids[d], 0.0), s)
        return out


class NoSubsetRetriever:
    def __init__(self):
        self.calls = 0

    def __call__(self, query, bm25_k):
        self.calls += 1
        return {}


def _engine(tmp_path, retriever_of, extra_names=()):
    names = BIG + SMALL
    n, d = len(names), 16
    corpus = H.gauss(31, n, d)
    rows = []
    for i, name in enumerate(names):
        module = "Big.Mod" if i < 40 else "Small.Sub.Deep"
        rows.append((3000 + i, name, module, None, f"def d{i}", f"http://x/{i}", None, f"informal {i}",
                     loader.embedding_to_blob(corpus[i].tolist())))
    db = tmp_path / "lean_explore.db"
    _make_db(db, rows)
    ids, loaded = loader.load_corpus_from_sqlite(db)
    lex_ids = [3000 + i for i in range(n)] + [999000 + j for j in range(len(extra_names))]
    retriever = retriever_of(lex_ids, names + list(extra_names))
    eng = S.SearchEngine(db_path=db, embedding_client=FakeEmbed(corpus[45] * 2.0), index=ParamsOracleIndex(loaded),
                         ids_map=list(ids), lexical_retriever=retriever)
    return eng, retriever


def _want_small(names, ids, rows):
    want = {}
    for tok in (tokenize_spaced, tokenize_raw):
        ref = R.build([list(dict.fromkeys(tok(n))) for n in names])
        docs, sc = ref_subset(ref, tok(QUERY), rows, min(BM25_K, len(rows)))
        for d, s in zip(docs.tolist(), sc.tolist()):
            if d >= 0:
                want[ids[d]] = max(want.get(ids[d], 0.0), s)
    return want


def test_the_global_top_k_holds_no_small_name():
    """The issue's case on the oracle: the global top-5 of both tokenisations is rows 0-4, all `Big`."""
    for tok in (tokenize_spaced, tokenize_raw):
        ref = R.build([list(dict.fromkeys(tok(n))) for n in BIG + SMALL])
        docs, _ = R.retrieve(ref, tok(QUERY), BM25_K)
        assert docs.tolist() == [0, 1, 2, 3, 4]


def test_lexical_flag_off_calls_the_retriever_exactly_as_before(tmp_path):
    eng, r = _engine(tmp_path, RefRetriever)
    seen = []
    fuse = eng._compute_rrf_scores
    eng._compute_rrf_scores = lambda bm25_map, semantic_map: (seen.append(dict(bm25_map)), fuse(bm25_map, semantic_map))[1]
    asyncio.run(eng.search_prefiltered(QUERY, ["Small"], limit=5, faiss_k=5, bm25_k=BM25_K, rerank_top=None))
    asyncio.run(eng.search_prefiltered(QUERY, ["Small"], limit=5, faiss_k=5, bm25_k=BM25_K, rerank_top=None,
                                       lexical=False))
    asyncio.run(eng.search(QUERY, limit=5, faiss_k=5, bm25_k=BM25_K, rerank_top=None, packages=["Small"]))
    assert r.calls == [((QUERY, BM25_K), {})] * 3 and not r.masks
    small_ids = set(range(3040, 3050))
    assert len(seen) == 3 and all(m and not (set(m) & small_ids) for m in seen)
    asyncio.run(S.Service(engine=eng).search(QUERY, limit=5, rerank_top=None, packages=["Small"], prefilter_packages=True))
    assert r.calls[-1] == ((QUERY, 1000), {}) and not r.masks


def test_lexical_prefilter_returns_the_packages_names(tmp_path):
    eng, r = _engine(tmp_path, RefRetriever)
    seen = []
    fuse = eng._compute_rrf_scores
    eng._compute_rrf_scores = lambda bm25_map, semantic_map: (seen.append(dict(bm25_map)), fuse(bm25_map, semantic_map))[1]
    ids = [3000 + i for i in range(50)]
    want = _want_small(BIG + SMALL, ids, np.arange(40, 50))
    assert len(want) == 5 and set(want) <= set(range(3040, 3050))
    res = asyncio.run(eng.search_prefiltered(QUERY, ["Small"], limit=5, faiss_k=5, bm25_k=BM25_K, rerank_top=None,
                                             lexical=True))
    assert seen[-1] == want
    assert eng._retrieve_bm25_candidates(QUERY, BM25_K, ["Small"]) == want
    assert len(res) == 5 and all(x.module.startswith("Small") for x in res)
    assert len(r.masks) == 1 and np.array_equal(np.nonzero(r.masks[0])[0], np.arange(40, 50))
    assert r.calls[0][0] == (QUERY, BM25_K) and set(r.calls[0][1]) == {"subset"}
    # a second call with the same packages reuses the cached subset; another package set is another subset
    asyncio.run(eng.search_prefiltered(QUERY, ["Small"], limit=5, faiss_k=5, bm25_k=BM25_K, rerank_top=None, lexical=True))
    assert len(r.masks) == 1 and r.calls[-1][1]["subset"] is r.calls[0][1]["subset"]
    asyncio.run(eng.search_prefiltered(QUERY, ["Big", "Small"], limit=5, faiss_k=5, bm25_k=BM25_K, rerank_top=None,
                                       lexical=True))
    assert len(r.masks) == 2 and r.masks[1].all()
    # the service reaches it
    resp = asyncio.run(S.Service(engine=eng).search(QUERY, limit=5, rerank_top=None, packages=["Small"],
                                                    prefilter_packages=True, prefilter_lexical=True))
    assert resp.count == 5 and all(x.module.startswith("Small") for x in resp.results)
    assert len(r.masks) == 2 and set(r.calls[-1][1]) == {"subset"} and r.calls[-1][0] == (QUERY, 1000)
    assert set(seen[-1]) == set(range(3040, 3050))  # (bm25_k = 1000 is cut to the 10 selected documents)


def test_ids_outside_the_database_are_not_selected(tmp_path):
    eng, r = _engine(tmp_path, RefRetriever, extra_names=["Small.ghostAddComm"])
    got = eng._retrieve_bm25_candidates(QUERY, 1000, ["Small"])
    assert np.array_equal(np.nonzero(r.masks[0])[0], np.arange(40, 50))
    assert set(got) == set(range(3040, 3050))


def test_prefilter_lexical_needs_prefilter_packages(tmp_path):
    eng, r = _engine(tmp_path, RefRetriever)
    with pytest.raises(ValueError, match="prefilter_packages"):
        asyncio.run(S.Service(engine=eng).search(QUERY, packages=["Small"], prefilter_lexical=True))
    with pytest.raises(ValueError, match="prefilter_packages"):
        asyncio.run(S.Service(engine=eng).search(QUERY, prefilter_lexical=True))
    assert not r.calls


def test_a_retriever_without_subset_is_refused_before_any_search(tmp_path):
    eng, r = _engine(tmp_path, lambda ids, names: NoSubsetRetriever())
    with pytest.raises(TypeError, match="subset"):
        asyncio.run(eng.search_prefiltered(QUERY, ["Small"], limit=5, faiss_k=5, rerank_top=None, lexical=True))
    assert r.calls == 0 and not eng.faiss_informal_index.calls
    asyncio.run(eng.search_prefiltered(QUERY, ["Small"], limit=5, faiss_k=5, rerank_top=None))  # flag off: served
    assert r.calls == 1


def test_disabled_lexical_signal_and_ivf_refusal_are_unchanged(tmp_path):
    eng, _ = _engine(tmp_path, lambda ids, names: False)
    assert eng._retrieve_bm25_candidates(QUERY, BM25_K, ["Small"]) == {}
    res = asyncio.run(eng.search_prefiltered(QUERY, ["Small"], limit=5, faiss_k=5, rerank_top=None, lexical=True))
    assert len(res) == 5
    ivf = S.SearchEngine(base_path=tmp_path, index=object(), ids_map=[], lexical_retriever=False, semantic_index="ivf")
    with pytest.raises(ValueError, match="ivf"):
        asyncio.run(ivf.search_prefiltered("x", ["Mathlib"], lexical=True))


def test_bm25_subset_python_argument_checks():
    from lean_explore_amd.bm25 import BM25Index, BM25Subset

    ix = BM25Index().index([["a", "b"], ["b"], ["c"]])
    other = BM25Index().index([["a"], ["b"]])
    fake = BM25Subset(other, 1, 1)
    assert not fake.valid  # no handle behind it
    with pytest.raises(ValueError):
        ix.retrieve(["a"], 2, subset=fake)  # a subset of another index
    with pytest.raises(ValueError):
        ix.retrieve(["a"], 2, subset=object())
    with pytest.raises(ValueError):
        ix.subset(np.zeros(5, bool))  # mask of the wrong length


# ------------------------------------------------------------------ build-time facts of the list-driven kernel
def test_list_kernel_uses_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=fast",
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S", str(CSRC / "ls_bm25.hip"),
                        "-o", str(tmp_path / "bm25.s")], capture_output=True, text=True, timeout=900)
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
    kernels = {n: u for n, u in usage.items() if "bm25_score" in n}
    assert len(kernels) == 2 and sum("bm25_score_list_kernel" in n for n in kernels) == 1, sorted(usage)
    for n, u in kernels.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u.get("VGPRs Spill", 0) == 0, (n, u)
