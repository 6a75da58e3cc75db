"""What the Python layer answers for every combination of the small-batch switches, without a device or the library:
each row of the sweep below against tests/switch_ledger_py_parent.txt, recorded by this same file (run as a script, it
prints the ledger) at the commit that file names. Equality is row for row, with no margin.

Part 1, 648 rows: (FlatIPIndex, FlatL2Index) x dtype x metric x placement x switch keywords (none, each alone, each pair,
all four). The answer is the ValueError text, or "ok" with the four properties and what every set_*(True / False) on the
unbuilt object answers, in the order f16, sq8, subset, l2. Part 2, accept / refuse only: the faiss_compat constructors,
read_index keyword combinations on the three containers, and SearchEngine with an injected index."""

import itertools
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

LEDGER = Path(__file__).resolve().parent / "switch_ledger_py_parent.txt"
SWITCHES = ("f16", "sq8", "subset", "l2")
PLACEMENTS = {"single": {}, "sharded": {"devices": [0, 1]}, "replicated": {"devices": [0, 1], "replicate": True}}
SUBSETS = [c for r in (0, 1, 2, 4) for c in itertools.combinations(SWITCHES, r)]


def _call(f):
    try:
        f()
        return "ok"
    except ValueError as e:
        return f"ValueError: {e}"


def flat_rows():
    from lean_explore_amd.index import FlatIPIndex, FlatL2Index

    for cls, dtype, metric, place, on in itertools.product((FlatIPIndex, FlatL2Index), ("f32", "f16", "sq8"),
                                                           (None, "ip", "l2"), PLACEMENTS, SUBSETS):
        name = f"{cls.__name__}/{dtype}/{metric}/{place}/{'+'.join(on) or 'none'}"
        kw = {f"{s}_small_batch": True for s in on}
        try:
            ix = cls(16, dtype=dtype, metric=metric, **PLACEMENTS[place], **kw)
        except ValueError as e:
            yield name, f"ValueError: {e}"
            continue
        ans = ["ok", " ".join(f"{s}={int(getattr(ix, s + '_small_batch'))}" for s in SWITCHES)]
        for s in SWITCHES:
            for v in (True, False):
                ans.append(f"set_{s}({v})=" + _call(lambda: getattr(ix, f"set_{s}_small_batch")(v)))
        ans.append(" ".join(f"{s}={int(getattr(ix, s + '_small_batch'))}" for s in SWITCHES))
        yield name, " | ".join(ans)


def _accepts(f):
    try:
        f()
        return "accepted"
    except ValueError:
        return "refused"


def compat_rows():
    from lean_explore_amd import faiss_compat as F
    from lean_explore_amd.search.engine import SearchEngine

    for metric, dtype, sb in itertools.product((F.METRIC_INNER_PRODUCT, F.METRIC_L2), ("f32", "f16", "sq8"), (False, True)):
        yield f"IndexFlat/{metric}/{dtype}/l2={int(sb)}", _accepts(lambda: F.IndexFlat(16, metric, dtype=dtype, l2_small_batch=sb))
    for dtype, sb in itertools.product(("f32", "f16", "sq8"), (False, True)):
        yield f"IndexFlatIP/{dtype}/subset={int(sb)}", _accepts(lambda: F.IndexFlatIP(16, dtype=dtype, subset_small_batch=sb))
        yield f"IndexFlatL2/{dtype}/l2={int(sb)}", _accepts(lambda: F.IndexFlatL2(16, dtype=dtype, l2_small_batch=sb))
    for metric, sb in itertools.product((F.METRIC_INNER_PRODUCT, F.METRIC_L2), (False, True)):
        yield f"IndexScalarQuantizer/{metric}/sq8={int(sb)}", _accepts(
            lambda: F.IndexScalarQuantizer(16, F.QT_8bit, metric, sq8_small_batch=sb))
    for metric, dtype, ivf, sb in itertools.product((F.METRIC_INNER_PRODUCT, F.METRIC_L2), ("f32", "f16", "sq8"),
                                                    (False, True), (False, True)):
        yield f"IndexIVFFlat/{metric}/{dtype}/ivf={int(ivf)}/ivf_sb={int(sb)}", _accepts(
            lambda: F.IndexIVFFlat(None, 16, 4, metric, dtype=dtype, ivf=ivf, ivf_small_batch=sb))

    rows = np.random.default_rng(5).integers(-3, 4, size=(8, 16)).astype(np.float32)
    with tempfile.TemporaryDirectory() as tmp:
        files = {}
        flat = F.IndexFlatIP(16)
        flat.add(rows)
        files["IxFI"] = Path(tmp) / "ip.index"
        F.write_index(flat, files["IxFI"])
        l2 = F.IndexFlatL2(16)
        l2.add(rows)
        files["IxF2"] = Path(tmp) / "l2.index"
        F.write_index(l2, files["IxF2"])
        for tag, metric in (("IwFl", "ip"), ("IwFl-l2", "l2")):
            ivf = F.IVFFlatIndex(16, 2, metric=metric)
            ivf.set_centroids(rows[:2])
            ivf.add(rows, assign=np.arange(8, dtype=np.int32) % 2)
            files[tag] = Path(tmp) / f"{tag}.index"
            F.write_index(ivf, files[tag])
        keys = ("f16_small_batch", "sq8_small_batch", "ivf_small_batch", "l2_small_batch")
        for tag, dtype, ivf, place in itertools.product(files, ("f32", "f16", "sq8"), (False, True), PLACEMENTS):
            for on in [c for r in (0, 1, 2) for c in itertools.combinations(keys, r)]:
                kw = dict({k: True for k in on}, **PLACEMENTS[place])
                yield (f"read_index/{tag}/{dtype}/ivf={int(ivf)}/{place}/{'+'.join(k[:-12] for k in on) or 'none'}",
                       _accepts(lambda: F.read_index(files[tag], dtype=dtype, ivf=ivf, **kw)))
        for dtype, sem, place, f16, sq8 in itertools.product(("f32", "f16", "sq8"), ("flat", "ivf"), PLACEMENTS,
                                                             (False, True), (False, True)):
            kw = dict(PLACEMENTS[place])
            yield (f"SearchEngine/{dtype}/{sem}/{place}/f16={int(f16)}/sq8={int(sq8)}", _accepts(
                lambda: SearchEngine(base_path=tmp, index=object(), ids_map=[], lexical_retriever=False, storage_dtype=dtype,
                                     semantic_index=sem, f16_small_batch=f16, sq8_small_batch=sq8, **kw)))


def all_rows():
    yield from flat_rows()
    yield from compat_rows()


def ledger():
    out = {}
    for line in LEDGER.read_text().splitlines():
        if line and not line.startswith("#"):
            name, _, answer = line.partition("\t")
            out[name] = answer
    return out


def test_the_flat_index_answers_every_switch_combination_as_the_parent_did():
    want, have = ledger(), dict(flat_rows())
    assert len(have) == 648
    for name, answer in have.items():
        assert name in want, f"{name}: no row in {LEDGER.name}"
        assert answer == want[name], f"{name}: {answer!r}, the ledger says {want[name]!r}"


def test_the_callers_of_the_table_accept_and_refuse_what_the_parent_did():
    want, have = ledger(), dict(compat_rows())
    assert len(have) >= 800
    for name, answer in have.items():
        assert name in want, f"{name}: no row in {LEDGER.name}"
        assert answer == want[name], f"{name}: {answer}, the ledger says {want[name]}"
    assert set(want) == set(have) | set(dict(flat_rows()))


if __name__ == "__main__":
    for name, answer in all_rows():
        print(f"{name}\t{answer}")
