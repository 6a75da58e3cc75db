"""The small-batch switches' rule table (csrc/ls_switch_plan.h) without a GPU: the header in a plain host program with its own
main (tests/switch_plan_check.cpp), built with AddressSanitizer and UndefinedBehaviorSanitizer, held row for row to what the
library's setters answered on real handles at the parent commit (tests/switch_ledger_c_parent.txt)."""

import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "lean-explore_amd" / "csrc"
CHECK = str(ROOT / "tests" / "switch_plan_check.cpp")
TABLE = str(ROOT / "tests" / "switch_ledger_c_parent.txt")


def test_switch_plan_under_sanitizers_against_the_parent_ledger(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host check of ls_switch_plan.h"
    exe = tmp_path / "switch_plan_check"
    p = subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", str(CSRC), CHECK, "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([str(exe), TABLE], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    assert p.stdout.split() == ["ok", "82", "table", "rows"], p.stdout  # (9 flat handles x 8 calls + 5 IVF handles x 2)


# One term of a rule changed, as (the header's text, its replacement). The ledger alone must refuse each. (That sq8 and l2
# refuse a group handle cannot be held this way: no sq8 or L2 group handle can be built to record a row from.)
MUTANTS = [
    ("if (enable && group)", "if (group)"),                                     # subset: switching off on a group is LS_OK
    ("if (enable && group)", "if (enable && group && dtype == LS_DTYPE_F32)"),   # subset: the group's words come before the dtype's
    ('if (enable && dtype != LS_DTYPE_F32)\n            return refuse("ls_set_subset',
     'if (dtype != LS_DTYPE_F32)\n            return refuse("ls_set_subset'),   # subset: switching off on fp16 rows is LS_OK
    ('if (l2) return refuse("ls_set_f16', 'if (l2 && dtype == LS_DTYPE_F16) return refuse("ls_set_f16'),  # f16: L2 before the dtype
    ('if (dtype == LS_DTYPE_F16) return refuse("ls_set_sq8', 'if (false) return refuse("ls_set_sq8'),    # sq8: fp16 rows' own words
    ("if (enable && l2)", "if (l2)"),                                           # ivf: switching off on an L2 handle is LS_OK
]


def test_the_ledger_refuses_single_term_changes_of_the_rules(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host check of ls_switch_plan.h"
    header = (CSRC / "ls_switch_plan.h").read_text()
    procs = []
    for i, (old, new) in enumerate(MUTANTS):
        assert header.count(old) == 1, old
        inc = tmp_path / f"m{i}" / "lean-explore_amd" / "csrc"  # (the header reaches include/ by a relative path)
        inc.mkdir(parents=True)
        (inc / "ls_switch_plan.h").write_text(header.replace(old, new))
        shutil.copytree(ROOT / "include", tmp_path / f"m{i}" / "include")
        procs.append(subprocess.Popen([gxx, "-O0", "-std=c++17", "-I", str(inc), CHECK, "-o", str(inc / "check")],
                                      stderr=subprocess.PIPE, text=True))
    for i, (p, (old, new)) in enumerate(zip(procs, MUTANTS)):
        assert p.wait(timeout=300) == 0, (old, p.stderr.read()[-1000:])
        r = subprocess.run([str(tmp_path / f"m{i}" / "lean-explore_amd" / "csrc" / "check"), TABLE], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "the table says" in r.stderr, f"the ledger does not notice: {old!r} -> {new!r}"


def test_one_home_for_the_drain_sequences_and_the_apply_step():
    """What the table replaced stays replaced: ls_i_flush_deferred has one caller outside ls_batched.hip, ls_i_batched_repair
    and ls_i_export_flags (ls_i_settle), and index.py applies a switch to a handle in one place. A tripwire on the source
    text, no proof: it matches the lines `if (int rc = ls_i_flush_deferred(ix)) return rc;` as they are written today, so a
    reformat of ls_api.hip trips it, and a caller written another way (`return ls_i_flush_deferred(ix);`) slips past it."""
    callers = []
    for f in sorted(CSRC.glob("*.hip")):
        if f.name != "ls_batched.hip":
            callers += [f.name for line in f.read_text().splitlines() if "ls_i_flush_deferred(ix)" in line and "int rc" in line]
    assert callers == ["ls_api.hip"] * 3, callers  # ls_i_batched_repair, ls_i_export_flags, ls_i_settle
    index_py = (ROOT / "lean-explore_amd" / "index.py").read_text()
    assert index_py.count("native.check(lib.ls_set_") == 1 and index_py.count("SWITCHES[name].symbol") == 1  # (the base; a switch)
