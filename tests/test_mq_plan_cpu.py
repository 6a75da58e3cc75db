"""The one plan of the small-batch passes (csrc/ls_mq_plan.h) without a GPU: tests/mq_plan_check.cpp, a plain host program
built with AddressSanitizer and UndefinedBehaviorSanitizer, holds the header to the table of what the four plan functions
it replaced answered (tests/mq_plan_parent.txt) and runs its own checks for all four kinds; this file reads what it
lists."""

import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "lean-explore_amd" / "csrc"
TABLE = ROOT / "tests" / "mq_plan_parent.txt"


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host check of ls_mq_plan.h"
    exe = tmp_path_factory.mktemp("mq_plan") / "mq_plan_check"
    p = subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", str(CSRC), str(ROOT / "tests" / "mq_plan_check.cpp"),
                        "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([str(exe), str(TABLE)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    return p.stdout.strip().splitlines()


def test_header_answers_the_parent_table_row_for_row(check_output):
    """Every row of the table is answered as the replaced functions answered it; the only difference is an fp32 plan that
    declined with workgroups and k' still set, which is all zeros now. 744 rows of 5 query counts; 292 such plans."""
    m = re.fullmatch(r"ok (\d+) served (\d+) declined (\d+) table rows (\d+) zeroed", check_output[-1])
    assert m, check_output[-1]
    rows = sum(1 for ln in TABLE.read_text().splitlines() if ln and not ln.startswith("#"))
    assert int(m.group(3)) == rows == 744
    zeroed = [ln for ln in check_output if ln.startswith("zeroed ")]
    assert len(zeroed) == int(m.group(4)) == 292
    assert all(ln.startswith("zeroed 0 ") for ln in zeroed)  # fp32 only


def test_only_the_fp32_kind_grants_a_pass_it_cannot_plan(check_output):
    """(kind, rows, k, n_cu) where the grouping rule produces a group that has no plan although the pass is granted: the
    fp32 route grants 32 queries per pass on the eight-wave plan and plans its groups of 2..16 with the four-wave plan,
    which can decline (left as it is here). The other three kinds have one predicate and no such case."""
    defects = [tuple(int(x) for x in ln.split()[1:]) for ln in check_output if ln.startswith("defect ")]
    assert defects and {d[0] for d in defects} == {0}
    assert (0, 200_000, 1100, 256) in defects
