"""The scan path's launch decisions (csrc/ls_scan_call_plan.h) without a GPU: the header in a plain host program with its own
main (tests/scan_call_plan_check.cpp), built with AddressSanitizer and UndefinedBehaviorSanitizer, held row for row to
what the expressions it replaced answered (tests/scan_call_plan_parent.txt), and to four implications over its own sweep."""

import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "lean-explore_amd" / "csrc"


def test_scan_call_plan_under_sanitizers_against_the_parent_table(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host check of ls_scan_call_plan.h"
    exe = tmp_path / "scan_call_plan_check"
    p = subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", str(CSRC), str(ROOT / "tests" / "scan_call_plan_check.cpp"),
                        "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([str(exe), str(ROOT / "tests" / "scan_call_plan_parent.txt")], capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    last = p.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) >= 800, p.stdout[-500:]  # (table rows read)


# One term or one bound of a decision changed, as (the header's text, its replacement). The table alone must refuse each.
MUTANTS = [
    ("!in.profiling && ", ""),                                            # lane_call while ls_set_profiling is on
    (" &&\n                  !(in.stream & LS_STREAM_LANE);", ";"),        # lane_call fed from a lane's own stream
    (">= LS_LANE_MIN_BYTES", "> LS_LANE_MIN_BYTES"),                       # the size rule, exactly at the limit
    ("(240ll << 20)", "(241ll << 20)"),
    ("(in.nq >= 2 || in.elem == 2)", "(in.nq >= 2 || in.elem != 1)"),       # lane_kind: a lone fp32 query is no pass
    ("(in.nq == 1 && in.opt_scan_skip_scores)", "(in.nq <= 2 && in.opt_scan_skip_scores)"),
    ("keff <= 256 &&", "keff <= 257 &&"),                                  # same_launch
    ("blocks * (kprime + 1) <= LS_GRAN_MAX", "blocks * kprime <= LS_GRAN_MAX"),
    ("in.n_groups <= LS_NSETS", "in.n_groups <= 3"),
    ("in.opt_same_launch != 0 && !in.reserving && in.has_done", "in.opt_same_launch != 0 && in.has_done"),
    ("p.host_words = !in.pipeline && in.has_done && in.has_retry", "p.host_words = !in.pipeline && in.has_done"),
    ("in.has_retry && !in.reserving;", "in.has_retry;"),                   # host_words of a retry
    ("(use_mq || (NQ == 1 && in.opt_scan_skip_scores)) && in.repairable &&", "(use_mq || (NQ == 1 && in.opt_scan_skip_scores)) &&"),  # dev_keep
    ("!in.reserving && !in.has_done && in.opt_mq_skip_scores && in.n > 0", "!in.reserving && in.opt_mq_skip_scores && in.n > 0"),
    ("(use_mq || NQ == 1) && in.repairable && !in.reserving && keep_full", "(use_mq || NQ == 1) && in.repairable && keep_full"),  # repair_first
    ("s.repair_first = !lane_call && ", "s.repair_first = "),
    ("NQ > in.s_vecs", "NQ >= in.s_vecs"),                                 # grow_scores
]


def test_the_table_refuses_single_term_changes_of_every_decision(tmp_path):
    """The committed table holds the header at its decision boundaries: a copy of the header with one term of lane_call,
    same_launch, host_words, dev_keep, repair_first or grow_scores dropped, or one bound moved by one, fails the table part
    of the check (no sanitizers here: the mutants are not the code under test)."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host check of ls_scan_call_plan.h"
    header = (CSRC / "ls_scan_call_plan.h").read_text()
    table = str(ROOT / "tests" / "scan_call_plan_parent.txt")
    procs = []
    for i, (old, new) in enumerate(MUTANTS):
        assert header.count(old) == 1, old
        inc = tmp_path / f"m{i}"
        inc.mkdir()
        (inc / "ls_scan_call_plan.h").write_text(header.replace(old, new))
        for dep in ("ls_mq_plan.h", "ls_scan_plan.h"):
            (inc / dep).write_text((CSRC / dep).read_text())
        procs.append(subprocess.Popen([gxx, "-O0", "-std=c++17", "-I", str(inc), str(ROOT / "tests" / "scan_call_plan_check.cpp"),
                                       "-o", str(inc / "check")], stderr=subprocess.PIPE, text=True))
    for i, (p, (old, new)) in enumerate(zip(procs, MUTANTS)):
        assert p.wait(timeout=300) == 0, (old, p.stderr.read()[-1000:])
        r = subprocess.run([str(tmp_path / f"m{i}" / "check"), table, "table"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "the table says" in r.stderr, f"the table does not notice: {old!r} -> {new!r}"
    # ... and the header as it is passes the same part
    exe = tmp_path / "plain"
    subprocess.run([gxx, "-O0", "-std=c++17", "-I", str(CSRC), str(ROOT / "tests" / "scan_call_plan_check.cpp"), "-o", str(exe)],
                   check=True, timeout=300)
    r = subprocess.run([str(exe), table, "table"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout, r.stderr[-1000:])


def test_the_scan_path_reads_no_call_state_from_the_handle():
    """The call context is an argument (ls_scan_call, ls_index.h): none of the seven fields it replaced is left."""
    text = "".join((CSRC / f).read_text() for f in ("ls_index.h", "ls_api.hip", "ls_callers.hip", "ls_batched.hip"))
    for gone in ("done_base", "gran_out_base", "cur_retry", "cur_done_seq", "force_gen", "dev_call_repairable",
                 "ix->reserving"):
        assert gone not in text, gone
