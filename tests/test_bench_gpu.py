"""bench.py's launch contract: `--gpus N` must really run N ranks (self-spawned under
torch.distributed.run when no launcher set WORLD_SIZE) or refuse to print a line; the default
single-GPU `--full` line must carry both halves of BASELINE's metric plus the host-API block; a plain
run times the headline only and `--dump-outputs` writes what its last timed step computed."""

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def run_bench(args, env_extra=None, timeout=900, full=True):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, str(ROOT / "bench.py")] + (["--full"] if full else []) + args, env=env,
                       timeout=timeout, capture_output=True, text=True)
    # stdout: `[bench details] {...}` (everything), `[bench summary] {...}`, then the ONE compact JSON line the driver
    # parses. The tests read the details; `_line` / `_line_len` / `_summary` carry the other two.
    lines = p.stdout.splitlines()
    det = [ln for ln in lines if ln.startswith("[bench details] ")]
    summ = [ln for ln in lines if ln.startswith("[bench summary] ")]
    last = [ln for ln in lines if ln.startswith("{")]
    if not det or not last:
        return p, None
    out = json.loads(det[-1][len("[bench details] "):])
    assert lines[-1] == last[-1], "the compact JSON line must be the LAST stdout line"
    out["_line"] = json.loads(last[-1])
    out["_line_len"] = len(last[-1])
    out["_summary"] = json.loads(summ[-1][len("[bench summary] "):]) if summ else None
    return p, out


def test_gpus_2_self_spawns_two_ranks():
    """One GPU here: the two ranks share it over gloo (LS_BENCH_SHARE_GPU, a rehearsal of the
    N > 1 code path: row shards, pipelined packed all-gather, strided merge, max-over-ranks)."""
    p, out = run_bench(["--gpus", "2", "--workload", "c1", "--steps", "48", "--warmup", "8",
                        "--secondary", "none", "--no-host-api", "--no-cpu-baseline",
                        "--launcher", "torchrun"],
                       {"LS_BENCH_SHARE_GPU": "1"})
    assert p.returncode == 0, p.stderr[-2000:]
    assert out is not None and out["n_gpus"] == 2 and out["rccl_ranks_seen"] == 2
    assert out["recall_at_k"] == 1.0 and "rehearsal" in out
    assert out["config"]["parallelism"] == "row-shard x2" and out["config"]["rows_per_gpu"] == 5000


def test_gpus_2_batched_exchange_rehearsal():
    """The batched (MFMA) path sharded two ways: async local search, flags shipped with the
    results, finish() after the timed region."""
    p, out = run_bench(["--gpus", "2", "--workload", "c3", "--steps", "6", "--warmup", "2",
                        "--secondary", "none", "--no-host-api", "--no-cpu-baseline",
                        "--launcher", "torchrun"],
                       {"LS_BENCH_SHARE_GPU": "1"})
    assert p.returncode == 0, p.stderr[-2000:]
    assert out["n_gpus"] == 2 and out["recall_at_k"] == 1.0


@pytest.mark.parametrize("workload,steps", [("c1", 40), ("c3", 6), ("c4", 3)])
def test_gpus_n_in_one_process_through_the_sharded_handle(workload, steps):
    """`bench.py --gpus 3` with no launcher: ONE process, the library's own sharded handle
    (ls_create_sharded). One GPU here, so the three shards share it (copies instead of RCCL)."""
    p, out = run_bench(["--gpus", "3", "--workload", workload, "--steps", str(steps), "--warmup", "2",
                        "--secondary", "none", "--no-host-api", "--no-cpu-baseline",
                        "--c4-rows", "200000"], {"LS_BENCH_SHARE_GPU": "1"})
    assert p.returncode == 0, p.stderr[-2000:]
    assert out["n_gpus"] == 3 and out["config"]["parallelism"] == "row-shard x3"
    assert out["recall_at_k"] == 1.0 and "one process" in out["process_model"]
    assert "rehearsal" in out and out["devices_seen"] == 1 and out["rccl_ranks_seen"] == 0


@pytest.mark.parametrize("workload,steps", [("c2", 24), ("c4", 3)])
def test_gpus_8_in_library_rehearsal(workload, steps):
    """The shape of the one-shot 8-GPU run, rehearsed on this box's single GPU: eight shards behind
    one handle, forced enqueue workers, exchange + merge, the JSON line with the exchange record."""
    p, out = run_bench(["--gpus", "8", "--workload", workload, "--steps", str(steps), "--warmup", "2",
                        "--secondary", "none", "--no-host-api", "--no-cpu-baseline",
                        "--c4-rows", "100000"], {"LS_BENCH_SHARE_GPU": "1"})
    assert p.returncode == 0, p.stderr[-2000:]
    assert out["n_gpus"] == 8 and out["config"]["parallelism"] == "row-shard x8"
    assert out["recall_at_k"] == 1.0 and "rehearsal" in out
    info = out["exchange_info"]
    assert len(info["devices"]) == 8 and len(info["peer_access"]) == 8
    assert "copies" in out["exchange"] and out["rccl_ranks_seen"] == 0


def test_gpus_8_torchrun_rehearsal():
    """The driver's own N = 8 command (`python -m torch.distributed.run --nproc-per-node 8 bench.py
    --gpus 8`), eight ranks sharing this box's GPU over gloo: c2 as the headline plus the c3 / c4
    secondaries the default line carries at N > 1 (c4 reduced to 100 k rows per rank)."""
    p, out = run_bench(["--gpus", "8", "--steps", "16", "--warmup", "4", "--no-host-api",
                        "--no-cpu-baseline", "--c4-rows", "100000", "--launcher", "torchrun"],
                       {"LS_BENCH_SHARE_GPU": "1"}, timeout=1500)
    assert p.returncode == 0, p.stderr[-3000:]
    assert out["n_gpus"] == 8 and out["rccl_ranks_seen"] == 8 and "rehearsal" in out
    assert out["recall_at_k"] == 1.0 and out["config"]["rows_per_gpu"] == 25000
    assert out["secondary"]["c3"]["recall_at_k"] == 1.0 and out["secondary"]["c4"]["recall_at_k"] == 1.0
    assert out["secondary"]["c4"]["scaling"] == "weak"


def test_refuses_rank_count_it_cannot_run():
    import torch

    if torch.cuda.device_count() >= 2:
        pytest.skip("needs a box with fewer GPUs than requested ranks")
    p, out = run_bench(["--gpus", "2", "--workload", "c1", "--steps", "4", "--warmup", "1",
                        "--secondary", "none", "--no-host-api", "--no-cpu-baseline"])
    assert p.returncode != 0 and out is None
    p, out = run_bench(["--gpus", "1", "--workload", "c1", "--steps", "4", "--warmup", "1"],
                       {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode != 0 and out is None


def test_default_line_carries_both_metric_halves_and_host_api():
    p, out = run_bench(["--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--c4-rows", "2000000"])
    assert p.returncode == 0, p.stderr[-2000:]
    assert out["secondary"]["c4"]["recall_at_k"] == 1.0 and out["secondary"]["c2p"]["recall_at_k"] == 1.0
    assert out["n_gpus"] == 1 and out["config"]["workload"].startswith("c2:")
    assert out["recall_at_k"] == 1.0 and 0.3 < out["roofline"]["frac"] <= 1.0
    c3 = out["secondary"]["c3"]
    assert c3["recall_at_k"] == 1.0 and c3["roofline"]["bound"] == "mfma"
    assert 0.0 < c3["roofline"]["frac_whole_batch"] <= c3["roofline"]["frac"] <= 1.0
    for w in ("c2", "c2p"):
        assert out["host_api"][w]["us_per_call_mean"] > 0
    # round 5: the zero-excuse parity block on the timed arrays, the 8-queries-per-pass shapes, concurrent callers
    assert out["parity"]["kernel_order_mismatches"] == 0 and out["parity"]["bit_identical_queries"] == 1
    for w in ("c2x8", "c2px8"):
        x = out["secondary"][w]
        assert x["recall_at_k"] == 1.0 and x["roofline"]["kernel"] == "ls_mq_kernel"
        assert x["parity"]["kernel_order_mismatches"] == 0 and x["parity"]["bit_identical_queries"] == 8
    cc = out["host_api"]["concurrent_callers"]
    assert cc["callers_2"]["queries_per_s"] > cc["callers_1"]["queries_per_s"] and cc["combined_batches"] > 0
    cp = out["host_api"]["concurrent_callers_c2p"]  # long passes: the callers are gathered into one pass
    assert cp["callers_4"]["queries_per_s"] > 1.5 * cp["callers_1"]["queries_per_s"]
    # round 6: the line the driver records is short (its record keeps ~2 KB verbatim) and carries BOTH halves of
    # BASELINE's metric: the batch-1024 block (c3) and config 4 nested inside `roofline`
    line = out["_line"]
    assert out["_line_len"] < 2000, out["_line_len"]
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in line, key
    assert line["value"] == out["value"] and line["config"]["workload"].startswith("c2:")
    b1024 = line["roofline"]["batch1024"]
    assert b1024["workload"].startswith("c3:") and b1024["bound"] == "mfma" and b1024["recall"] == 1.0
    assert b1024["frac"] == c3["roofline"]["frac"] and 0 < b1024["frac_whole_batch"] <= b1024["frac"]
    assert b1024["value"] == c3["value"] and b1024["kernel_ms"] > 0
    assert line["roofline"]["c4"]["workload"].startswith("c4:") and line["roofline"]["c4"]["recall"] == 1.0
    assert line["roofline"]["frac"] == out["roofline"]["frac"]
    summ = out["_summary"]
    assert summ["host_api"]["c2"]["scan_kernel_us"] > 0 and summ["bm25"]["bit_exact_vs_oracle"] is True
    assert summ["host_api"]["c2"]["us_per_call_p50"] > summ["host_api"]["c2"]["scan_kernel_us"]


def test_scale_day_script_rehearsal():
    """tools/scale_day.sh (verdict r5 item 7): the one script for the first N-GPU node - bit-equality of sharded
    results with one index in both process models, bench.py at G = 1, 2 for c2 and c4, the exchange record and
    the table - rehearsed with two shards sharing this box's GPU and reduced sizes."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update({"SCALE_SHARE": "1", "SCALE_C4_ROWS": "100000", "SCALE_STEPS_C2": "48", "SCALE_STEPS_C4": "3",
                "SCALE_CHECK_ROWS": "20000", "SCALE_CHECK_C2_ROWS": "40000"})
    p = subprocess.run(["bash", str(ROOT / "tools" / "scale_day.sh"), "2"], env=env, timeout=1500, capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-2000:])
    assert "scale_check inlib: OK" in p.stdout and "scale_check dist: OK" in p.stdout and "scale_day: OK" in p.stdout
    assert "bit-identical to one index" in p.stdout and "DIFFERS" not in p.stdout
    rows = [ln for ln in p.stdout.splitlines() if ln.startswith("| inlib |") or ln.startswith("| dist |")]
    assert len(rows) == 8, rows  # 2 models x 2 workloads x G = 1, 2
    assert "exchange:" in p.stdout


def test_plain_run_times_the_headline_and_dumps_its_last_step(tmp_path):
    """No --full: the K timed steps and the result line only; --dump-outputs holds the last timed step's rows in
    the order of the workload's queries (c2x8: each step searches the 8 queries rotated, 37 steps end mid-cycle)."""
    from oracle import oracle

    p, out = run_bench(["--workload", "c2x8", "--steps", "37", "--warmup", "3", "--dump-outputs", str(tmp_path)],
                       full=False)
    assert p.returncode == 0, p.stderr[-2000:]
    line = out["_line"]
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 37 and line["warmup"] == 3 and line["ms_per_step"] > 0 and line["dtype"] == "f32"
    assert "secondary" not in out and "host_api" not in out and "roofline" not in line and out["_summary"] is None
    s, i = np.load(tmp_path / "scores.npy"), np.load(tmp_path / "indices.npy")
    assert s.dtype == np.float32 and i.dtype == np.float64 and s.shape == i.shape == (8, 50)
    corpus, queries = H.gauss(1234, 200_000, 384), H.gauss(5678, 8, 384)  # bench.py's c2x8 inputs
    Dr, Ir = oracle.c_search(corpus, queries, 50)
    _, _, S = oracle.np_search(corpus, queries, 50)
    assert oracle.compare_topk(s, i.astype(np.int64), Dr, Ir, S)["recall"] == 1.0
