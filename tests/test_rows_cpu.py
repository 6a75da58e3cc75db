"""The kernels of csrc/ls_rows.hip - the device side of ``ls_ivf_add``, ``ls_ivf_remove`` and ``ls_remove`` - without a
GPU: what the gfx950 compile reports of them."""

import re
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "lean-explore_amd" / "csrc"


def test_kernels_use_no_scratch(tmp_path):
    """The gfx950 compile of csrc/ls_rows.hip holds exactly six kernels: TWO instantiations of the row mover's one body
    (every dtype and row geometry; with and without the second source and the ids), the list count and scatter kernels,
    the IVF subset shift and the dst_of scatter. Two, not one: with the source select and the ids check in the loop of a
    single instantiation, the flat removal's move_ms came out 0.5 to 1 % above the spread of two runs of the parent
    (profiles/ab/rows_refactor.txt), so the second source became a template flag. Each kernel reports 0 bytes of scratch,
    no VGPR or SGPR spill and at most 64 VGPRs; the mover uses no LDS, count and scatter the four waves' totals
    (16 bytes); both mover bodies move rows as 16-byte nontemporal loads and stores."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    asm = tmp_path / "rows.s"
    p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=fast",
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S",
                        str(CSRC / "ls_rows.hip"), "-o", str(asm)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|"
                      r"LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1)] = int(m.group(2))
    kinds = ("ls_rows_move_kernel", "ls_list_count_kernel", "ls_list_scatter_kernel", "ls_ivf_subset_shift_kernel",
             "ls_remove_dst_kernel")
    found = {k: [n for n in usage if k in n] for k in kinds}
    movers = sorted(found["ls_rows_move_kernel"])
    assert len(movers) == 2 and "ILb0E" in movers[0] and "ILb1E" in movers[1], movers
    assert all(len(found[k]) == 1 for k in kinds[1:]) and len(usage) == len(kinds) + 1, sorted(usage)
    for n, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (n, u)
        assert u["VGPRs"] <= 64, (n, u)
    for n in movers:
        assert usage[n]["LDS Size [bytes/block]"] == 0, (n, usage[n])
    for k in kinds[1:3]:
        assert usage[found[k][0]]["LDS Size [bytes/block]"] == 16, (k, usage[found[k][0]])  # the four waves' totals
    text = asm.read_text()
    for n in movers:
        body = text[text.index(n + ":"):]
        body = body[:body.index("s_endpgm")]
        assert re.search(r"global_load_dwordx4 .* nt", body) and re.search(r"global_store_dwordx4 .* nt", body), n
