"""The host rules that decide what a CG solve runs, on the CPU:
perc_solve_plan.h is the one copy of the family / flag rules (solve_plan), the
march variant choice over the one variant list (select_march), the band policy
and the chunk schedule.  solve_plan_check.cpp sweeps the rules against the
digest of the select_format they replaced, walks a hand table of one case per
rule, and checks that select_march is total over what the host can form and
that no compiled variant is unreachable."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, os.pardir, "percolation_amd", "csrc")


def test_solve_plan_rules(tmp_path):
    exe = str(tmp_path / "solve_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(HERE, "solve_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    # fmt x mode bits x dot order x assembly checks x res_G x slots x rows x rowptr x N
    assert lines[0].startswith("sweep: %d points" % (5 * 128 * 3 * 8 * 2 * 2 * 2 * 2 * 7)), lines[0]
    assert lines[-1].endswith("0 violations") and int(lines[-1].split()[0]) >= 30, lines[-1]


def test_memory_owners_free_once_under_host_sanitizers(tmp_path):
    """DevBuf / PinnedBuf (perc_common.h) over malloc-backed stand-ins of the
    four HIP allocation calls: a stand-alone host program under
    AddressSanitizer and UBSan, no GPU"""
    exe = str(tmp_path / "owner_check")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g",
                           "-Wno-unused-value", "-Xarch_host", "-fsanitize=address,undefined", "-I", CSRC,
                           os.path.join(HERE, "owner_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("0 violations"), r.stdout[-2000:]
