"""The batch calls' host-only plan on the CPU: perc_batch_plan.h is the one
copy of the run planner (which trials a launch's rank arrays hold, and under
which numbers its items name them), of the item checks every entry point makes
before a kernel indexes those arrays, and of the orders' inverse permutations."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, os.pardir, "percolation_amd", "csrc")


def test_plan_runs_checks_and_ranks(tmp_path):
    exe = str(tmp_path / "batch_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(HERE, "batch_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("0 violations"), r.stdout[-2000:]
    # nitems 0..12 x (ntrials 1..5: ntrials + 17 maps) x caps 1..13, then the item checks and the orders
    assert int(r.stdout.split()[-4]) >= 13 * 100 * 13 + 3 * 2 * 16 + 8
