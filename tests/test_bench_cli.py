"""bench.py's command line: a plain run does only what its headline figure
needs, --full adds the legs that take runs of their own, --dump-outputs
writes what the last timed step returned.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the keys of the result line that only --full fills
FULL_ONLY = ("kernel_probe", "stream_copy", "labeling", "in_flight", "cpu_baseline",
             "cpu_baseline_ensemble")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*args, timeout=300):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + list(args),
                       capture_output=True, text=True, timeout=timeout, cwd=REPO, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_dump_outputs_writes_float64_arrays(tmp_path):
    """CPU: dump_outputs writes one float64 .npy per result of a step"""
    sys.path.insert(0, REPO)
    import bench
    d = str(tmp_path / "dump")
    bench.dump_outputs(d, dict(gtop=0.25, gbot=0.125, iter=392, nspan=1, t_total_ms=3.0))
    assert sorted(os.listdir(d)) == ["gbot.npy", "gtop.npy", "iter.npy", "nspan.npy"]
    for name, want in (("gtop", 0.25), ("gbot", 0.125), ("iter", 392.0), ("nspan", 1.0)):
        a = np.load(os.path.join(d, name + ".npy"))
        assert a.dtype == np.float64 and a.shape == (1,) and a[0] == want


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_last_step(tmp_path):
    """A plain run carries the headline figures and none of the --full legs;
    with one timed step the ensemble statistics of the result line are that
    step's results, so the dumped arrays must equal them exactly."""
    d = str(tmp_path / "dump")
    out = _bench("--gpus", "1", "--steps", "1", "--warmup", "1", "--L", "1024", "--dump-outputs", d)
    for k in HEADLINE:
        assert k in out, k
    assert out["steps"] == 1 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert abs(out["value"] - 1e3 / out["ms_per_step"]) <= 1e-2 * out["value"]
    assert not [k for k in FULL_ONLY if k in out]
    assert "achievable" not in out["roofline"]
    got = {n: np.load(os.path.join(d, n + ".npy")) for n in ("gtop", "gbot", "iter", "nspan")}
    assert all(a.dtype == np.float64 and a.shape == (1,) for a in got.values())
    assert got["nspan"][0] >= 1 and out["cg_solves"] == 1
    assert got["gtop"][0] == out["gtop_mean"] > 0
    assert got["iter"][0] == out["cg_iterations_mean"]


@pytest.mark.gpu
def test_full_run_keeps_the_other_legs():
    """--full: the kernel probe, the stream-copy ceiling, the labeling phases
    are in the result line as before (the CPU baselines, minutes of host
    time, are left to a run of the benchmark itself)"""
    out = _bench("--full", "--steps", "1", "--warmup", "0", "--L", "1024", "--no-cpu-baseline",
                 "--inflight", "0")
    for k in HEADLINE + ("kernel_probe", "stream_copy", "labeling"):
        assert k in out, k
    assert out["kernel_probe"] and out["stream_copy"]["gbs"] > 0
    assert out["roofline"]["achievable"] == out["stream_copy"]["gbs"]
