"""The hipGraph capture contract (engine.CaptureFailed): a failed capture is reported and ends the process with exit code 3 -- it is never
`recovered' from in-process (round 2's recovery path crashed with SIGSEGV a few seconds later) -- and bench.py probes the capture in a
child process before the measuring process touches the GPU."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_failed_capture_ends_the_process_with_the_reason_and_code_3():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "capture_failure_child.py")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 3, (r.returncode, r.stderr[-2000:])
    assert "hipGraph capture failed" in r.stderr and "trainer refuses further launches" in r.stderr, r.stderr[-2000:]


def test_bench_probes_the_capture_in_a_child_process_first():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--batch", "8", "--steps", "3", "--warmup", "2", "--no-cpu-baseline", "--no-roofline"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert "hipGraph replay" in line["config"]["workload"], line["config"]
    assert "capture probe ok" in r.stderr          # the child's verdict (its stderr is inherited)


def test_plain_bench_times_the_steps_and_dumps_the_last_one(tmp_path):
    """A plain run prints the contract line without the --full measurements, and --dump-outputs writes the last timed step's results."""
    import numpy as np
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--batch", "8", "--steps", "4", "--warmup", "2", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 4 and line["ms_per_step"] > 0 and line["roofline"] is None and line["cpu_baseline"] is None, line
    for k in ("metric", "value", "unit", "higher_is_better", "dtype"):
        assert k in line, k
    losses = np.load(tmp_path / "losses.npy")
    assert losses.dtype == np.float32 and losses.shape == (3,) and np.isfinite(losses).all()
    np.testing.assert_allclose(losses, [line["final_losses"][k] for k in ("g", "d", "info")], atol=1e-4)
    w = np.load(tmp_path / "G.conv_blocks.0.bias.npy")
    assert w.dtype == np.float32 and w.shape == (1024,) and np.isfinite(w).all()
