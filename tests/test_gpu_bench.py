"""bench.py on the device: a plain run prints the contract line and nothing of `--full`, runs exactly --steps timed steps,
and --dump-outputs writes the same arrays in every run with the same arguments."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--layers", "1", "--dump-outputs", str(out_dir), *args],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("workload", ["fp8", "mxfp4-sq"])
def test_plain_run_and_its_dump_repeat(workload, tmp_path):
    a = _plain_run(tmp_path / "a", "--workload", workload)
    b = _plain_run(tmp_path / "b", "--workload", workload)
    for line in (a, b):
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in line
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
        assert "extra" not in line and line.get("cpu_baseline") is None and "node_copy_GBs" not in line["roofline"]
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b")) and "weights.npy" in files
    total = 0
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float32 and x.size > 0 and np.isfinite(x).all()
        assert np.array_equal(x, y), f"{workload}: {f} differs between two runs with the same arguments"
        total += x.nbytes
    assert total <= 64 * 1024 * 1024
