"""GPU: bench.py's plain run and `--dump-outputs`.  A plain run prints the headline fields and none of what `--full` adds; runs with
the same arguments dump the same outputs of their last timed step, with or without `--full` (whose last timed step carries an
event pair around every op); the dumped labels are the class of the smallest mean error."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = {"roofline", "kernels", "parity", "cpu_baseline", "other_workloads"}


def _bench(out_dir, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--workload", "small-unet-2x8", "--dump-outputs", str(out_dir), *extra],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-1000:]
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_the_same_outputs_as_full(tmp_path):
    runs = {name: _bench(tmp_path / name, *extra) for name, extra in (("a", ()), ("b", ()), ("full", ("--full",)))}
    for name, d in runs.items():
        assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
        assert d["unit"] == "images/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
        assert d["metric"] == "images classified/sec (node), small-unet-2x8"
    assert not EXTRAS & set(runs["a"]) and not EXTRAS & set(runs["b"])
    assert {"roofline", "kernels", "parity", "cpu_baseline"} <= set(runs["full"])
    B, C, T = 8, 2, 8
    out = {}
    for name in runs:
        lab, err = np.load(tmp_path / name / "labels.npy"), np.load(tmp_path / name / "errors.npy")
        assert lab.dtype == np.float64 and lab.shape == (B,) and err.dtype == np.float32 and err.shape == (B, C, T)
        out[name] = (lab, err)
    for name in ("b", "full"):
        for x, y in zip(out["a"], out[name]):
            np.testing.assert_array_equal(x, y)
    lab, err = out["a"]
    assert np.isfinite(err).all() and (err > 0).all()
    m = err.astype(np.float64).mean(2)
    assert (m[np.arange(B), lab.astype(np.int64)] <= m.min(1) * (1 + 1e-6)).all()
