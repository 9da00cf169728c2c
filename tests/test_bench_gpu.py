"""-m gpu: a plain bench.py run (no --full) prints the headline line only, and --dump-outputs writes the same outputs for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--gaussians", "100000",
           "--width", "640", "--height", "360", "--dump-outputs", str(out_dir)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_its_outputs_repeat(tmp_path):
    d = _bench(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"):
        assert k in d, k
    assert d["steps"] == 4 and d["warmup"] == 2 and d["full"] is False and d["unit"] == "views/s" and d["higher_is_better"] is True
    # both figures are rounded to three decimals (bench.py): value to 0.5e-3 views/s, ms_per_step to 0.5e-3 ms, which moves 1e3 / ms_per_step by
    # up to value * 0.5e-3 / ms_per_step — more than a flat 1e-3 of value once a step is shorter than half a millisecond (0.392 ms here)
    assert d["ms_per_step"] > 0.001
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) <= d["value"] * 0.5e-3 / (d["ms_per_step"] - 0.5e-3) + 1e-3
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["value_long"] is None and d["dropin_host"] is None
    d2 = _bench(tmp_path / "b")
    names = sorted(f for f in os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"rows.npy", "visible.npy", "loss_terms.npy", "xyz.npy", "features_dc.npy", "features_rest.npy", "opacity.npy", "scaling.npy",
            "rotation.npy"} <= set(names)
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.all(np.isfinite(a)), n
        assert np.array_equal(a, b), n   # same arguments: same inputs, and the step is deterministic
        total += os.path.getsize(tmp_path / "a" / n)
    assert total <= 64 << 20
    assert np.load(tmp_path / "a" / "visible.npy").sum() > 0 and d2["steps"] == 4
