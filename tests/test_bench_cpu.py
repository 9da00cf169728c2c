"""bench.py without a GPU: the --dump-outputs writer (caller's row order, fixed sample, size budget) and the option checks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(P, order):   # (a map on the CPU, for bench.py's own functions: not gpu_helpers.scene_model, which builds on the GPU)
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.synthetic import random_scene
    return trainer.GaussianModel(random_scene(P, 64, 48, sh_degree=3, seed=0), torch.device("cpu"), order=order)


@pytest.mark.parametrize("order", ["insertion", "morton"])
def test_dump_outputs_rows_in_the_callers_order(tmp_path, order):
    import bench
    P = 3000
    model, ref = _model(P, order), _model(P, "insertion")
    tie = model.tie_rank if order == "morton" else torch.arange(P)   # original row of every storage row
    vis = tie < 100                                                    # original rows 0 .. 99 seen, wherever they are stored
    names = bench.dump_outputs(str(tmp_path), model, "train", {"terms": torch.tensor([0.25, 0.5]), "visible": vis})
    assert set(names) == {"rows", "loss_terms", "visible"} | set(model.NAMES)
    got = {n: np.load(tmp_path / (n + ".npy")) for n in names}
    assert got["rows"].dtype == np.float64 and np.array_equal(got["rows"], np.arange(P))
    assert all(got[n].dtype == np.float32 for n in names if n != "rows")
    np.testing.assert_array_equal(got["loss_terms"], [0.25, 0.5])
    np.testing.assert_array_equal(got["visible"], (np.arange(P) < 100).astype(np.float32))
    for n in model.NAMES:   # the parameters come back in the order the map was created in
        np.testing.assert_array_equal(got[n], getattr(ref, n).detach().numpy())


def test_dump_outputs_samples_large_maps_within_the_budget(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_ROWS", 500)
    P = 3000
    model = _model(P, "morton")
    names = bench.dump_outputs(str(tmp_path / "a"), model, "train", {"loss": torch.tensor(1.5), "visible": torch.ones(P, dtype=torch.bool)})
    bench.dump_outputs(str(tmp_path / "b"), model, "train", {"loss": torch.tensor(1.5), "visible": torch.ones(P, dtype=torch.bool)})
    rows = np.load(tmp_path / "a" / "rows.npy")
    assert rows.shape == (500,) and np.all(np.diff(rows) > 0) and rows[-1] < P
    ref = _model(P, "insertion")
    for n in names:   # the same sample every time
        a, b = np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy"))
        assert np.array_equal(a, b), n
        if n in model.NAMES:
            np.testing.assert_array_equal(a, getattr(ref, n).detach().numpy()[rows.astype(np.int64)])
    assert sum(os.path.getsize(tmp_path / "a" / (n + ".npy")) for n in names) <= bench.DUMP_BYTES_MAX

    # the default sample of a map of any size stays inside the budget: 60 floats per row, the row list, the loss terms
    monkeypatch.undo()
    assert bench.DUMP_ROWS * (60 * 4 + 8) + 64 <= bench.DUMP_BYTES_MAX


def test_render_mode_dumps_the_visibility_mask_only(tmp_path):
    import bench
    model = _model(200, "insertion")
    names = bench.dump_outputs(str(tmp_path), model, "render", {"visible": torch.ones(200, dtype=torch.bool)})
    assert set(names) == {"rows", "visible"}


@pytest.mark.parametrize("flags", [["--steps", "0"], ["--extras"], ["--profile-all"]])
def test_bench_rejects_flags_before_touching_a_device(flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + flags, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "error" in r.stderr, r.stderr[-1000:]
