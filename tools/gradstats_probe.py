#!/usr/bin/env python
"""Timing probe: the fused training step with and without the gradient densification statistics (trainer.GradientStats) at config 3 — the bench's
map (2M Gaussians, random scene, SH degree 3, Morton order, learning rates x0.01) and view (1920 x 1080).  One process, one model: after warm-up the
two variants are timed in alternating rounds with device events (ms per step, median of the rounds)
  plain   training_step_fused(...)                      gslic_rasterize_backward_adam
  stats   training_step_fused(..., grad_stats=st)       gslic_rasterize_backward_adam_stats (the rule inside the per-Gaussian kernel)
then the library profiler's K_PREPROCESS_BWD class of each (ms per step), and the stand-alone gslic_gradient_stats_accumulate alone (ms per call).
    python tools/gradstats_probe.py [P W H rounds steps_per_round]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_lic_amd  # noqa: F401,E402
from gaussian_lic_amd import _lib, trainer  # noqa: E402
from gaussian_lic_amd.camera import synthetic_camera  # noqa: E402
from gaussian_lic_amd.synthetic import gt_image, random_scene  # noqa: E402

P, W, H, ROUNDS, N = (int(v) for v in (sys.argv[1:6] + ["2000000", "1920", "1080", "5", "100"][len(sys.argv) - 1:]))
dev = torch.device("cuda:0")
model = trainer.GaussianModel(random_scene(P, W, H, sh_degree=3, seed=0), dev, order="morton")
model.training_setup({k: v * 0.01 for k, v in trainer.DEFAULT_LRS.items()})
cam = synthetic_camera(W, H).to_device(dev)
gt = gt_image(H, W, seed=2).to(dev)
bg = torch.zeros(3, device=dev)
st = trainer.GradientStats(model)
print(f"P={P} W={W} H={H} rounds={ROUNDS} steps/round={N}", flush=True)

variants = {
    "plain": lambda: trainer.training_step_fused(model, cam, gt, bg),
    "stats": lambda: trainer.training_step_fused(model, cam, gt, bg, grad_stats=st),
}


def clock(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


for fn in variants.values():
    clock(fn, 10)
times = {k: [] for k in variants}
for r in range(ROUNDS):
    for name, fn in variants.items():
        times[name].append(clock(fn, N))
    print("round", r, " ".join(f"{k}={v[-1]:.4f}" for k, v in times.items()), flush=True)
med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
print("median ms/step:", " ".join(f"{k}={v:.4f}" for k, v in med.items()), f"views/s plain={1e3 / med['plain']:.1f} stats={1e3 / med['stats']:.1f}", flush=True)
print("min    ms/step:", " ".join(f"{k}={min(v):.4f}" for k, v in times.items()), flush=True)
print(f"stats / plain (medians): {med['stats'] / med['plain']:.4f}", flush=True)
seen = st.n_seen()
print(f"rows seen {int((seen > 0).sum())} of {P}; views accumulated {int(seen.max())}", flush=True)

for name, fn in variants.items():
    clock(fn, 3)
    _lib.profile_reset()
    _lib.profile_enable(True)
    clock(fn, N)
    k = _lib.profile_collect()
    _lib.profile_enable(False)
    print(f"kernels {name} (ms/step, launches/step):", " ".join(f"{kn} {ms / N:.4f} {nl / N:.1f}" for kn, (ms, nl) in sorted(k.items()) if nl), flush=True)

m2d = torch.randn(P, 3, device=dev)
radii = (torch.rand(P, device=dev) < 0.6).to(torch.int32) * 5
print(f"stand-alone kernel: {clock(lambda: st.accumulate_from(m2d, radii), N):.4f} ms/call on {int((radii > 0).sum())} visible rows", flush=True)
