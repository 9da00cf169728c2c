#!/usr/bin/env python
"""Timing probe: LiDAR depth supervision on the single-GPU step at config 3 (2M Gaussians, 1920 x 1080, SH 3, Morton row order, learning rates
scaled by 0.01 as bench.py does).  The depth target is a sparse Camera.project_depth image of every 20th point of the scene itself, pushed out by
5 %.  In one process, after warm-up, the variants are timed in alternating rounds (wall clock between two device synchronisations, ms per step):
  fused        training_step_fused, colour only (the headline step)
  fused_depth  training_step_fused(gt_depth=, lambda_depth=)            (depth forward, 4 loss launches, gslic_rasterize_backward_depth_adam)
  autograd_depth  training_step(gt_depth=, lambda_depth=)               (render(return_depth) -> LibTorch loss ops -> backward() -> Adam)
  graphed_depth   GraphedStep(gt_depth=, lambda_depth=, use_graph=True).step
then prints the library profiler's per-kernel table (ms per step) of fused and fused_depth.
    python tools/depth_step_probe.py [P W H rounds steps_per_round]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_lic_amd  # noqa: F401,E402
from gaussian_lic_amd import _lib, trainer  # noqa: E402
from gaussian_lic_amd.camera import synthetic_camera  # noqa: E402
from gaussian_lic_amd.synthetic import gt_image, random_scene  # noqa: E402
from gaussian_lic_amd.trainer import DEFAULT_LRS  # noqa: E402

P, W, H, ROUNDS, N = (int(v) for v in (sys.argv[1:6] + ["2000000", "1920", "1080", "5", "20"][len(sys.argv) - 1:]))
LAMBDA_D = 0.1
dev = torch.device("cuda:0")
raw = random_scene(P, W, H, 3, 0)
model = trainer.GaussianModel(raw, dev, order="morton")
model.training_setup({k: v * 0.01 for k, v in DEFAULT_LRS.items()})
cam = synthetic_camera(W, H).to_device(dev)
gt = gt_image(H, W, seed=2).to(dev)
gtd = cam.project_depth(raw["xyz"][::20].to(dev) * 1.05)
bg = torch.zeros(3, device=dev)
print(f"P={P} W={W} H={H} lambda_depth={LAMBDA_D} measured_pixels={int((gtd > 0).sum())} rounds={ROUNDS} steps/round={N}", flush=True)

graphed = trainer.GraphedStep(model, cam, gt, bg, use_graph=True, gt_depth=gtd, lambda_depth=LAMBDA_D)
variants = {
    "fused": lambda: trainer.training_step_fused(model, cam, gt, bg),
    "fused_depth": lambda: trainer.training_step_fused(model, cam, gt, bg, gt_depth=gtd, lambda_depth=LAMBDA_D),
    "autograd_depth": lambda: trainer.training_step(model, cam, gt, bg, gt_depth=gtd, lambda_depth=LAMBDA_D),
    "graphed_depth": lambda: graphed.step(),
}


def clock(fn, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t) / n


for name, fn in variants.items():   # warm-up (allocations, caches, the graph's first replays)
    clock(fn, 5)
graphed.check()
times = {k: [] for k in variants}
for r in range(ROUNDS):
    for name, fn in variants.items():
        times[name].append(clock(fn, N))
    graphed.check()
    print("round", r, " ".join(f"{k}={v[-1]:.4f}" for k, v in times.items()), flush=True)
print("median ms/step:", " ".join(f"{k}={sorted(v)[len(v) // 2]:.4f}" for k, v in times.items()), flush=True)
print("min    ms/step:", " ".join(f"{k}={min(v):.4f}" for k, v in times.items()), flush=True)

for name in ("fused", "fused_depth"):
    fn = variants[name]
    clock(fn, 3)
    _lib.profile_reset()
    _lib.profile_enable(True)
    clock(fn, N)
    k = _lib.profile_collect()
    _lib.profile_enable(False)
    tot = sum(v[0] for v in k.values()) / N
    print(f"kernels {name} (ms/step, launches/step; sum {tot:.4f}):", flush=True)
    for kn, (ms, nl) in sorted(k.items(), key=lambda kv: -kv[1][0]):
        print(f"  {kn:18s} {ms / N:8.4f} {nl / N:5.1f}", flush=True)
