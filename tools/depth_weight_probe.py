#!/usr/bin/env python
"""Timing probe: the weighted / Huber depth loss on the single-GPU depth step at config 3 (2M Gaussians, 1920 x 1080, SH 3, Morton row order,
learning rates scaled by 0.01 as bench.py does; the depth target of tools/depth_step_probe.py).  In one process, after warm-up, the variants are
timed in alternating rounds (wall clock between two device synchronisations, ms per step, median of the rounds):
  depth              training_step_fused(gt_depth=, lambda_depth=)                        (today's step: gslic_depth_l1_loss_forward_backward)
  depth_weight       ... depth_weight=range_weight(gt_depth, 0.05, 0.02)                  (gslic_depth_loss_weighted_forward_backward)
  depth_huber        ... depth_huber=0.3
  depth_weight_huber ... both
then the loss call alone on the step's last depth image (device events, ms per call) and the profiler's `depth_loss` row of each variant.
`--baseline` times `depth` alone, with no keyword this probe's commit added: the same file runs on the parent commit's tree.
    python tools/depth_weight_probe.py [--baseline] [P W H rounds steps_per_round]"""
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

argv = [a for a in sys.argv[1:] if a != "--baseline"]
BASELINE = "--baseline" in sys.argv
P, W, H, ROUNDS, N = (int(v) for v in (argv[:5] + ["2000000", "1920", "1080", "7", "20"][len(argv):]))
LAMBDA_D, HUBER = 0.1, 0.3
dev = torch.device("cuda:0")
raw = random_scene(P, W, H, 3, 0)
model = trainer.GaussianModel(raw, dev, order="morton")
model.training_setup({k: v * 0.01 for k, v in DEFAULT_LRS.items()})
cam = synthetic_camera(W, H).to_device(dev)
gt = gt_image(H, W, seed=2).to(dev)
gtd = cam.project_depth(raw["xyz"][::20].to(dev) * 1.05)
bg = torch.zeros(3, device=dev)
base = dict(gt_depth=gtd, lambda_depth=LAMBDA_D)
print(f"P={P} W={W} H={H} lambda_depth={LAMBDA_D} measured_pixels={int((gtd > 0).sum())} rounds={ROUNDS} steps/round={N} baseline={BASELINE}", flush=True)

variants = {"depth": lambda: trainer.training_step_fused(model, cam, gt, bg, **base)}
if not BASELINE:
    w = trainer.range_weight(gtd, 0.05, 0.02)
    variants.update({
        "depth_weight": lambda: trainer.training_step_fused(model, cam, gt, bg, depth_weight=w, **base),
        "depth_huber": lambda: trainer.training_step_fused(model, cam, gt, bg, depth_huber=HUBER, **base),
        "depth_weight_huber": lambda: trainer.training_step_fused(model, cam, gt, bg, depth_weight=w, depth_huber=HUBER, **base),
    })


def clock(fn, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t) / n


for fn in variants.values():
    clock(fn, 5)
times = {k: [] for k in variants}
for r in range(ROUNDS):
    for name, fn in variants.items():
        times[name].append(clock(fn, N))
    print("round", r, " ".join(f"{k}={v[-1]:.4f}" for k, v in times.items()), flush=True)
print("median ms/step:", " ".join(f"{k}={sorted(v)[len(v) // 2]:.4f}" for k, v in times.items()), flush=True)
print("min    ms/step:", " ".join(f"{k}={min(v):.4f}" for k, v in times.items()), flush=True)

for name, fn in variants.items():
    clock(fn, 3)
    _lib.profile_reset()
    _lib.profile_enable(True)
    clock(fn, N)
    k = _lib.profile_collect()
    _lib.profile_enable(False)
    ms, nl = k.get("depth_loss", (0.0, 0))
    print(f"profiler {name}: depth_loss {ms / N:.4f} ms/step in {nl / N:.1f} launches; all kernels {sum(v[0] for v in k.values()) / N:.4f} ms/step", flush=True)

if not BASELINE:
    from gaussian_lic_amd import loss  # noqa: E402
    fl = loss.FusedLoss(0.2)
    depth = torch.where(gtd > 0, gtd + 0.4 * torch.randn(H, W, device=dev), torch.rand(H, W, device=dev) * 10.0)
    calls = {"depth": lambda: fl.depth_forward_backward(depth, gtd, LAMBDA_D), "depth_weight": lambda: fl.depth_forward_backward(depth, gtd, LAMBDA_D, w),
             "depth_huber": lambda: fl.depth_forward_backward(depth, gtd, LAMBDA_D, None, HUBER),
             "depth_weight_huber": lambda: fl.depth_forward_backward(depth, gtd, LAMBDA_D, w, HUBER)}

    def clock_ev(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    for fn in calls.values():
        clock_ev(fn, 20)
    ct = {k: [] for k in calls}
    for r in range(ROUNDS):
        for name, fn in calls.items():
            ct[name].append(clock_ev(fn, 200))
    print("loss call alone, median ms/call:", " ".join(f"{k}={sorted(v)[len(v) // 2]:.4f}" for k, v in ct.items()), flush=True)
