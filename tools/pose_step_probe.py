#!/usr/bin/env python
"""Timing probe: the joint map + camera-pose step (gslic_rasterize_backward_camera: preprocess_bwd_kernel<.., CAM = true>) and the N > 1 style
un-fused backward (no Adam inside: gradients written), per step and per kernel.  python tools/pose_step_probe.py [P W H n]
Depth leg: `python tools/pose_step_probe.py [P W H n] --depth [rounds]` times the colour-only pose step against the pose step under LiDAR depth
supervision (gslic_rasterize_backward_depth_camera; the target of tools/depth_step_probe.py) in alternating rounds of n steps in one process, ms per
step between two device synchronisations, then prints the library profiler's per-kernel table of both."""
import os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_lic_amd
from gaussian_lic_amd import trainer, _lib
from gaussian_lic_amd.camera import synthetic_camera
from gaussian_lic_amd.synthetic import random_scene, gt_image
from gaussian_lic_amd.trainer import DEFAULT_LRS
DEPTH = "--depth" in sys.argv
ROUNDS = 5
if DEPTH:
    tail = sys.argv[sys.argv.index("--depth") + 1:]
    ROUNDS = int(tail[0]) if tail else 5
    sys.argv = sys.argv[:sys.argv.index("--depth")]
P, W, H, N = (int(v) for v in (sys.argv[1:5] + ["2000000", "1920", "1080", "100"][len(sys.argv) - 1:]))
dev = torch.device("cuda:0")
raw = random_scene(P, W, H, 3, 0)
model = trainer.GaussianModel(raw, dev, order="morton")
model.training_setup({k: v * 0.01 for k, v in DEFAULT_LRS.items()})
cam = synthetic_camera(W, H, 3).to_device(dev); gt = gt_image(H, W, seed=2).to(dev); bg = torch.zeros(3, device=dev)
def clock(fn, n=N):
    for _ in range(10): fn()
    torch.cuda.synchronize()
    _lib.profile_reset(); _lib.profile_enable(True)
    t = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize(); dt = 1e3 * (time.perf_counter() - t) / n
    k = _lib.profile_collect(); _lib.profile_enable(False)
    return round(dt, 4), {n_: round(v[0] / max(v[1], 1), 4) for n_, v in k.items() if n_ in ("preprocess_bwd", "adam", "render_bwd")}
for _ in range(25): trainer.training_step_fused(model, cam, gt, bg)
if not DEPTH: print("pose_step", clock(lambda: trainer.training_step_with_pose(model, cam, gt, bg, pose_lr=1e-6)), flush=True)
if not DEPTH: print("fused_step", clock(lambda: trainer.training_step_fused(model, cam, gt, bg)), flush=True)
if DEPTH:
    LAMBDA_D = 0.1
    gtd = cam.project_depth(raw["xyz"][::20].to(dev) * 1.05)
    legs = {"pose_step": lambda: trainer.training_step_with_pose(model, cam, gt, bg, pose_lr=1e-6),
            "pose_step_depth": lambda: trainer.training_step_with_pose(model, cam, gt, bg, pose_lr=1e-6, gt_depth=gtd, lambda_depth=LAMBDA_D)}
    def wall(fn, n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n): fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t) / n
    for fn in legs.values(): wall(fn, 5)
    times = {k: [] for k in legs}
    for r in range(ROUNDS):
        for k, fn in legs.items(): times[k].append(wall(fn, N))
        print("round", r, " ".join(f"{k}={v[-1]:.4f}" for k, v in times.items()), flush=True)
    print("median ms/step:", " ".join(f"{k}={sorted(v)[len(v) // 2]:.4f}" for k, v in times.items()), flush=True)
    print("min    ms/step:", " ".join(f"{k}={min(v):.4f}" for k, v in times.items()), flush=True)
    for name, fn in legs.items():
        wall(fn, 3)
        _lib.profile_reset(); _lib.profile_enable(True)
        wall(fn, N)
        k = _lib.profile_collect(); _lib.profile_enable(False)
        print(f"kernels {name} (ms/step, launches/step; sum {sum(v[0] for v in k.values()) / N:.4f}):", flush=True)
        for kn, (ms, nl) in sorted(k.items(), key=lambda kv: -kv[1][0]):
            print(f"  {kn:18s} {ms / N:8.4f} {nl / N:5.1f}", flush=True)
