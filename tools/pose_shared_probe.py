#!/usr/bin/env python
"""Timing probe of the shared extrinsic / time-offset step (gslic_pose_step_shared), modelled on tools/pose_probe.py.  Without arguments it is a
driver that holds no GPU itself: it runs the measurement as ONE child process under a time limit and appends what it prints to the log (its
stderr only when it failed).  The child measures, in one process and in alternating rounds, the median of five:
  kernel    per call as a Python host issues it (device events around back-to-back PoseSet calls on made-up gradients, microseconds per call):
            the shared step on sets of V = 1, 100, 1000 and 5000 views (seeded twists, lr_time != 0: every row moves) against gslic_pose_step
  steps     one joint map + pose step at config 3 (2M Gaussians, 1920 x 1080, SH 3, Morton row order, learning rates scaled by 0.01 as bench.py
            does) with training_step_with_pose(poses=, shared=True) against training_step_with_pose(poses=): wall clock between two device
            synchronisations, ms per step
    python tools/pose_shared_probe.py [--log profiles/pose_shared_config3.log] [P W H rounds steps_per_round]
    python tools/pose_shared_probe.py --leg steps [P W H rounds steps_per_round]      (what the driver starts)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pose_probe import clock, clock_ev   # noqa: E402  (the two clocks of the per-view probe)

LIMIT = 420   # seconds (the leg builds a 2M-Gaussian model)
SIZES = (1, 100, 1000, 5000)


def _args():
    argv, leg, log = list(sys.argv[1:]), None, os.path.join(ROOT, "profiles", "pose_shared_config3.log")
    if "--leg" in argv:
        i = argv.index("--leg"); leg = argv[i + 1]; del argv[i:i + 2]
    if "--log" in argv:
        i = argv.index("--log"); log = argv[i + 1]; del argv[i:i + 2]
    return leg, log, argv, [int(v) for v in (argv[:5] + ["2000000", "1920", "1080", "5", "20"][len(argv):])]


def driver(log, argv):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "steps"] + argv
    os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
    with open(log, "a") as f:
        f.write(f"== steps: python {os.path.relpath(cmd[1], ROOT)} {' '.join(cmd[2:])}\n"); f.flush()
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT)] + cmd, stdout=f, stderr=subprocess.PIPE, text=True, cwd=ROOT)
        if r.returncode != 0:   # (what the child wrote to stderr is kept only when it failed: driver warnings of a box are no measurement)
            f.write(r.stderr)
        f.write(f"== steps: exit status {r.returncode}\n")
    print("steps exit status", r.returncode, flush=True)
    return r.returncode


def leg_steps(P, W, H, ROUNDS, N):
    import torch
    sys.path.insert(0, ROOT)
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import loss, trainer
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import gt_image, random_scene
    dev = torch.device("cuda:0")
    rate = 1e-6   # small: every variant keeps looking at the same scene through the run
    cam = synthetic_camera(W, H).to_device(dev)
    print(f"P={P} W={W} H={H} rounds={ROUNDS} steps/round={N}", flush=True)
    median = lambda v: sorted(v)[len(v) // 2]
    # ---- the launch alone, on made-up (seeded random) camera gradients
    g = torch.Generator().manual_seed(0)
    grads = tuple((1e-3 * torch.randn(n, generator=g)).to(dev) for n in (16, 16, 3))
    per_view = trainer.PoseSet(2, cam, dev, lr_rot=rate, lr_trans=rate)
    calls = {"pose_step": lambda: per_view.adam_step(1, grads)}
    sets = {}
    for V in SIZES:
        ps = sets[V] = trainer.PoseSet(V, cam, dev, lr_rot=rate, lr_trans=rate, shared=True, lr_time=rate)
        ps.twist.copy_(torch.randn(V, 6, generator=g))
        calls[f"shared_V{V}"] = (lambda ps: lambda: ps.shared_adam_step(0, grads))(ps)
    for fn in calls.values():
        clock_ev(fn, 50)
    times = {k: [] for k in calls}
    for r in range(ROUNDS):
        for name, fn in calls.items():
            times[name].append(1e3 * clock_ev(fn, 10 * N))
        print("kernel round", r, " ".join(f"{k}={v[-1]:.2f}" for k, v in times.items()), "us/call", flush=True)
    print("kernel median us/call:", " ".join(f"{k}={median(v):.2f}" for k, v in times.items()), flush=True)
    print("kernel spread us/call (max - min over the rounds):", " ".join(f"{k}={max(v) - min(v):.2f}" for k, v in times.items()), flush=True)
    base = median(times["pose_step"])
    for V in SIZES:
        print(f"shared step at V={V} against gslic_pose_step: {median(times[f'shared_V{V}']) - base:+.2f} us/call", flush=True)
    print("shared sets after the run: ssteps", [int(sets[V].ssteps[0]) for V in SIZES], "tau", [float(sets[V].tau[0]) for V in SIZES], flush=True)
    # ---- the joint step
    raw = random_scene(P, W, H, 3, 0)
    model = trainer.GaussianModel(raw, dev, order="morton")
    model.training_setup({k: v * 0.01 for k, v in trainer.DEFAULT_LRS.items()})
    gt = gt_image(H, W, seed=2).to(dev)
    bg = torch.zeros(3, device=dev)
    fl = loss.FusedLoss(trainer.LAMBDA_DSSIM)
    ps_view = trainer.PoseSet(2, cam, dev, lr_rot=rate, lr_trans=rate)
    ps_shared = trainer.PoseSet(2, cam, dev, lr_rot=rate, lr_trans=rate, shared=True, lr_time=rate)
    variants = {
        "pose_set": lambda: trainer.training_step_with_pose(model, cam, gt, bg, fused_loss=fl, poses=ps_view, view=0),
        "shared": lambda: trainer.training_step_with_pose(model, cam, gt, bg, fused_loss=fl, poses=ps_shared, view=0, shared=True),
    }
    for fn in variants.values():
        clock(fn, 5)
    times = {k: [] for k in variants}
    for r in range(ROUNDS):
        for name, fn in variants.items():
            times[name].append(clock(fn, N))
        print("steps round", r, " ".join(f"{k}={v[-1]:.4f}" for k, v in times.items()), flush=True)
    med = {k: median(v) for k, v in times.items()}
    print("median ms/step:", " ".join(f"{k}={v:.4f}" for k, v in med.items()), flush=True)
    print("spread ms/step (max - min over the rounds):", " ".join(f"{k}={max(v) - min(v):.4f}" for k, v in times.items()), flush=True)
    print(f"shared against pose_set: {med['shared'] - med['pose_set']:+.4f} ms/step ({med['shared'] / med['pose_set']:.4f}x)", flush=True)


if __name__ == "__main__":
    leg, log, argv, sizes = _args()
    if leg is None:
        sys.exit(driver(log, argv))
    leg_steps(*sizes)
