#!/usr/bin/env python
"""Timing probe: one joint map + pose step at config 3 (2M Gaussians, 1920 x 1080, SH 3, Morton row order, learning rates scaled by 0.01 as
bench.py does) with the pose step on the device (training_step_with_pose(poses=...): gslic_pose_step, one launch behind the map's Adam) against
the host route (training_step_with_pose(pose_lr != 0): a blocking copy of 35 floats, the chain in numpy float64, Camera.set_pose, to_device).
Without arguments it is a driver that holds no GPU itself: it runs the measurement as ONE child process under a time limit and appends what it
prints to the log (its stderr only when it failed).  The child measures, in one process and in alternating rounds:
  steps     the two joint steps: wall clock between two device synchronisations, ms per step, median of the rounds
  kernel    gslic_pose_step alone on made-up gradients (device events around back-to-back launches, microseconds per launch, median of the rounds)
    python tools/pose_probe.py [--log profiles/pose_config3.log] [P W H rounds steps_per_round]
    python tools/pose_probe.py --leg steps [P W H rounds steps_per_round]      (what the driver starts)"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 420   # seconds (the leg builds a 2M-Gaussian model)


def _args():
    argv, leg, log = list(sys.argv[1:]), None, os.path.join(ROOT, "profiles", "pose_config3.log")
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


def clock(fn, n):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t) / n


def clock_ev(fn, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def leg_steps(P, W, H, ROUNDS, N):
    import torch
    sys.path.insert(0, ROOT)
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import loss, trainer
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import gt_image, random_scene
    dev = torch.device("cuda:0")
    raw = random_scene(P, W, H, 3, 0)
    model = trainer.GaussianModel(raw, dev, order="morton")
    model.training_setup({k: v * 0.01 for k, v in trainer.DEFAULT_LRS.items()})
    gt = gt_image(H, W, seed=2).to(dev)
    bg = torch.zeros(3, device=dev)
    fl = loss.FusedLoss(trainer.LAMBDA_DSSIM)
    rate = 1e-6   # small: both routes keep looking at the same scene through the run
    cam_host = synthetic_camera(W, H).to_device(dev)
    cam_set = synthetic_camera(W, H).to_device(dev)
    ps = trainer.PoseSet(2, cam_set, dev, lr_rot=rate, lr_trans=rate)
    print(f"P={P} W={W} H={H} rounds={ROUNDS} steps/round={N}", flush=True)
    variants = {
        "host_route": lambda: trainer.training_step_with_pose(model, cam_host, gt, bg, pose_lr=rate, fused_loss=fl),
        "pose_set": lambda: trainer.training_step_with_pose(model, cam_set, gt, bg, fused_loss=fl, poses=ps, view=0),
    }
    for fn in variants.values():
        clock(fn, 5)
    times = {k: [] for k in variants}
    for r in range(ROUNDS):
        for name, fn in variants.items():
            times[name].append(clock(fn, N))
        print("round", r, " ".join(f"{k}={v[-1]:.4f}" for k, v in times.items()), flush=True)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    print("median ms/step:", " ".join(f"{k}={v:.4f}" for k, v in med.items()), flush=True)
    print("min    ms/step:", " ".join(f"{k}={min(v):.4f}" for k, v in times.items()), flush=True)
    print(f"pose_set against host_route: {med['pose_set'] - med['host_route']:+.4f} ms/step ({med['pose_set'] / med['host_route']:.4f}x)", flush=True)
    # the launch alone, on made-up (seeded random) camera gradients
    g = torch.Generator().manual_seed(0)
    grads = tuple((1e-3 * torch.randn(n, generator=g)).to(dev) for n in (16, 16, 3))
    launch = lambda: ps.adam_step(1, grads)
    clock_ev(launch, 50)
    per = sorted(1e3 * clock_ev(launch, 10 * N) for _ in range(ROUNDS))
    print(f"gslic_pose_step alone, back-to-back launches (device events): median {per[len(per) // 2]:.2f} us/launch, min {per[0]:.2f}, max {per[-1]:.2f}",
          flush=True)
    print("row 0 after the run: steps", ps.steps.tolist(), "campos", [round(v, 6) for v in ps.campos[0].tolist()], flush=True)


if __name__ == "__main__":
    leg, log, argv, sizes = _args()
    if leg is None:
        sys.exit(driver(log, argv))
    leg_steps(*sizes)
