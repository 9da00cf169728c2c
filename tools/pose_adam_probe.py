#!/usr/bin/env python
"""Timing probe: the joint map + pose iteration at config 3 (2M Gaussians, 1920 x 1080, SH 3, Morton row order, learning rates scaled by 0.01 as
bench.py does) with the map's Adam inside the camera backward (gslic_rasterize_backward_camera_adam / _depth_camera_adam) against the two-call
route (the camera backward into the gradient slab, then SparseGaussianAdam.step).  Like tools/pose_probe.py, whose clock and argument parsing it uses:
without arguments it holds no GPU itself and runs the measurement as ONE child process under a time limit, appending what it prints to the log.
The child measures, in one process and in alternating rounds (wall clock between two device synchronisations, ms per step, median of the rounds):
  joint / joint_adam              training_step_with_pose(poses=) without and with adam_in_backward, colour-only
  joint_depth / joint_depth_adam  the same pair under depth supervision
  graphed_train_pose              GraphedStep(poses=, train_pose=True): the joint iteration as one capacity-mode step
  graphed_then_pose               GraphedStep(poses=) followed by pose_gradient(poses=, do_step=True): what a host had to do before
    python tools/pose_adam_probe.py [--log profiles/pose_adam_config3.log] [P W H rounds steps_per_round]
    python tools/pose_adam_probe.py --leg steps [P W H rounds steps_per_round]      (what the driver starts)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pose_probe  # noqa: E402


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
    rate = 1e-6   # small: every route keeps looking at the same scene through the run
    cam = synthetic_camera(W, H).to_device(dev)
    gtd = cam.project_depth(raw["xyz"][::5].float()).to(dev)
    ps = trainer.PoseSet(2, cam, dev, lr_rot=rate, lr_trans=rate)
    dkw = dict(gt_depth=gtd, lambda_depth=0.5)
    step = lambda **kw: trainer.training_step_with_pose(model, cam, gt, bg, fused_loss=fl, poses=ps, view=0, **kw)
    g_joint = trainer.GraphedStep(model, cam, gt, bg, poses=ps, view=0, train_pose=True, check_every=0)
    g_plain = trainer.GraphedStep(model, cam, gt, bg, poses=ps, view=0, check_every=0)

    def graphed_then_pose():
        g_plain.step()
        trainer.pose_gradient(model, cam, gt, bg, fused_loss=fl, poses=ps, view=0, do_step=True)

    print(f"P={P} W={W} H={H} rounds={ROUNDS} steps/round={N}", flush=True)
    variants = {
        "joint": lambda: step(),
        "joint_adam": lambda: step(adam_in_backward=True),
        "joint_depth": lambda: step(**dkw),
        "joint_depth_adam": lambda: step(adam_in_backward=True, **dkw),
        "graphed_train_pose": lambda: g_joint.step(),
        "graphed_then_pose": graphed_then_pose,
    }
    for fn in variants.values():
        pose_probe.clock(fn, 5)
    times = {k: [] for k in variants}
    for r in range(ROUNDS):
        for name, fn in variants.items():
            times[name].append(pose_probe.clock(fn, N))
        print("round", r, " ".join(f"{k}={v[-1]:.4f}" for k, v in times.items()), flush=True)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    print("median ms/step:", " ".join(f"{k}={v:.4f}" for k, v in med.items()), flush=True)
    print("min    ms/step:", " ".join(f"{k}={min(v):.4f}" for k, v in times.items()), flush=True)
    for new, old in (("joint_adam", "joint"), ("joint_depth_adam", "joint_depth"), ("graphed_train_pose", "joint"), ("graphed_train_pose", "graphed_then_pose")):
        print(f"{new} against {old}: {med[new] - med[old]:+.4f} ms/step ({med[new] / med[old]:.4f}x)", flush=True)
    print("steps that did not fit:", g_joint.check(), g_plain.check(), " row 0 after the run: steps", ps.steps.tolist(), flush=True)


def driver(log, argv):
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "steps"] + argv
    os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
    with open(log, "a") as f:
        f.write(f"== steps: python {os.path.relpath(cmd[1], ROOT)} {' '.join(cmd[2:])}\n"); f.flush()
        r = subprocess.run(["timeout", "-k", "10", str(pose_probe.LIMIT)] + cmd, stdout=f, stderr=subprocess.PIPE, text=True, cwd=ROOT)
        if r.returncode != 0:   # (as pose_probe's driver: the child's stderr is kept only when it failed)
            f.write(r.stderr)
        f.write(f"== steps: exit status {r.returncode}\n")
    print("steps exit status", r.returncode, flush=True)
    return r.returncode


if __name__ == "__main__":
    leg, log, argv, sizes = pose_probe._args()
    if leg is None:
        sys.exit(driver(log if "--log" in sys.argv else os.path.join(ROOT, "profiles", "pose_adam_config3.log"), argv))
    leg_steps(*sizes)
