#!/usr/bin/env python
"""Timing probe: the per-view exposure on the single-GPU step at config 3 (2M Gaussians, 1920 x 1080, SH 3, Morton row order, learning rates
scaled by 0.01 as bench.py does).  Without arguments it is a driver that holds no GPU itself: it runs its measurement steps one after the other,
each as ONE child process under a time limit of its own, stops at the first one that fails, and appends everything they print to the log:
  hbm       tools/ubench/hbm_rate, when it is built (the practical stream rates the kernels are held against)
  steps     GraphedStep (eager capacity-mode step and captured graph) with and without an exposure, in alternating rounds: wall clock between two
            device synchronisations, ms per step, median of the rounds
  kernels   gslic_exposure_apply and gslic_exposure_backward alone on a 3 x H x W image (device events, ms per call, median of the rounds) and
            their achieved bytes per second: 24 and 36 bytes per pixel
    python tools/exposure_probe.py [--log profiles/exposure_config3.log] [P W H rounds steps_per_round]
    python tools/exposure_probe.py --leg steps|kernels [P W H rounds steps_per_round]      (what the driver starts)"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = {"hbm": 90, "steps": 420, "kernels": 180}   # seconds per step (the steps leg builds a 2M-Gaussian model and four GraphedSteps)


def _args():
    argv, leg, log = list(sys.argv[1:]), None, os.path.join(ROOT, "profiles", "exposure_config3.log")
    if "--leg" in argv:
        i = argv.index("--leg"); leg = argv[i + 1]; del argv[i:i + 2]
    if "--log" in argv:
        i = argv.index("--log"); log = argv[i + 1]; del argv[i:i + 2]
    return leg, log, argv, [int(v) for v in (argv[:5] + ["2000000", "1920", "1080", "7", "20"][len(argv):])]


def driver(log, argv):
    steps = []
    hbm = os.path.join(ROOT, "tools", "ubench", "hbm_rate")
    if os.path.exists(hbm):
        steps.append(("hbm", [hbm]))
    steps += [(leg, [sys.executable, os.path.abspath(__file__), "--leg", leg] + argv) for leg in ("steps", "kernels")]
    os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
    with open(log, "a") as f:
        for name, cmd in steps:
            shown = ["python" if c == sys.executable else os.path.relpath(c, ROOT) if os.path.isabs(c) else c for c in cmd]
            f.write(f"== {name}: {' '.join(shown)}\n"); f.flush()
            r = subprocess.run(["timeout", "-k", "10", str(LIMITS[name])] + cmd, stdout=f, stderr=subprocess.STDOUT, cwd=ROOT)
            f.write(f"== {name}: exit status {r.returncode}\n"); f.flush()
            print(name, "exit status", r.returncode, flush=True)
            if r.returncode != 0:   # a fault, an abort or a time limit: nothing more is started on the device
                return r.returncode
    return 0


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


def report(times, unit):
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    print(f"median {unit}:", " ".join(f"{k}={v:.4f}" for k, v in med.items()), flush=True)
    print(f"min    {unit}:", " ".join(f"{k}={min(v):.4f}" for k, v in times.items()), flush=True)
    return med


def leg_steps(P, W, H, ROUNDS, N):
    import torch
    sys.path.insert(0, ROOT)
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import gt_image, random_scene
    dev = torch.device("cuda:0")
    raw = random_scene(P, W, H, 3, 0)
    model = trainer.GaussianModel(raw, dev, order="morton")
    model.training_setup({k: v * 0.01 for k, v in trainer.DEFAULT_LRS.items()})
    cam = synthetic_camera(W, H).to_device(dev)
    gt = gt_image(H, W, seed=2).to(dev)
    bg = torch.zeros(3, device=dev)
    ex = trainer.Exposure(2, dev, lr=0.001)
    print(f"P={P} W={W} H={H} rounds={ROUNDS} steps/round={N}", flush=True)
    variants = {}
    for graph in (False, True):
        tag = "graph" if graph else "eager"
        plain = trainer.GraphedStep(model, cam, gt, bg, use_graph=graph, check_every=0)
        withex = trainer.GraphedStep(model, cam, gt, bg, use_graph=graph, check_every=0, exposure=ex, view=0)
        variants[tag] = plain.step
        variants[tag + "_exposure"] = lambda s=withex: s.step(view=0)
    for fn in variants.values():
        clock(fn, 5)
    times = {k: [] for k in variants}
    for r in range(ROUNDS):
        for name, fn in variants.items():
            times[name].append(clock(fn, N))
        print("round", r, " ".join(f"{k}={v[-1]:.4f}" for k, v in times.items()), flush=True)
    med = report(times, "ms/step")
    for tag in ("eager", "graph"):
        print(f"{tag}: exposure adds {med[tag + '_exposure'] - med[tag]:+.4f} ms/step ({med[tag + '_exposure'] / med[tag]:.4f}x)", flush=True)
    print("E after the run:", [round(v, 5) for v in ex.matrix(0).flatten().tolist()], "steps", ex.steps.tolist(), flush=True)


def leg_kernels(P, W, H, ROUNDS, N):
    import torch
    sys.path.insert(0, ROOT)
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib, loss, trainer
    from gaussian_lic_amd.synthetic import gt_image
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    img = gt_image(H, W, seed=2).to(dev)
    dL = (1e-6 * torch.randn(3, H, W, generator=g)).to(dev)
    ex = trainer.Exposure(2, dev, lr=0.0)
    out, dimg, dE = torch.empty_like(img), torch.empty_like(img), torch.empty(12, device=dev)
    partials = torch.empty(int(_lib.lib().gslic_exposure_partials_count(H, W)), device=dev)
    adam = ex._descriptor(ex._views[0:1])
    calls = {
        "apply": lambda: loss.exposure_apply(img, ex.params[0], out),
        "backward": lambda: loss.exposure_backward(img, ex.params[0], dL, dimg, partials, dE),
        "backward_adam": lambda: loss.exposure_backward(img, ex.params[0], dL, dimg, partials, dE, adam),
    }
    nbytes = {"apply": 24 * H * W, "backward": 36 * H * W, "backward_adam": 36 * H * W}
    print(f"W={W} H={H} rounds={ROUNDS} calls/round={10 * N}: apply moves {nbytes['apply'] / 1e6:.1f} MB, backward {nbytes['backward'] / 1e6:.1f} MB per call", flush=True)
    for fn in calls.values():
        clock_ev(fn, 20)
    times = {k: [] for k in calls}
    for r in range(ROUNDS):
        for name, fn in calls.items():
            times[name].append(clock_ev(fn, 10 * N))
        print("round", r, " ".join(f"{k}={v[-1]:.4f}" for k, v in times.items()), flush=True)
    med = report(times, "ms/call")
    print("achieved TB/s (algorithmic bytes over the median; back-to-back calls on one image, which the 256 MB last-level cache can hold):",
          " ".join(f"{k}={nbytes[k] / (med[k] * 1e-3) / 1e12:.3f}" for k in calls), flush=True)


if __name__ == "__main__":
    leg, log, argv, sizes = _args()
    if leg is None:
        sys.exit(driver(log, argv))
    {"steps": leg_steps, "kernels": leg_kernels}[leg](*sizes)
