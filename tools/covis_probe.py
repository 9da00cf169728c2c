#!/usr/bin/env python
"""Timing probe of the covisibility sets (gslic_covis_*, trainer.Covisibility), modelled on tools/pose_shared_probe.py.  Without arguments it is a
driver that holds no GPU itself: it runs the measurement as ONE child process under a time limit and appends what it prints to the log (its stderr
only when it failed).  The child measures at config 3 (2M Gaussians, 1920 x 1080, SH 3, Morton row order, learning rates scaled by 0.01 as
bench.py does), in one process and in alternating rounds, the median of five:
  record    gslic_covis_record alone (device events around back-to-back calls, microseconds per call) at F = 32 and F = 128, against the bytes
            the rule moves: per row 4 of radii and one word loaded and stored, 12 P bytes whatever F is
  steps     GraphedStep on a 3-slot keyframe store with and without covis= (wall clock between two device synchronisations, ms per step), the
            difference next to the round-to-round spread
  queries   pair_counts, frame_counts, seen_count and redundant (device events, microseconds per call) on bits recorded from 32 and from 128
            synthetic views of the scene (yaw -14 .. 14 degrees, x -0.9 .. 0.9 m), with the share of set bits
    python tools/covis_probe.py [--log profiles/covis_config3.log] [P W H rounds steps_per_round]
    python tools/covis_probe.py --leg steps [P W H rounds steps_per_round]      (what the driver starts)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pose_probe import clock, clock_ev   # noqa: E402  (the two clocks of the pose probes)

LIMIT = 540   # seconds (the leg builds a 2M-Gaussian model and renders 128 views)


def _args():
    argv, leg, log = list(sys.argv[1:]), None, os.path.join(ROOT, "profiles", "covis_config3.log")
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
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import gt_image, random_scene
    dev = torch.device("cuda:0")
    print(f"P={P} W={W} H={H} rounds={ROUNDS} steps/round={N}", flush=True)
    median = lambda v: sorted(v)[len(v) // 2]
    model = trainer.GaussianModel(random_scene(P, W, H, 3, 0), dev, order="morton")
    model.training_setup({k: v * 0.01 for k, v in trainer.DEFAULT_LRS.items()})
    bg = torch.zeros(3, device=dev)
    cam = synthetic_camera(W, H).to_device(dev)

    def radii_of(camera):
        rr = trainer._RawRaster(model, camera, bg)
        with torch.no_grad():
            rr.forward()
        return rr.state[2]
    # ---- the record launch alone
    radii = radii_of(cam)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    sets = {F: trainer.Covisibility(model, F) for F in (32, 128)}
    calls = {f"record_F{F}": (lambda cv: lambda: cv._record(word, radii=radii))(cv) for F, cv in sets.items()}
    for fn in calls.values():
        clock_ev(fn, 50)
    times = {k: [] for k in calls}
    for r in range(ROUNDS):
        for name, fn in calls.items():
            times[name].append(1e3 * clock_ev(fn, 10 * N))
        print("record round", r, " ".join(f"{k}={v[-1]:.2f}" for k, v in times.items()), "us/call", flush=True)
    print("record median us/call:", " ".join(f"{k}={median(v):.2f}" for k, v in times.items()), flush=True)
    print("record spread us/call (max - min over the rounds):", " ".join(f"{k}={max(v) - min(v):.2f}" for k, v in times.items()), flush=True)
    for k, v in times.items():
        print(f"{k}: the rule moves {12 * P / 1e6:.1f} MB per call: {12 * P / median(v) / 1e6:.2f} TB/s as issued from Python", flush=True)
    # ---- the queries, on bits recorded from 32 and from 128 synthetic views
    for F, cv in sets.items():
        for f in range(F):
            t = f / (F - 1) - 0.5
            cv.record(f, radii_of(synthetic_camera(W, H, dict(ypr=(28.0 * t, 0.0, 0.0), t=(1.8 * t, 0.0, 0.0))).to_device(dev)))
        share = float(cv.seen_count().double().mean()) / F
        queries = {"pair_counts": cv.pair_counts, "frame_counts": lambda cv=cv, F=F: cv.frame_counts(F // 2), "seen_count": cv.seen_count,
                   "redundant": lambda cv=cv: cv.redundant(2)}
        for fn in queries.values():
            clock_ev(fn, 5)
        times = {k: [] for k in queries}
        for r in range(ROUNDS):
            for name, fn in queries.items():
                times[name].append(1e3 * clock_ev(fn, N))
        print(f"queries F={F} (share of set bits {share:.3f}, {4 * cv.words * P / 1e6:.1f} MB of bits) median us/call:",
              " ".join(f"{k}={median(v):.1f}" for k, v in times.items()), flush=True)
        print(f"queries F={F} spread us/call (max - min over the rounds):", " ".join(f"{k}={max(v) - min(v):.1f}" for k, v in times.items()), flush=True)
    # ---- the step on a keyframe store, with and without the record launch
    store = trainer.KeyframeStore(W, H, 3, dev)
    for s in range(3):
        store.add(gt_image(H, W, seed=2 + s).to(dev))
    cv = trainer.Covisibility(model, 128)
    steps = {"plain": trainer.GraphedStep(model, cam, None, bg, keyframes=store, frame=0, check_every=0),
             "covis": trainer.GraphedStep(model, cam, None, bg, keyframes=store, frame=0, check_every=0, covis=cv)}
    count = [0]

    def run(g):
        count[0] += 1
        g.step(frame=count[0] % 3)
    for g in steps.values():
        clock(lambda: run(g), 5)
        assert g.check() == 0
    times = {k: [] for k in steps}
    for r in range(ROUNDS):
        for name, g in steps.items():
            times[name].append(clock(lambda: run(g), N))
            assert g.check() == 0
        print("steps round", r, " ".join(f"{k}={v[-1]:.4f}" for k, v in times.items()), flush=True)
    med = {k: median(v) for k, v in times.items()}
    print("median ms/step:", " ".join(f"{k}={v:.4f}" for k, v in med.items()), flush=True)
    print("spread ms/step (max - min over the rounds):", " ".join(f"{k}={max(v) - min(v):.4f}" for k, v in times.items()), flush=True)
    print(f"covis against plain: {1e3 * (med['covis'] - med['plain']):+.1f} us/step ({med['covis'] / med['plain']:.4f}x)", flush=True)
    print("rows recorded per slot:", [int(cv.rows_of(s).sum()) for s in range(3)], flush=True)


if __name__ == "__main__":
    leg, log, argv, sizes = _args()
    if leg is None:
        sys.exit(driver(log, argv))
    leg_steps(*sizes)
