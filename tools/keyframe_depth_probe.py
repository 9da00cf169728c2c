#!/usr/bin/env python
"""Timing probe: the keyframe store's depth decode launch (gslic_keyframe_decode_depth) at 1920 x 1080, pyramid levels 0-2, with and without depth
weights, against what it replaces — and the config-3 depth-supervised GraphedStep on the store against the same step fed device tensors.  Without
arguments it is a driver that holds no GPU itself: it runs its two measurement legs, each as ONE child process under a time limit, and appends
everything they print to the log.  Both legs time all their paths in one process, in alternating rounds (median of the rounds).
  leg decode (device events, ms per call as a Python host issues them back to back), per level, without (d) and with (dw) depth weights:
    decode    trainer.KeyframeStore.depth_target(slot, level, out=...) cycling over the slots of an 8-slot store
    copy      the device-to-device copy_ of the float32 depth (+ weight) image(s) it replaces in GraphedStep
    h2d_page  the upload of the same image(s) from pageable host memory
    h2d_pin   ... from pinned host memory
    each also as GB/s against the bytes the RULE moves: (2 * 4^l + 4) bytes per output pixel, (3 * 4^l + 8) with weights; the decode kernel alone
    is timed once more by the library's per-kernel events
  leg step (wall clock, ms per step), config 3 (2M Gaussians, SH 3, Morton order), depth weights on, the frame changing every step, both steps
  in the default eager capacity mode (the host synchronises between rounds):
    store     GraphedStep(keyframes=store, frame=, lambda_depth=).step(frame=j)
    tensors   GraphedStep(gt_depth=, depth_weight=, lambda_depth=).step(gt_image, gt_depth=, depth_weight=) from device tensors
  and the bytes per keyframe: 3 B per pixel (codes + weight) against 8 B (two float32 images).
    python tools/keyframe_depth_probe.py [--log profiles/keyframe_depth_config3.log] [W H rounds calls_per_round]
    python tools/keyframe_depth_probe.py --leg decode|step [W H rounds calls_per_round]      (what the driver starts)"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 300   # seconds per leg
SLOTS = 8
LAMBDA_D = 0.1


def _args():
    argv, leg, log = list(sys.argv[1:]), None, os.path.join(ROOT, "profiles", "keyframe_depth_config3.log")
    if "--leg" in argv:
        i = argv.index("--leg"); leg = argv[i + 1]; del argv[i:i + 2]
    if "--log" in argv:
        i = argv.index("--log"); log = argv[i + 1]; del argv[i:i + 2]
    return leg, log, argv, [int(v) for v in (argv[:4] + ["1920", "1080", "5", "40"][len(argv):])]


def driver(log, argv):
    os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
    worst = 0
    for leg in ("decode", "step"):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg] + argv
        with open(log, "a") as f:
            f.write(f"== {leg}: python {os.path.relpath(cmd[1], ROOT)} {' '.join(cmd[2:])}\n"); f.flush()
            r = subprocess.run(["timeout", "-k", "10", str(LIMIT)] + cmd, stdout=f, stderr=subprocess.STDOUT, cwd=ROOT)
            f.write(f"== {leg}: exit status {r.returncode}\n")
        print(leg, "exit status", r.returncode, flush=True)
        worst = worst or r.returncode
        if r.returncode != 0:   # a leg that failed: nothing more is started on the device
            break
    return worst


def clock_ev(fn, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def _lidar_like(W, H, g):
    """A float depth image with about a third of its pixels measured (0.5 .. 60 m) and a weight image in [0, 1]."""
    import torch
    d = torch.rand(H, W, generator=g) * 59.5 + 0.5
    d[torch.rand(H, W, generator=g) > 0.35] = 0.0
    return d, torch.rand(H, W, generator=g)


def leg_decode(W, H, ROUNDS, N):
    import torch
    sys.path.insert(0, ROOT)
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib, trainer
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    zero = torch.zeros(H, W, 3, dtype=torch.uint8)
    print(f"W={W} H={H} slots={SLOTS} rounds={ROUNDS} calls/round={N}", flush=True)
    for weights in (False, True):
        tag = "dw" if weights else "d"
        st = trainer.KeyframeStore(W, H, SLOTS, dev, depths=True, depth_weights=weights)
        for _ in range(SLOTS):
            d, w = _lidar_like(W, H, g)
            st.add_u8(zero, depth=d, depth_weight=w if weights else None)
        print(f"{tag}: {(st.nbytes - st.color.numel()) / SLOTS / (W * H):.0f} B per pixel and keyframe in the depth slabs, against "
              f"{8 if weights else 4} B as float32", flush=True)
        for level in (0, 1, 2):
            Wl, Hl = st.level_size(level)
            out = st.depth_target_buffers(level)
            out = out if weights else out[0]
            as_list = lambda t: list(t) if weights else [t]
            src = [as_list(st.depth_target(s, level)) for s in range(2)]        # float images on the device: what copy_ reads
            host = [t.cpu() for t in src[0]]
            pinned = [t.pin_memory() for t in host]
            dst = [torch.empty_like(t) for t in src[0]]

            def copies(srcs, **kw):
                for a, b in zip(dst, srcs):
                    a.copy_(b, **kw)

            paths = {
                "decode": lambda i: st.depth_target(i % SLOTS, level, out=out),
                "copy": lambda i: copies(src[i % 2]),
                "h2d_page": lambda i: copies(host),
                "h2d_pin": lambda i: copies(pinned, non_blocking=True),
            }
            calls = {k: (N if not k.startswith("h2d") else max(4, N // 4)) for k in paths}
            per_px = ((3 if weights else 2) * 4 ** level, 8 if weights else 4)
            moved = sum(per_px) * Wl * Hl
            print(f"{tag} level {level}: {Wl} x {Hl}, the rule moves {moved / 1e6:.2f} MB per call ({per_px[0]} B read + {per_px[1]} B written per output "
                  f"pixel); the float image(s) are {per_px[1] * Wl * Hl / 1e6:.2f} MB", flush=True)
            for k, fn in paths.items():
                clock_ev(fn, 5)
            times = {k: [] for k in paths}
            for r in range(ROUNDS):
                for k, fn in paths.items():
                    times[k].append(clock_ev(fn, calls[k]))
                print(f"{tag} level {level} round {r}", " ".join(f"{k}={v[-1]:.4f}" for k, v in times.items()), flush=True)
            med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
            print(f"{tag} level {level} median ms/call:", " ".join(f"{k}={v:.4f}" for k, v in med.items()), flush=True)
            print(f"{tag} level {level} min    ms/call:", " ".join(f"{k}={min(v):.4f}" for k, v in times.items()), flush=True)
            print(f"{tag} level {level} GB/s against the rule's {moved / 1e6:.2f} MB (back-to-back calls; the 256 MB last-level cache can hold the slabs):",
                  " ".join(f"{k}={moved / (v * 1e-3) / 1e9:.1f}" for k, v in med.items()), flush=True)
            _lib.profile_enable(True, only=["gather_rows"])
            _lib.profile_reset()
            for i in range(N):
                paths["decode"](i)
            ms, launches = _lib.profile_collect()["gather_rows"]
            _lib.profile_enable(False)
            print(f"{tag} level {level}: the decode kernel alone (events around each of {launches} launches): {1e3 * ms / launches:.2f} us per launch, "
                  f"{moved / (ms / launches * 1e-3) / 1e9:.1f} GB/s against the rule's bytes", flush=True)
    return 0


def leg_step(W, H, ROUNDS, N, P=2000000):
    import torch
    sys.path.insert(0, ROOT)
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import gt_image, random_scene
    from gaussian_lic_amd.trainer import DEFAULT_LRS
    N = max(4, N // 2)
    dev = torch.device("cuda:0")
    raw = random_scene(P, W, H, 3, 0)
    cam = synthetic_camera(W, H).to_device(dev)
    bg = torch.zeros(3, device=dev)
    st = trainer.KeyframeStore(W, H, 4, dev, depths=True, depth_weights=True)
    g = torch.Generator().manual_seed(1)
    for s in range(4):
        gtd = cam.project_depth(raw["xyz"][s::20].to(dev) * 1.05)
        st.add(gt_image(H, W, seed=2 + s).to(dev), depth=gtd, depth_weight=torch.rand(H, W, generator=g))
    targets = [(st.target(s), *st.depth_target(s)) for s in range(4)]
    print(f"P={P} W={W} H={H} lambda_depth={LAMBDA_D} measured_pixels={int((targets[0][1] > 0).sum())} rounds={ROUNDS} steps/round={N}; per keyframe "
          f"{st.nbytes / 4 / 1e6:.1f} MB in the store ({(st.depth.numel() * 2 + st.dweight.numel()) / 4 / 1e6:.1f} MB of it depth: 3 B per pixel) "
          f"against {8 * W * H / 1e6:.1f} MB of float32 depth and weight", flush=True)

    def model():
        m = trainer.GaussianModel(raw, dev, order="morton")
        m.training_setup({k: v * 0.01 for k, v in DEFAULT_LRS.items()})
        return m

    on_store = trainer.GraphedStep(model(), cam, None, bg, keyframes=st, frame=0, lambda_depth=LAMBDA_D)
    on_tensors = trainer.GraphedStep(model(), cam, targets[0][0], bg, gt_depth=targets[0][1], depth_weight=targets[0][2], lambda_depth=LAMBDA_D)
    count = [0]

    def store_step():
        count[0] += 1
        on_store.step(frame=count[0] % 4)

    def tensor_step():
        count[0] += 1
        t = targets[count[0] % 4]
        on_tensors.step(gt_image=t[0], gt_depth=t[1], depth_weight=t[2])

    variants = {"store": store_step, "tensors": tensor_step}

    def clock(fn, n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t) / n

    for fn in variants.values():
        clock(fn, 4)
    on_store.check(); on_tensors.check()
    times = {k: [] for k in variants}
    for r in range(ROUNDS):
        for k, fn in variants.items():
            times[k].append(clock(fn, N))
        on_store.check(); on_tensors.check()
        print("step round", r, " ".join(f"{k}={v[-1]:.4f}" for k, v in times.items()), flush=True)
    print("step median ms/step:", " ".join(f"{k}={sorted(v)[len(v) // 2]:.4f}" for k, v in times.items()), flush=True)
    print("step min    ms/step:", " ".join(f"{k}={min(v):.4f}" for k, v in times.items()), flush=True)
    return 0


if __name__ == "__main__":
    leg, log, argv, sizes = _args()
    if leg is None:
        sys.exit(driver(log, argv))
    sys.exit(leg_decode(*sizes) if leg == "decode" else leg_step(*sizes))
