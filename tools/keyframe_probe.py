#!/usr/bin/env python
"""Timing probe: the keyframe store's decode launch (gslic_keyframe_decode) at 1920 x 1080, pyramid levels 0-2, against what it replaces.  Without
arguments it is a driver that holds no GPU itself: it runs its one measurement leg as ONE child process under a time limit and appends everything
it prints to the log.  The leg times, per level, all paths in one process, in alternating rounds, with device events (ms per call, median of the
rounds):
  decode    trainer.KeyframeStore.target(slot, level, out=...) cycling over the slots of an 8-slot store with masks off
  copy      the device-to-device copy of the float target it replaces in GraphedStep (gt.copy_ of a [3,H_l,W_l] float image)
  torch     the same bytes through torch: permute, float, mul by 1/255 and, above level 0, avg_pool2d(2^l)
  h2d_page  the upload of the float target from pageable host memory (what the reference does at every step: gaussian.cpp:678)
  h2d_pin   ... from pinned host memory
Each is reported as time and as GB/s against the bytes the RULE moves at that level: (3 * 4^l + 12) bytes per output pixel.  These are times
per call as a Python host issues them back to back; the decode kernel alone is timed once more by the library's per-kernel events.  The leg exits with
status 1 when the decode is slower than the torch route at any level.
    python tools/keyframe_probe.py [--log profiles/keyframes_config3.log] [W H rounds calls_per_round]
    python tools/keyframe_probe.py --leg decode [W H rounds calls_per_round]      (what the driver starts)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 300   # seconds for the leg
SLOTS = 8


def _args():
    argv, leg, log = list(sys.argv[1:]), None, os.path.join(ROOT, "profiles", "keyframes_config3.log")
    if "--leg" in argv:
        i = argv.index("--leg"); leg = argv[i + 1]; del argv[i:i + 2]
    if "--log" in argv:
        i = argv.index("--log"); log = argv[i + 1]; del argv[i:i + 2]
    return leg, log, argv, [int(v) for v in (argv[:4] + ["1920", "1080", "5", "40"][len(argv):])]


def driver(log, argv):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "decode"] + argv
    os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
    with open(log, "a") as f:
        f.write(f"== decode: python {os.path.relpath(cmd[1], ROOT)} {' '.join(cmd[2:])}\n"); f.flush()
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT)] + cmd, stdout=f, stderr=subprocess.STDOUT, cwd=ROOT)
        f.write(f"== decode: exit status {r.returncode}\n")
    print("decode exit status", r.returncode, flush=True)
    return r.returncode


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


def leg_decode(W, H, ROUNDS, N):
    import torch
    sys.path.insert(0, ROOT)
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib, trainer
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    st = trainer.KeyframeStore(W, H, SLOTS, dev)
    for _ in range(SLOTS):
        st.add_u8(torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8))
    print(f"W={W} H={H} slots={SLOTS} ({st.nbytes / 1e6:.1f} MB of slabs) rounds={ROUNDS} calls/round={N}", flush=True)
    lost = False
    for level in (0, 1, 2):
        Wl, Hl = st.level_size(level)
        out = st.target_buffers(level)[0]
        src = [st.target(s, level) for s in range(2)]                       # float targets on the device: what gt.copy_ reads
        host = src[0].cpu()
        pinned = host.pin_memory()
        gt = torch.empty_like(out)
        n = 1 << level

        def torch_route(i):
            x = st.color[i % SLOTS].permute(2, 0, 1).float().mul(1.0 / 255.0)
            return x if level == 0 else torch.nn.functional.avg_pool2d(x[None], n)[0]

        # the torch route computes the same image up to rounding (it divides where the rule multiplies once): a sanity check, not a bit test
        assert float((torch_route(1) - st.target(1, level)).abs().max()) < 1e-6
        paths = {
            "decode": lambda i: st.target(i % SLOTS, level, out=out),
            "copy": lambda i: gt.copy_(src[i % 2]),
            "torch": torch_route,
            "h2d_page": lambda i: gt.copy_(host),
            "h2d_pin": lambda i: gt.copy_(pinned, non_blocking=True),
        }
        calls = {k: (N if not k.startswith("h2d") else max(4, N // 4)) for k in paths}
        moved = (3 * 4 ** level + 12) * Wl * Hl
        print(f"level {level}: {Wl} x {Hl}, the rule moves {moved / 1e6:.2f} MB per call ({3 * 4 ** level} B read + 12 B written per output pixel); "
              f"the float target is {12 * Wl * Hl / 1e6:.2f} MB", flush=True)
        for k, fn in paths.items():
            clock_ev(fn, 5)
        times = {k: [] for k in paths}
        for r in range(ROUNDS):
            for k, fn in paths.items():
                times[k].append(clock_ev(fn, calls[k]))
            print(f"level {level} round {r}", " ".join(f"{k}={v[-1]:.4f}" for k, v in times.items()), flush=True)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        print(f"level {level} median ms/call:", " ".join(f"{k}={v:.4f}" for k, v in med.items()), flush=True)
        print(f"level {level} min    ms/call:", " ".join(f"{k}={min(v):.4f}" for k, v in times.items()), flush=True)
        print(f"level {level} GB/s against the rule's {moved / 1e6:.2f} MB (back-to-back calls; the 256 MB last-level cache can hold the slabs):",
              " ".join(f"{k}={moved / (v * 1e-3) / 1e9:.1f}" for k, v in med.items()), flush=True)
        # the launch alone, by the library's own per-kernel events (the figures above include what the Python host spends issuing a call)
        _lib.profile_enable(True, only=["gather_rows"])
        _lib.profile_reset()
        for i in range(N):
            paths["decode"](i)
        ms, launches = _lib.profile_collect()["gather_rows"]
        _lib.profile_enable(False)
        print(f"level {level}: the decode kernel alone (events around each of {launches} launches): {1e3 * ms / launches:.2f} us per launch, "
              f"{moved / (ms / launches * 1e-3) / 1e9:.1f} GB/s against the rule's bytes", flush=True)
        verdict = "faster than" if med["decode"] <= med["torch"] else "SLOWER than"
        print(f"level {level}: decode is {verdict} the torch route ({med['torch'] / med['decode']:.2f}x)", flush=True)
        lost = lost or med["decode"] > med["torch"]
    return 1 if lost else 0


if __name__ == "__main__":
    leg, log, argv, sizes = _args()
    if leg is None:
        sys.exit(driver(log, argv))
    sys.exit(leg_decode(*sizes))
