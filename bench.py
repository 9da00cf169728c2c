#!/usr/bin/env python
"""bench.py — throughput of the hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

Both forms work for N > 1: without WORLD_SIZE in the environment `--gpus N` spawns the N ranks itself (torch.distributed.run on 127.0.0.1).

A "step" = one iteration of the reference's optimize() loop (src/gaussian.cpp:674-716) on one camera view:
render forward -> 0.8*L1 + 0.2*(1-SSIM) -> backward -> visibility-masked Adam, at BASELINE.json config 3
(2M Gaussians, 1920x1080, SH degree 3).  N > 1: one rank per GPU, each rank renders a different view of the same
replica and the ranks meet in ONE exchange step per optimiser step (default: an all-gather of the colour gradients +
masks and two all-reduces of the small gradients; "weak" scaling: views per step = N).
value = views (fwd+bwd) per second over the whole job.

A plain run sets up, warms up (W untimed steps), times exactly K steps with nothing else on the device, writes the outputs of the last
timed step when `--dump-outputs DIR` is given, and prints ONE JSON line: `metric`, `value`, `unit`, `higher_is_better`, `dtype`,
`ms_per_step` (wall time of one timed step) and the workload in `config`.  At N > 1 the line also carries `rccl_ranks` (ranks a real
all-reduce reached), `per_rank_ms_per_step`, `exchange` and `launch`.

`--full` measures everything beside the headline as well: `roofline` (the two longest kernels of an instrumented warm-up pass, HIP-event timed
inside the timed region), `cpu_baseline` (the CPU oracle, N=1 only), `value_long` (the same step over a >= 1 s window) and, at N > 1,
`rccl_microbench` (the step's collectives alone at the step's sizes) and a per-kernel roofline.  At N = 1 it then runs SURVEY 8d's literal
config-3 schedule (1.5M -> 2.0M Gaussians by five extend() appends, the reference's learning rates) in a SECOND process and puts it into
`config.growth_schedule` beside the stationary line, and a THIRD process measures the reference's unmodified host on the drop-in boundary
(`dropin_host`, `config.dropin_host`); `--no-extras` runs neither.  `--extras` adds the secondary legs (views_cycle, math_modes,
other_host_path, graphed, joint_pose_step, C++ hosts) the same way.  The legs themselves live in bench_legs.py; this file is the contract line.

`--dump-outputs DIR` writes what the timed path handed its caller after the last timed step as `DIR/<name>.npy` (dump_outputs()).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # multi-process GPU work on this driver needs dmabuf IPC (already exported on the GPU boxes)

import numpy as np
import torch

HBM_PEAK_GBS = 8000.0       # MI355X spec, /opt/skills/guides/MI355X_MICROARCH.md


def algorithmic_bytes(kernel, s):
    """Algorithmic HBM bytes of ONE launch of `kernel` (per-unit figures of DESIGN.md §4 x this run's unit counts).
    s: P, V, R, B (64-entry buckets), N (pixels), T (tiles), K (SH coefficients incl. DC), Npad = T*256."""
    P, V, R, B, N, T, K, Np = s["P"], s["V"], s["R"], s["B"], s["N"], s["T"], s["K"], s["T"] * 256
    Rl, Bl = s.get("R_live", R), s.get("B_live", B)   # instances / buckets in front of their tile's last contributor (the others are skipped)
    hb = 2048 if s.get("strict", True) else 0          # recorded blend decisions: 8 B x 64 entries x 4 strips per bucket (strict mode)
    table = {
        # in: xyz 12 + scale 12 + rot 16 + opacity 4 per P; out: radii 4 + tiles 4 per P; per visible: SH 12K in, 48 B record out
        "preprocess": 52 * P + V * (12 * K + 48),
        # per Gaussian: offset 4; per visible: record 48 in, start 4 out; per instance: tile 4 + gaussian id 4 + depth bits 4 out
        "keybuild": 4 * P + 52 * V + 12 * R,
        "sort_hist": 4 * R,                       # tile keys once per pass
        "sort_scatter": 32 * R,                   # key + slot + gaussian id + depth bits in and out, per pass (the first pass reads no slot: 28)
        # per-tile depth sort: depth 4 + gaussian id 4 + slot 4 in, gaussian id 4 + slot 4 out per instance; ranges 8 per tile
        "tile_lsort": 20 * R + 8 * T,
        "finalize_lists": 4 * R + 8 * T,          # sorted tile ids in, ranges out
        # grouping by tile without a sort (tile_bin.hip): the histogram reads the tile ids and the single-workgroup scan turns the counts into ranges;
        # the binning reads tile, Gaussian id, depth bits (12) and writes one 16-byte row + the cleared dead flag (1) per instance.  The per-tile
        # sort then reads rows (16) instead of three arrays (12): + 4 R on "tile_lsort", not itemised
        "tile_hist": 4 * R + 8 * T,
        "tile_scan": 24 * T,                      # counts in; ranges, bucket offsets and the zeroed max_contrib out
        "tile_bin": 29 * R,
        # list 4 + record 48 per instance of a live bucket; checkpoints 4096 (+ decision masks) per live bucket; pix_final 16/px(padded), image 16/px
        "render_fwd": 52 * Rl + (4096 + hb) * Bl + 16 * Np + 16 * N,
        # live buckets: checkpoints 4096 (+ masks), list 4 + slot 4 + record 48 in, partial row 36 out per instance; dead buckets: slot 4 in,
        # flag 1 out per instance; pixel data once: 16 + 12 per px
        "render_bwd": (4096 + hb) * Bl + 92 * Rl + 5 * (R - Rl) + 16 * Np + 12 * N,
        # partial rows 36/live instance + flag 1/instance; per P radii 4; per visible in: xyz 12 scale 12 rot 16 SH 12K rec 16 off 8; out: the gradients
        "preprocess_bwd": 36 * Rl + R + 4 * P + V * (12 * K + 64) + P * 4 * (3 + 4 + 1 + 3 + 3 + 6 + 3 * K + 3 + 4),
        # the same kernel with Adam applied in place (fused host path, single GPU): no gradient tensors; per visible Gaussian the
        # 59 scalars' param/m/v are read and written (24 B/scalar), SH and the record are read once
        "preprocess_bwd+adam": 36 * Rl + R + 12 * P + V * (16 + 24 * (11 + 3 * K)),
        # visible rows: param, grad, m, v in; param, m, v out (28 B/scalar); mask byte per scalar-thread
        "adam": 28 * (11 + 3 * K - 3) * V + (11 + 3 * K - 3) * P,
        "ssim_fwd": 24 * N + 48 * N,
        "ssim_bwd": 72 * N + 12 * N,
        # ---- the N > 1 compute leg (rank-1 exchange); nv = views whose colour gradients a rank rebuilds from, Vu = rows some view sees
        # per Gaussian: nv x 12 B dRGB + 12 B mean + 1 B mask in; per row some view sees: features_dc + features_rest (48 scalars) param / m / v read and written
        "sh_grad_from_rgb": P * (12 * s.get("nv", 1) + 13) + s.get("Vu", V) * 24 * 3 * K,
        # Adam on the four small groups (xyz, opacity, scaling, rotation: 11 scalars) of the rows some view sees, mask byte per scalar-thread
        "adam_small": 28 * 11 * s.get("Vu", V) + 11 * P,
    }
    return float(table.get(kernel, 0))


def a_view_bytes(s):
    """SURVEY.md section 8d's algorithmic bytes of ONE view (forward + backward + Adam + loss), evaluated at this run's unit counts.  The SURVEY's
    bucket is the reference's 32-entry one (B32 = sum over tiles of ceil(n_t / 32)); each logical array is counted once per stage that must touch
    it, the sort as one read + one write.  roofline.step divides it by ms_per_step: the whole step's fraction of the 8 TB/s HBM peak."""
    P, V, R, N, T, K, B32 = s["P"], s["V"], s["R"], s["N"], s["T"], s["K"], s.get("B32", 2 * s["B"])
    a_fwd = 52 * P + V * (12 * K + 67) + 8 * P + 36 * V + 12 * R + 24 * R + 8 * R + 24 * T + 40 * R + 4096 * B32 + 20 * N
    a_bwd = 4096 * B32 + 40 * R + 28 * N + 72 * R + 4 * P + V * (12 * K + 103) + V * (12 * K + 40)
    a_adam = 28 * (11 + 3 * K) * V + (11 + 3 * K) * P
    a_loss = 72 * N + 84 * N + 60 * N
    return {"A_fwd": float(a_fwd), "A_bwd": float(a_bwd), "A_adam": float(a_adam), "A_loss": float(a_loss), "A_view": float(a_fwd + a_bwd + a_adam + a_loss)}


# Modelled VALU issue cost of the blend kernels' instruction mix: (instructions of each class in the kernel's inner loop, from the ISA) x (cycles a
# wave64 instruction of that class occupies a SIMD's issue port, tools/ubench/issue_rate on gfx950: 2.3 plain VGPR operands, 4.1-4.2 DPP / packed /
# SGPR operand / v_bfe / v_bfi, 8.0 v_exp / v_rcp), averaged.  roofline.frac of a VALU-bound kernel = instructions issued x this / SIMD cycles.
VALU_CYCLES_PER_INST = {
    "render_bwd": 3.25,       # row-scan kernel (render_bwd_scan.hip): 43.5 per step = 10 DPP + 4 packed + 2 transcendental + 2 bfe / bfi + 25.5 plain
    "render_bwd_pipeline": 3.05,   # pipeline kernel (render.hip): 36 per step = 2 DPP + 7 packed + 2 transcendental + 2 bfe / bfi + 23 plain
    "render_fwd": 2.7,        # strict body: 36 per (entry, quadrant) = 1 transcendental + 3 SGPR-operand + 32 plain (+ SALU, not counted)
}
SHADER_CLOCK_GHZ = 2.0        # what the part sustains under this workload (2.4 nominal)




from bench_legs import _freeze_gc, _trace   # (shared with the leg processes: bench_legs.py)


def _free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: run ourselves under torch.distributed.run with N ranks on this node (rendezvous on
    127.0.0.1, a free port) — exactly the command the driver uses for N > 1 — and hand its exit code back.  Rank 0 of the child prints the line."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    print(f"[bench] --gpus {n} without WORLD_SIZE: launching {' '.join(cmd[1:8])} ...", file=sys.stderr, flush=True)
    env = dict(os.environ, GSLIC_BENCH_SELF_LAUNCHED="1")
    return subprocess.call(cmd, env=env)


def run_leg_process(leg, budget_s, args):
    """A secondary leg in a process of its own (`bench.py --leg NAME` with this run's size flags): the contract line's process measures the
    contract and nothing else.  Returns the leg's JSON dict, or {"error": ...}; a leg that overruns its budget is killed (its PID, nothing else)."""
    import subprocess
    keep = ["--gaussians", str(args.gaussians), "--width", str(args.width), "--height", str(args.height), "--scene", args.scene, "--lr-scale", repr(args.lr_scale),
            "--views", str(args.views), "--steps", str(args.steps), "--density", repr(args.density), "--opacity-shift", repr(args.opacity_shift), "--math", args.math, "--map-order", args.map_order]
    keep += ["--ply", args.ply] if args.ply else []
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--no-cpu-baseline"] + keep
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "GSLIC_FORCE_DIST")}
    t0 = time.perf_counter()
    try:
        pr = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=sys.stderr, text=True)
        try:
            so, _ = pr.communicate(timeout=budget_s)
        except subprocess.TimeoutExpired:
            pr.kill()
            pr.communicate()
            return {"error": f"leg '{leg}' stopped after its budget of {budget_s:.0f} s"}
        line = [l for l in so.splitlines() if l.startswith("{")]
        if pr.returncode != 0 or not line:
            return {"error": f"leg '{leg}' rc {pr.returncode}: {so[-300:]}"}
        res = json.loads(line[-1])
        res["process_seconds"] = round(time.perf_counter() - t0, 1)
        return res
    except Exception as ex:
        return {"error": str(ex)[:300]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=400, help="timed steps (default 400: about one second of GPU time at config 3)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--gaussians", type=int, default=2_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scene", default="random", choices=["random", "lidar"])
    ap.add_argument("--mode", default="train", choices=["train", "render", "slam"],
                    help="train = fwd+loss+bwd+Adam; render = bare fwd+bwd; slam = train with extend() appends every 20 steps "
                         "(SURVEY config 3 instance: starts at 75 %% of --gaussians, +5 %% LiDAR points per append)")
    ap.add_argument("--host", default="fused", choices=["fused", "dropin"],
                    help="fused = the framework's own step on the fused entry points (activations + loss inside the kernels, no autograd "
                         "graph); dropin = the reference's operator API + LibTorch autograd, i.e. what an unmodified reference host runs")
    ap.add_argument("--lr-scale", type=float, default=0.01,
                    help="learning rates = reference defaults x this.  The synthetic scene has no real target: at the full rates it fades within ~40 "
                         "steps (instances R 8M -> 3.6M), i.e. the work per step would shrink while it is being timed; 0.01 keeps every step on the "
                         "same workload.  Every kernel still does its full work (Adam updates every visible row)")
    ap.add_argument("--split-adam", action="store_true", help="fused host path with Adam as its own launch (the N > 1 compute path: gradients to the slab, then Adam), on one GPU")
    ap.add_argument("--graph", action="store_true", help="time the step as ONE hipGraph replay (capacity-mode forward, no host round trip) instead of eager launches; "
                                                          "single GPU, fused host path.  The default run reports it next to `value` as `graphed`")
    ap.add_argument("--ply", default=None, help="load the map from a saveMap-format PLY file (gaussian.cpp:306-397, io_ply.load_map) instead of generating "
                                               "the synthetic scene; --gaussians is ignored, the camera is the synthetic rig's")
    ap.add_argument("--density", type=float, default=1.0, help="multiply every Gaussian's sigma by this (raw scaling += log k): 2-3 gives 10-20 tile "
                                                             "instances per visible Gaussian instead of the default scene's 4.3 (long lists, sort at R ~ 15-30M)")
    ap.add_argument("--opacity-shift", type=float, default=0.0, help="added to the raw (logit) opacities: negative values keep pixels unsaturated for longer, "
                                                                   "i.e. the blend kernels walk further down their lists")
    ap.add_argument("--math", default="default", choices=["default", "strict", "fast"],
                    help="arithmetic of the blend kernels for the timed region: default = the library's (strict unless GSLIC_FAST_MATH=1)")
    ap.add_argument("--views", type=int, default=16, help="views of the `views_cycle` leg: K synthetic cameras (yaw / translation rig of SURVEY 8d continued) with K "
                                                             "different targets, visited in a shuffled order, every step's target uploaded from pinned host memory on a "
                                                             "side stream while the previous step runs — the reference's optimize() pattern (gaussian.cpp:645-678); 0 = skip")
    ap.add_argument("--map-order", default="morton", choices=["morton", "insertion"],
                    help="row order of the map in device memory (trainer.GaussianModel(order=...)).  morton (default): the library keeps the rows sorted along a "
                         "space-filling curve, as a SLAM map's frame-by-frame insertion order does by itself and the synthetic scene's random order does not; "
                         "results are bit-identical to the insertion order (tests/test_morton_order_gpu.py).  insertion: the rows as generated")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="the contract line only: no second process at all (neither the growth-schedule leg nor --extras)")
    ap.add_argument("--extras", action="store_true", help="with --full: after the contract measurements, run the secondary legs (views_cycle, math_modes, other_host_path, graphed, "
                                                          "joint_pose_step, cpp hosts) in a SECOND process and merge its results into the line")
    ap.add_argument("--leg", default=None, choices=["growth_schedule", "extras", "dropin"], help=argparse.SUPPRESS)   # child mode: one leg process
    ap.add_argument("--profile-all", action="store_true", help="HIP-event time every kernel inside the timed region (adds overhead; --full)")
    ap.add_argument("--full", action="store_true", help="besides the headline: roofline, cpu_baseline, value_long, the N > 1 per-kernel pass and "
                                                        "collectives alone, and the growth_schedule / dropin_host legs (off: set up, warm up, time, print)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="after the timed steps, write what the last timed step handed its caller "
                                                                        "(loss terms, visibility mask, updated parameters) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if (args.profile_all or args.extras) and not args.full:
        ap.error("--profile-all and --extras are --full measurements: add --full")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args.gpus))   # `python bench.py --gpus N`, the shape of the driver's N = 1 command: spawn the N ranks ourselves
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    json_out = sys.stdout
    if world > 1 or os.environ.get("GSLIC_FORCE_DIST") == "1":
        # ONE JSON line on stdout is the contract, and the collective libraries talk on stdout from C++ (gloo: "[Gloo] Rank 1 is connected to ..."):
        # keep the real stdout for the line, send everything else that is written to file descriptor 1 to stderr
        json_out = os.fdopen(os.dup(1), "w")
        sys.stdout.flush()
        os.dup2(2, 1)
    assert torch.cuda.is_available(), "bench.py needs a GPU (no CPU fallback exists)"
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run (or let bench.py spawn the ranks: unset WORLD_SIZE)"
    ndev = torch.cuda.device_count()
    dev = torch.device("cuda", local_rank % ndev)
    torch.cuda.set_device(dev)   # before the process group: RCCL binds the communicator to the current device
    # one rank per GPU over RCCL is the product path.  On a box with fewer GPUs than ranks (a one-GPU box running `--gpus 2`) the ranks share
    # devices, which RCCL refuses (duplicate GPU in a communicator): the SAME step then runs its collectives through gloo on device tensors,
    # the line says so in `launch.backend`, and `rccl_ranks` stays null — a plumbing check, not a scaling number.
    backend = "nccl" if world <= ndev else "gloo"
    if world > 1 or os.environ.get("GSLIC_FORCE_DIST") == "1":
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        if backend == "nccl":
            torch.distributed.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            torch.distributed.init_process_group("gloo", rank=rank, world_size=world)

    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib, trainer
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import gt_image, lidar_scene, pixel_grad, random_scene

    if args.leg is not None:   # child mode: one secondary leg in this process, its JSON dict on stdout, nothing else
        import bench_legs
        res = {"growth_schedule": bench_legs.growth_schedule, "extras": bench_legs.secondary_legs, "dropin": bench_legs.dropin_legs}[args.leg](args, dev)
        print(json.dumps(res), flush=True)
        return
    W, H, P = args.width, args.height, args.gaussians
    if args.math != "default":
        _lib.set_math_mode(args.math == "strict")
    strict_mode = bool(_lib.set_math_mode(True)); _lib.set_math_mode(strict_mode)   # (read the mode in force)
    if args.ply:
        from gaussian_lic_amd import io_ply
        raw = io_ply.load_map(args.ply, sh_degree=3)
        if raw["features_rest"].shape[1] != 15:   # the path is timed at SH degree 3: pad / cut the rest coefficients
            rest = torch.zeros(raw["xyz"].shape[0], 15, 3)
            m = min(15, raw["features_rest"].shape[1]); rest[:, :m] = raw["features_rest"][:, :m]
            raw["features_rest"] = rest
        P = int(raw["xyz"].shape[0])
    else:
        raw = (random_scene if args.scene == "random" else lidar_scene)(P, W, H, sh_degree=3, seed=0)
    if args.density != 1.0:
        raw["scaling"] = (raw["scaling"] + float(np.log(args.density))).contiguous()
    if args.opacity_shift != 0.0:
        raw["opacity"] = (raw["opacity"] + args.opacity_shift).contiguous()
    if args.mode == "slam":   # the map does not cover the right 30 % of the image yet: that is where extend() inserts LiDAR points
        u_pix = raw["xyz"][:, 0] * (0.675 * W) / raw["xyz"][:, 2].abs().clamp_min(0.2) + 0.4857 * W
        keep = u_pix < 0.7 * W
        raw = {k: (v[keep].contiguous() if torch.is_tensor(v) else v) for k, v in raw.items()}
    model = trainer.GaussianModel(raw, dev, capacity=P if args.mode == "slam" else None, order=args.map_order)
    from gaussian_lic_amd.trainer import DEFAULT_LRS
    model.training_setup({k: v * args.lr_scale for k, v in DEFAULT_LRS.items()})
    cam = synthetic_camera(W, H, None if world == 1 else rank % 8).to_device(dev)
    gt = gt_image(H, W, seed=2 + rank).to(dev)
    dL = pixel_grad(H, W, seed=1).to(dev)
    bg = torch.zeros(3, device=dev)

    # Size the caching allocator for 288 GB HBM up front: one reserved slab that every later request is carved from,
    # so no hipMalloc (tens of ms each at these sizes) lands inside the timed region.
    slab = torch.empty(int(min(24, 6 + 10 * P / 2e6)) << 30, dtype=torch.uint8, device=dev)
    del slab

    host = dict(mode=args.host)
    slam = dict(it=9, inserted=0, ms=0.0, calls=0, warm=False)   # it=9: the first step() of the warm-up makes the uncounted first extend()
    if args.mode == "slam":
        frame = lidar_scene(P // 20, W, H, sh_degree=3, seed=100)   # one LiDAR frame in the camera's view: 5 % of the map size
        f_pts = frame["xyz"].to(dev)
        f_col = (frame["features_dc"].reshape(-1, 3) * 0.28209479177387814 + 0.5).to(dev)
        f_rsp = frame["xyz"][:, 2].contiguous().to(dev)
        Rcw = torch.from_numpy(cam.world_view_transform[:3, :3].T.copy())
        tcw = torch.from_numpy(cam.world_view_transform[3, :3].copy())

    graphed = dict(gs=None)
    last = {}   # what the latest step handed back to its caller (--dump-outputs)

    def step():
        if graphed["gs"] is not None:
            last["terms"] = graphed["gs"].step()
            return None
        if args.mode == "slam":
            slam["it"] += 1
            if slam["it"] % 10 == 0:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                n_ins = model.extend(cam, f_pts, f_col, f_rsp, Rcw, tcw, (float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy)))
                e1.record(); e1.synchronize()
                if slam["warm"]:   # the first call pays one-off allocations; it is made in the warm-up and not counted
                    slam["inserted"] += n_ins; slam["ms"] += e0.elapsed_time(e1); slam["calls"] += 1
                slam["warm"] = True
        if args.mode in ("train", "slam"):
            if host["mode"] == "fused":
                last["terms"], v = trainer.training_step_fused(model, cam, gt, bg, adam_in_backward=not args.split_adam)
                return v
            last["loss"], v = trainer.training_step(model, cam, gt, bg)
            return v
        return trainer.render_fwd_bwd(model, cam, dL, bg)

    def sync_all():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    if args.graph:
        assert world == 1 and args.mode == "train" and args.host == "fused" and not args.split_adam, "--graph: single GPU, --mode train --host fused"
    # ---- Python's cyclic garbage collector out of the timed loop.  A generation-2 pass over this process's heap (torch imported: ~1e6 objects) takes
    # 47-75 ms, and the N > 1 step allocates enough container objects (c10d Work handles, lists of views) to trigger ONE at about its 70th-79th
    # step — the "one-off 36-39 ms stall at the 79th step of a process group" that rounds 4-5 pushed out of the window with 90 untimed priming steps
    # and attributed to a runtime pool (tools/diag_dist_stall.py, profiles/r06g_dist_stall.log: the collector's own callbacks place the pass inside
    # the slow step; no stall with gc.freeze() or with the collector off; 400 extra collectives beforehand do not move it).  gc.freeze() moves
    # everything allocated so far into the permanent generation: later passes only look at what the loop itself creates.  No priming steps.
    _freeze_gc()
    # (N > 1 keeps ten untimed steps in front of the W warm-up steps as insurance for what a first collective of each size sets up on real links —
    # connections, channel buffers — which no box this repository ran on could show; the garbage collector needs none)
    prime_steps = int(os.environ.get("GSLIC_DIST_PRIME_STEPS", "10" if world > 1 else "0"))
    if prime_steps and trainer._dist_on() and args.mode == "train" and args.host == "fused":
        for _ in range(prime_steps):
            step()
        torch.cuda.synchronize()
    _trace("model on the device; warm-up")
    # ---- warm-up (untimed); with --full the last warm-up steps double as the per-kernel breakdown pass
    nprof = min(3, args.warmup) if args.full else 0
    for _ in range(args.warmup - nprof):
        step()
    torch.cuda.synchronize()
    vis = None
    if args.full:
        _lib.profile_reset()
        _lib.profile_enable(True)
    for _ in range(nprof):
        vis = step()
    breakdown = _lib.profile_collect() if nprof else {}
    _lib.profile_enable(False)
    # the two longest kernels of the instrumented warm-up pass are timed inside the timed region (round 6: preprocess_bwd and render_bwd are within
    # 3 % of each other and trade places from box to box); the DOMINANT one is whichever takes longer over the K timed steps
    candidates = sorted(breakdown, key=lambda k: -breakdown[k][0])[:2] if breakdown else ["render_bwd"]
    dominant = candidates[0]
    if args.graph:   # the timed region replays the captured step; per-kernel HIP events cannot be recorded inside a replay
        graphed["gs"] = trainer.GraphedStep(model, cam, gt, bg, check_every=0, use_graph=True)
        for _ in range(3):
            step()

    _trace("timed region")
    # ---- timed region: exactly K steps (--full: the two candidate kernels bracketed by HIP events on their launch stream)
    dist_on = trainer._dist_on() and args.mode == "train" and args.host == "fused"
    if dist_on:
        trainer.DIST_TIMING = {}
    if args.full:
        _lib.profile_reset()
        _lib.profile_enable(True, only=None if args.profile_all else candidates)
    sync_all()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        vis = step()
    sync_all()
    t1 = time.perf_counter()
    timed = _lib.profile_collect() if args.full else {}
    _lib.profile_enable(False)
    exchange = None
    if dist_on:
        tm, trainer.DIST_TIMING = trainer.DIST_TIMING, None
        n_ev = min(len(tm.get("start", [])), len(tm.get("bwd_done", [])), len(tm.get("end", [])))
        if n_ev:
            comp = sum(a.elapsed_time(b) for a, b in zip(tm["start"][:n_ev], tm["bwd_done"][:n_ev])) / n_ev
            tail = sum(a.elapsed_time(b) for a, b in zip(tm["bwd_done"][:n_ev], tm["end"][:n_ev])) / n_ev
            Pn, n = model.P, world
            mode = trainer.exchange_mode()
            # ring all-reduce: 2 (n-1)/n of the buffer per rank; all-gather: (n-1) x the per-rank payload
            sent = {"rank1": 2.0 * (n - 1) / n * 44 * Pn + (n - 1) * (13 * Pn + 12),
                    "dense": 2.0 * (n - 1) / n * 236 * Pn + 2.0 * (n - 1) / n * Pn,
                    "single": 2.0 * (n - 1) / n * 240 * Pn}.get(mode)
            chunks = trainer.exchange_chunks() if mode == "rank1" else 1
            exchange = {"mode": mode, "chunks": chunks, "collectives_per_step": {"rank1": 3 if chunks == 1 else 2 * chunks, "dense": 4, "sparse": 2, "single": 1}[mode],
                        "compute_ms": round(comp, 3),
                        "exchange_window_ms": round(tail, 3),
                        "window_note": "GPU time from the end of the backward (chunks > 1: of its FIRST chunk) to the end of the step: the collectives AND the "
                                       "Adam / SH-rebuild kernels (and remaining backward chunks) that run behind them; 0.43 ms of Adam / rebuild kernels at 2M "
                                       "Gaussians in a one-rank group, where the collectives are copies",
                        "exposed_fraction_upper_bound": round(tail / max(comp + tail, 1e-9), 4), "bytes_sent_per_rank_per_step": None if sent is None else int(sent),
                        "world": n}
    if graphed["gs"] is not None:
        assert graphed["gs"].check() == 0, "a timed step did not fit its capacity buffers"
        last["visible"] = graphed["gs"].visible
        graphed["gs"] = None
    if args.dump_outputs and rank == 0:   # before anything else runs a step: the outputs of the LAST timed step
        dump_outputs(args.dump_outputs, model, args.mode, dict(last, visible=last.get("visible", vis)))
    timed_all = None
    if dist_on and args.full and not args.profile_all:
        # the N > 1 compute leg gets a per-kernel roofline of its own (sh_grad_from_rgb, the split Adam, preprocess_bwd without Adam): a short
        # fully instrumented pass AFTER the timed region
        _lib.profile_reset()
        _lib.profile_enable(True)
        for _ in range(min(10, args.steps)):
            step()
        sync_all()
        timed_all = _lib.profile_collect()
        _lib.profile_enable(False)
    dt = torch.tensor([t1 - t0], dtype=torch.float64, device=dev)
    if world > 1:
        torch.distributed.all_reduce(dt, op=torch.distributed.ReduceOp.MAX)
    elapsed = float(dt.item())

    _trace(f"timed region done: {1e3 * (t1 - t0) / args.steps:.3f} ms/step" + ("; unit counts" if args.full else ""))
    P = model.P
    stats, roofline, cpu = {}, None, None
    if args.full:
        # ---- unit counts of this workload (one extra forward, untimed), taken RIGHT AFTER the timed steps: the secondary legs below train the map
        # further, and the counts (live instances above all) drift with it — the roofline and the replayed counters must describe the timed region
        with torch.no_grad():
            from gaussian_lic_amd.rasterizer import render
            image, _, _, visible, radii = render(cam, model, bg)
        torch.cuda.synchronize()
        # R and B of the last forward are returned by the C-ABI; re-run through the functional API to read them
        from gaussian_lic_amd import rasterizer as rz
        rs = rz.GaussianRasterizationSettings(H, W, float(cam.tanfovx), float(cam.tanfovy), float(cam.limx_neg), float(cam.limx_pos),
                                              float(cam.limy_neg), float(cam.limy_pos), bg, 1.0, cam.d_world_view_transform,
                                              cam.d_full_proj_transform, 3, cam.d_camera_center)
        with torch.no_grad():
            e = torch.empty(0, device=dev)
            Rn, Bn = rz.rasterize_gaussians(bg, model.get_xyz(), e, model.get_opacity(), model.get_scaling(), model.get_rotation(), 1.0, e,
                                            rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, H, W, rs.limx_neg, rs.limx_pos,
                                            rs.limy_neg, rs.limy_pos, model.get_features_dc(), model.get_features_rest(), 3, rs.campos,
                                            False, False, False)[:2]
        stats = dict(P=P, V=int(visible.sum().item()), R=int(Rn), B=int(Bn), N=W * H, T=((W + 15) // 16) * ((H + 15) // 16), K=16, strict=strict_mode,
                     nv=world, Vu=int(vis.sum().item()) if (vis is not None and torch.is_tensor(vis)) else int(visible.sum().item()))   # (N > 1: `vis` of the last step is the OR over the views)
        try:   # instances / buckets in front of their tile's last contributor: what the blend kernels really process
            with torch.no_grad():
                fwd = rz.rasterize_gaussians(bg, model.get_xyz(), e, model.get_opacity(), model.get_scaling(), model.get_rotation(), 1.0, e,
                                             rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, H, W, rs.limx_neg, rs.limx_pos,
                                             rs.limy_neg, rs.limy_pos, model.get_features_dc(), model.get_features_rest(), 3, rs.campos, False, False, False)
                dbg = rz.debug_export(rs, P, 15, fwd[0], fwd[1], fwd[5], fwd[6], fwd[7], fwd[8], what=("ranges", "max_contrib"))
            n_t = (dbg["ranges"][:, 1] - dbg["ranges"][:, 0]).long()
            live_b = (dbg["max_contrib"].long() + 63) // 64
            stats["B32"] = int(((n_t + 31) // 32).sum().item())   # the reference's 32-entry buckets (SURVEY 8d's B)
            stats["B_live"] = int(live_b.sum().item())
            stats["R_live"] = int(torch.minimum(n_t, 64 * live_b).sum().item())
            del fwd, dbg
        except Exception:
            pass


        # ---- the same K steps through the other host path (reported next to `value`, not part of it)
        def timed_loop(fn, n):
            for _ in range(3):
                fn()
            sync_all()
            o0 = time.perf_counter()
            for _ in range(n):
                fn()
            sync_all()
            odt = torch.tensor([time.perf_counter() - o0], dtype=torch.float64, device=dev)
            if world > 1:
                torch.distributed.all_reduce(odt, op=torch.distributed.ReduceOp.MAX)
            return float(odt.item())

        # ---- the same step over a window of at least one second (the driver's --steps 20 is a 50 ms window): reported beside `value`
        _trace("roofline / cpu_baseline")
        # ---- roofline of the dominant kernel (and, beside it, of the runner-up among the two that were timed)
        fused_adam = args.mode in ("train", "slam") and args.host == "fused" and world == 1
        pmc_path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        pmc, pmc_units_ok = None, False
        if os.path.exists(pmc_path):
            try:
                pmc = json.load(open(pmc_path))
                # the counters are replayed only when they were collected on THIS workload: same scene, and the unit counts the kernels' work
                # depends on (visible Gaussians, instances, live instances / buckets) within 2 % of this run's — otherwise traffic is null
                pu = pmc.get("units") or {}
                pmc_units_ok = (pmc.get("workload") == f"{args.scene}-{P}-{W}x{H}" and strict_mode == bool(pmc.get("strict", True)) and
                                pmc.get("map_order", "insertion") == args.map_order and
                                all(k in pu and stats.get(k) and abs(pu[k] - stats[k]) <= 0.02 * stats[k] for k in ("V", "R", "R_live", "B_live")))
            except Exception:
                pmc = None
        units_now = {k: stats.get(k) for k in ("P", "V", "R", "R_live", "B_live")}

        def hbm_roofline(kname):
            """`bound` is "hbm" for every kernel of this path (integer / fp32 streaming work, no MFMA): achieved = ALGORITHMIC bytes of a launch / its
            average duration by HIP events inside the timed region, frac = achieved / 8 TB/s.  For the two blend kernels that fraction is small because
            they are bound by VALU issue and latency, not by bytes: a model of that sits beside it as `valu_model`, never as `frac`."""
            k_ms, k_n = timed.get(kname, (0.0, 0))
            avg_ms = k_ms / max(k_n, 1)
            abytes = algorithmic_bytes("preprocess_bwd+adam" if (kname == "preprocess_bwd" and fused_adam) else kname, stats)
            if kname == "adam" and dist_on and trainer.exchange_mode() == "rank1":
                abytes = algorithmic_bytes("adam_small", stats)   # rank-1 exchange: features_dc / features_rest are updated inside sh_grad_from_rgb
            if kname == "adam" and k_n > args.steps:
                abytes /= round(k_n / args.steps)   # N > 1: the optimiser runs once per exchanged segment; the formula is per STEP, the time per launch
            achieved = abytes / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
            # HBM traffic and VALU instruction counts cannot be measured from inside this process (PMC counters need rocprofv3 around it): they are
            # REPLAYED from the committed profile of the same workload and labelled with the file they come from; null when the workload differs.
            traffic, traffic_src = None, None
            scan_on = strict_mode and os.environ.get("GSLIC_BWD_SCAN", "1") != "0"
            if pmc is not None and pmc_units_ok:
                pu = pmc.get("units") or {}
                for key in (f"{kname}_scan_kernel" if scan_on else None, f"{kname}_tail_kernel", f"{kname}_kernel", kname):
                    hit = [v for n, v in pmc.get("kernels", {}).items() if key and n.split("<")[0].strip() == key]
                    if hit and traffic is None:
                        traffic = hit[0]["hbm_bytes_per_launch"]
                        traffic_src = (f"profiles/pmc_traffic.json@{pmc.get('tag', 'untagged')} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, calibrated on a "
                                       f"1 GiB copy; collected at V={pu.get('V')} R={pu.get('R')} R_live={pu.get('R_live')} B_live={pu.get('B_live')})")
            r = dict(bound="hbm", kernel=kname, achieved=round(achieved, 2), peak=HBM_PEAK_GBS, unit="GB/s",
                     frac=round(achieved / HBM_PEAK_GBS, 5), traffic=traffic, traffic_source=traffic_src, algorithmic_bytes_per_launch=abytes,
                     avg_launch_ms=round(avg_ms, 4), launches_timed=int(k_n), ms_in_timed_region=round(k_ms, 3),
                     timing="HIP events around every launch of the kernel inside the timed region", units=units_now)
            if kname in ("render_fwd", "render_bwd"):
                cpi = VALU_CYCLES_PER_INST["render_bwd" if (kname == "render_bwd" and scan_on) else ("render_bwd_pipeline" if kname == "render_bwd" else "render_fwd")]
                r["valu_model"] = dict(modelled_issue_cycles_per_inst=cpi, shader_clock_ghz=SHADER_CLOCK_GHZ, simds=1024,
                                       note="NOT the roofline fraction.  VALU instructions per launch (rocprofv3 SQ_INSTS_VALU of the same workload) x modelled issue "
                                            "cycles per instruction (instruction mix of the inner loop x tools/ubench/issue_rate) / (launch duration x 1024 SIMDs x "
                                            "clock): an upper bound on how issue-bound the kernel is — it counts the set-up code's instructions too, and timed by "
                                            "elimination (profiles/r04y_bwd_scan_by_elimination.log) the row-scan backward's inner loops are 37 % of its time")
                try:
                    import ast
                    import glob
                    sq_files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_sq_counters.txt")))   # the newest tag sorts last
                    for line in (open(sq_files[-1]) if sq_files else []):
                        name, _, rest = line.partition(" {")
                        if name.split("<")[0].strip() in (f"{kname}_kernel", f"{kname}_tail_kernel", f"{kname}_scan_kernel" if scan_on else "-") and pmc_units_ok:
                            c = ast.literal_eval("{" + rest.strip())
                            insts = c["SQ_INSTS_VALU"] * 32.0   # the extract averages per shader engine; 32 engines
                            cycles = 1024.0 * avg_ms * 1e-3 * SHADER_CLOCK_GHZ * 1e9
                            r["valu_model"].update(valu_insts_per_launch=insts, counters_source="profiles/" + os.path.basename(sq_files[-1]),
                                                   simd_cycles_per_valu_inst=round(cycles / insts, 2) if insts else None,
                                                   issue_frac_modelled=round(insts * cpi / cycles, 4) if cycles else None)
                except Exception:
                    pass
            return r

        tie = False
        if len(candidates) > 1 and all(k in timed for k in candidates):
            t_a, t_b = timed[candidates[0]][0], timed[candidates[1]][0]
            dominant = max(candidates, key=lambda k: timed[k][0])
            # Within 5 % of each other the order is run-to-run noise (same box, same script: preprocess_bwd 434.8 us by HIP events and 452.7 under
            # rocprofv3, render_bwd 440.4 / 442.6: profiles/r06z_*): the tie goes to the kernel that moves more bytes — the one the HBM roofline binds —
            # and the other sits beside it as `runner_up` with its own time, bytes and fraction.
            if abs(t_a - t_b) <= 0.05 * max(t_a, t_b):
                tie = True
                fa = args.mode in ("train", "slam") and args.host == "fused" and world == 1
                ab = {k: algorithmic_bytes("preprocess_bwd+adam" if (k == "preprocess_bwd" and fa) else k, stats) for k in candidates}
                dominant = max(candidates, key=lambda k: ab[k])
        roofline = hbm_roofline(dominant)
        others = [k for k in candidates if k != dominant]
        if others:
            ru = hbm_roofline(others[0])
            roofline["runner_up"] = {k: ru[k] for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes_per_launch",
                                                         "avg_launch_ms", "launches_timed", "ms_in_timed_region")}
            roofline["dominant_rule"] = ("the longer of the two longest kernels over the K timed steps (HIP events around both)" if not tie else
                                         "the two longest kernels are within 5 % of each other over the K timed steps (HIP events around both; their order is "
                                         "run-to-run noise): named is the one that moves more algorithmic bytes, the other is `runner_up`")
        # the whole step against the HBM peak on SURVEY 8d's A_view (the survey's figure of merit): algorithmic bytes of one view / ms_per_step
        av = a_view_bytes(stats)
        step_ms = 1e3 * elapsed / args.steps
        roofline["step"] = dict(algorithmic_bytes=av["A_view"], parts={k: v for k, v in av.items() if k != "A_view"},
                                achieved_TBps=round(av["A_view"] * world / (step_ms * 1e-3) / 1e12, 3) if step_ms > 0 else None,
                                frac=round(av["A_view"] * world / (step_ms * 1e-3) / 1e9 / (HBM_PEAK_GBS * world), 4) if step_ms > 0 else None,
                                note="SURVEY.md 8d A_view at this run's P, V, R, B32, N, T (per view; N > 1: per GPU) / ms_per_step / 8 TB/s")

        # ---- CPU baseline: the oracle (C port of the reference kernels, OpenMP) on a 1/16-scale sample of the same workload
        if world == 1 and not args.no_cpu_baseline:
            cpu = cpu_baseline(args)

    views = args.steps * world
    if (P, W, H) == (2_000_000, 1920, 1080) and args.scene == "random":
        config_label = "BASELINE config 3" if world == 1 else "BASELINE config 4"
    elif (P, W, H) == (500_000, 1920, 1080) and args.scene == "lidar":
        config_label = "BASELINE config 2"
    elif (P, W, H) == (5_000_000, 3840, 2160):
        config_label = "BASELINE config 5 shape" + (" on one GPU" if world == 1 else "")
    else:
        config_label = "custom configuration"
    if args.ply:
        config_label = f"map loaded from {os.path.basename(args.ply)} (saveMap PLY)"
    if args.density != 1.0 or args.opacity_shift != 0.0:
        config_label += f", sigma x{args.density:g}, logit opacity {args.opacity_shift:+g}"
    out = {
        "metric": "rendered views/sec (fwd+bwd) at 1080p, 2M Gaussians" if (P == 2_000_000 and (W, H) == (1920, 1080))
        else f"rendered views/sec (fwd+bwd) at {W}x{H}, {P} Gaussians",
        "value": round(views / elapsed, 3), "unit": "views/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic", "full": bool(args.full),
        "config": {"workload": f"{config_label}: {P} Gaussians ({'PLY map' if args.ply else args.scene + ' scene, seed 0'}), {W}x{H}, SH degree 3, "
                               + ("render fwd + 0.8*L1+0.2*(1-fused-SSIM) + bwd + sparse Adam per view"
                                  if args.mode in ("train", "slam") else "bare render fwd+bwd per view")
                               + (" (fused entry points: activations and loss inside the kernels)" if args.host == "fused" and args.mode != "render"
                                  else " (reference operator API + LibTorch autograd)")
                               + (f"; learning rates x{args.lr_scale:g} (stationary synthetic scene)" if args.mode != "render" else "")
                               + ("; map rows kept in Morton order by the library (bit-identical results; `insertion_order` beside it with --extras)" if args.map_order == "morton" else "")
                               + ("; step replayed as one hipGraph (capacity-mode forward)" if args.graph else "")
                               + ("; extend() append of a LiDAR frame every 10 steps, timed" if args.mode == "slam" else "")
                               + ("" if world == 1 else f"; {world} views/step, one gradient exchange per step ({trainer.exchange_mode()}: "
                                  + {"rank1": "xyz / opacity / scaling / rotation all-reduced, the 3-float colour gradients all-gathered and the SH rows rebuilt locally",
                                     "dense": "the [P x 59] slab all-reduced", "sparse": "the visible rows of the slab all-reduced",
                                     "single": "ONE all-reduce of the [P x 59] slab + the visibility mask as P more floats"}[trainer.exchange_mode()] + ")"),
                   "mode": args.mode, "host": args.host if args.mode != "render" else "dropin", "parallelism": f"dp{world}" if world > 1 else "single",
                   "math": "strict" if strict_mode else "fast", "map_order": args.map_order,
                   # how the forward grouped the instances by tile in the instrumented warm-up pass (without --full: in the last timed step)
                   # (GSLIC_BINNING / gslic_set_binning_mode; auto follows the row order)
                   "binning": (("atomic" if "tile_bin" in breakdown else "radix") if args.full else _lib.binning_path()[0])
                              + " (" + os.environ.get("GSLIC_BINNING", "auto") + ")",
                   "visible": stats.get("V"), "instances_R": stats.get("R"), "buckets_B": stats.get("B"), "instances_live": stats.get("R_live"),
                   "buckets_live": stats.get("B_live")},
        "roofline": roofline,
        "cpu_baseline": cpu,
        "value_long": None,
        "exchange": exchange,
        "views_cycle": None,
        "math_modes": None,
        "other_host_path": None,
        "dropin_host": None,
        "graphed": None,
        "cpp_fused_host": None,
        "joint_pose_step": None,
        "growth_schedule": None,
        "extend": None if args.mode != "slam" else {"calls": slam["calls"], "inserted": slam["inserted"], "final_gaussians": model.P,
                                                    "ms_per_call": round(slam["ms"] / max(slam["calls"], 1), 3)},
        # per-kernel time of the fully INSTRUMENTED warm-up pass (a HIP-event pair around every launch: the events' own overhead makes the
        # sum exceed ms_per_step; used to pick the dominant kernel, not to price the step)
        "kernel_ms_per_step_instrumented": {k: round(v[0] / max(nprof, 1), 4) for k, v in sorted(breakdown.items(), key=lambda kv: -kv[1][0])} if args.full else None,
        "kernel_ms_per_launch_timed": None if not args.profile_all else {k: round(v[0] / max(v[1], 1), 4) for k, v in sorted(timed.items(), key=lambda kv: -kv[1][0])},
        "kernel_roofline": (kernel_table(timed, stats, fused_adam, rank1=dist_on and trainer.exchange_mode() == "rank1") if args.profile_all else
                            (kernel_table(timed_all, stats, False, rank1=trainer.exchange_mode() == "rank1") if timed_all else None)),
    }

    # ---- the contract measurements are complete at this point; with --full this process adds the same step over a >= 1 s window (`value_long`)
    # and, at N > 1, the collectives alone.  Every other leg runs in a process of its own AFTER this one has released the GPU.
    value_long = None
    if args.full and args.mode != "slam":
        _trace("value_long")
        n_long = int(min(4000, max(args.steps, np.ceil(1.2 * args.steps / max(elapsed, 1e-6)))))
        sec = timed_loop(step, n_long)
        value_long = {"value": round(n_long * world / sec, 3), "unit": "views/s", "ms_per_step": round(1e3 * sec / n_long, 3), "steps": n_long,
                      "seconds": round(sec, 3)}
    out["value_long"] = value_long
    if torch.distributed.is_initialized():   # N > 1, and the one-rank group that stands in for it (GSLIC_FORCE_DIST=1)
        _trace("per-rank times, collectives alone")
        per = torch.zeros(world, dtype=torch.float64, device=dev)
        per[rank] = 1e3 * (t1 - t0) / args.steps
        torch.distributed.all_reduce(per)
        ones = torch.ones(1, device=dev)
        torch.distributed.all_reduce(ones)   # a real collective: every rank contributes 1
        out["per_rank_ms_per_step"] = [round(float(v), 3) for v in per.tolist()]
        out["rccl_ranks"] = int(ones.item()) if backend == "nccl" else None
        out["launch"] = {"backend": ("nccl (RCCL), one rank per GPU" if backend == "nccl" else
                                     "gloo on device tensors: more ranks than GPUs on this box, RCCL refuses duplicate devices — plumbing check, not a scaling number"),
                         "ranks": world, "devices": ndev, "ranks_reached_by_all_reduce": int(ones.item()),
                         "self_launched": os.environ.get("GSLIC_BENCH_SELF_LAUNCHED") == "1",
                         "prime_steps": prime_steps, "gc": "gc.collect() + gc.freeze() before the warm-up: the one-off 36-75 ms stall of rounds 4-5 at the ~79th step of a "
                                                           "process group was a generation-2 pass of Python's garbage collector (profiles/r06g_dist_stall.log), not the runtime"}
        if args.full:
            try:
                from bench_legs import collectives_alone
                out["rccl_microbench"] = collectives_alone(model.P, world, rank, dev, backend)
            except Exception as ex:
                out["rccl_microbench"] = {"error": str(ex)[:300]}

    if rank != 0:
        if torch.distributed.is_initialized():
            torch.distributed.destroy_process_group()
        return
    try:
        import faulthandler
        faulthandler.cancel_dump_traceback_later()
    except Exception:
        pass
    if args.full and world == 1 and not args.no_extras and not trainer._dist_on() and args.mode == "train" and args.host == "fused" and not args.graph and not args.split_adam:
        # release the device, then the legs, each in its own process with a budget
        try:
            del model, gt, dL, image, visible, radii, vis
        except NameError:
            pass
        torch.cuda.empty_cache()
        _trace("growth_schedule (second process)")
        growth = run_leg_process("growth_schedule", float(os.environ.get("GSLIC_BENCH_GROWTH_BUDGET_S", "150")), args)
        out["growth_schedule"] = growth
        # SURVEY 8d's literal config-3 instance (1.5M -> 2.0M by five appends, the reference's learning rates) beside the stationary line
        out["config"]["growth_schedule"] = {k: growth.get(k) for k in ("workload", "value", "unit", "ms_per_iteration", "gaussians_start", "gaussians_end",
                                                                        "extend_ms_per_call", "error") if k in growth}
        # The reference's UNMODIFIED host on the drop-in boundary (north_star: "the C++ host keeps its torch::Tensor operator API") beside the fused
        # host `value` is measured on, on the contract line by default since round 6: C++ (the reference's renderer.cpp / rasterizer.cpp / loss_utils.h /
        # optim_utils.h compiled unmodified) and the Python mirror, on the map in BOTH row orders, plus a SLAM-like map grown by extend() in insertion order
        _trace("dropin (third process)")
        drop = run_leg_process("dropin", float(os.environ.get("GSLIC_BENCH_DROPIN_BUDGET_S", "300")), args)
        out["dropin_host"] = drop
        if "error" not in drop:
            out["other_host_path"] = drop.get("python_mirror", {}).get("map_order_of_value")
            out["cpp_fused_host"] = drop.get("cpp")
            best = drop.get("headline_dropin") or {}
            out["config"]["dropin_host"] = {"what": "the reference's unmodified C++ host lines (renderer.cpp:21-88 + gaussian.cpp:683-707 + optim_utils.h:102-137) on libgslic_torch_shim.so, same map, "
                                                    "same view, reference learning rates; rows in the order the HOST keeps them (as generated = random for the synthetic scene)",
                                            "value": best.get("value"), "unit": "views/s", "ms_per_step": best.get("ms_per_step"),
                                            "ratio_to_value": (round(best["value"] / out["value"], 3) if best.get("value") else None),
                                            "ratio_to_fused_step_on_the_same_row_order": drop.get("ratio_dropin_to_fused_same_row_order"),
                                            "fused_step_same_row_order": (drop.get("fused_insertion_order") or {}).get("value"),
                                            "map_order_sort_ms": drop.get("map_order_sort_ms")}
        if args.extras:
            _trace("extras (second process)")
            legs = run_leg_process("extras", float(os.environ.get("GSLIC_BENCH_LEGS_BUDGET_S", "300")), args)
            if "error" in legs:
                out["secondary_legs"] = legs["error"]
            out.update({k: v for k, v in legs.items() if k in ("views_cycle", "math_modes", "other_host_path", "graphed", "cpp_fused_host", "joint_pose_step", "insertion_order",
                                                                "reference_step_in_this_process", "capacity_eager")})
    print(json.dumps(out), file=json_out, flush=True)
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


def kernel_table(timed, stats, fused_adam, rank1=False):
    """Per-kernel roofline of a --profile-all run: average launch time (HIP events inside the timed region), algorithmic bytes per launch
    (DESIGN.md section 4 formulas x this run's unit counts), achieved GB/s and the fraction of the 8 TB/s HBM peak."""
    out = {}
    for k, (ms, n) in sorted(timed.items(), key=lambda kv: -kv[1][0]):
        avg = ms / max(n, 1)
        ab = algorithmic_bytes("preprocess_bwd+adam" if (k == "preprocess_bwd" and fused_adam) else ("adam_small" if (k == "adam" and rank1) else k), stats)
        if k == "adam" and n > 0 and rank1:
            ab /= max(1, round(n / max(1, timed.get("render_bwd", (0, n))[1])))   # launches per step
        gbs = ab / (avg * 1e-3) / 1e9 if avg > 0 else 0.0
        out[k] = {"avg_launch_ms": round(avg, 4), "launches": int(n), "algorithmic_bytes": ab, "achieved_GBps": round(gbs, 1), "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}
    return out


DUMP_ROWS = 1 << 17            # per-Gaussian rows --dump-outputs keeps (60 floats a row: 31.5 MB); a fixed, seeded sample when the map has more
DUMP_BYTES_MAX = 64 << 20


def dump_outputs(out_dir, model, mode, last):
    """--dump-outputs DIR: what the timed path handed its caller after the last timed step, as DIR/<name>.npy, so that two builds of the
    project can be compared output for output (every input of a run is seeded: the same arguments give the same inputs).  Per-Gaussian arrays
    are in the caller's row order (the order the map was created in, whatever order the library keeps its rows in) and, when the map has more
    than DUMP_ROWS rows, on a fixed sample of DUMP_ROWS of them (numpy default_rng(0), sorted):
      rows                  float64 [S]  the sampled rows
      visible               float32 [S]  1.0 where the step saw the Gaussian (radii > 0)
      loss_terms            float32 [2]  mean L1 and mean SSIM of the step (fused host)      loss  float32 [1]  the loss (--host dropin)
      xyz, features_dc, features_rest, opacity, scaling, rotation   float32 [S, ...]  the raw parameters after the step's Adam update
    --mode render hands back the visibility mask only (its gradients are dropped), and the parameters it leaves unchanged are not written."""
    os.makedirs(out_dir, exist_ok=True)
    P = model.P
    rows = np.arange(P) if P <= DUMP_ROWS else np.sort(np.random.default_rng(0).choice(P, DUMP_ROWS, replace=False))
    idx = torch.from_numpy(rows).to(model.device)
    order = model.original_order()   # storage row of every original row (None: the rows are stored in the original order)
    if order is not None:
        idx = order[idx]
    arrays = {"rows": rows.astype(np.float64)}
    for key, name in (("terms", "loss_terms"), ("loss", "loss")):
        if last.get(key) is not None:
            arrays[name] = last[key].detach().float().reshape(-1).cpu().numpy()
    if last.get("visible") is not None:
        arrays["visible"] = last["visible"].reshape(-1)[:P][idx].float().cpu().numpy()
    if mode in ("train", "slam"):
        for name in model.NAMES:
            arrays[name] = getattr(model, name).detach()[idx].float().cpu().numpy()
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_BYTES_MAX, f"--dump-outputs: {total} bytes over the {DUMP_BYTES_MAX} byte budget"
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return sorted(arrays)


def _cpu_step(orc, sc, cam, gt, state, lrs):
    """One training iteration on the CPU oracle: render forward -> 0.8 L1 + 0.2 (1 - SSIM) and its gradient -> render backward -> masked
    Adam on the six parameter groups: the same work as one bench step (the three elementwise activation chains are left out)."""
    f = orc.forward(sc, cam)
    img = f["color"]
    n = float(img.size)
    m, d1, d2, d3 = orc.ssim_forward(img[None], gt[None])
    dL = (0.8 / n) * np.sign(img - gt).astype(np.float32) + orc.ssim_backward(img[None], gt[None], np.full_like(m, -0.2 / n), d1, d2, d3)[0]
    g = orc.backward(sc, cam, f, dL)
    vis = f["pre"]["radii"] > 0
    for key, gname, lr in (("means", "dL_dmean3D", lrs[0]), ("dc", "dL_ddc", lrs[1]), ("shs", "dL_dsh", lrs[2]), ("opac", "dL_dopacity", lrs[3]),
                           ("scales", "dL_dscale", lrs[4]), ("rots", "dL_drot", lrs[5])):
        p = state[key]
        orc.adam(p[0], np.ascontiguousarray(g[gname], np.float32).reshape(p[0].shape), p[1], p[2], vis, lr)
    return f, g, dL


def cpu_baseline(args):
    """The CPU oracle (oracle/gs_oracle.c, a C port of the reference kernels, OpenMP) timed on this box's host cores on the SAME work as
    `value` (forward + loss + backward + Adam): (a) a bounded 1/16-scale sample with every thread and with ONE thread, (b) one
    iteration at the full size when the sample says it fits a 40 s budget.  Also the checker on the sample: max errors, not percentiles."""
    from oracle.oracle import Oracle, build
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import activate, gt_image, lidar_scene, pixel_grad, random_scene, to_numpy
    build()
    orc = Oracle(np.float32)
    nthreads = orc.max_threads()
    lrs = [1.6e-6, 2.5e-5, 2.5e-5 / 20.0, 5e-4, 5e-5, 1e-5]   # the reference's rates x 0.01, as the default bench

    def instance(Ps, Ws, Hs):
        raw = (random_scene if args.scene == "random" else lidar_scene)(Ps, Ws, Hs, sh_degree=3, seed=0)
        sc = to_numpy(activate(raw))
        state = {k: (np.ascontiguousarray(sc[k], np.float32), np.zeros_like(sc[k], np.float32), np.zeros_like(sc[k], np.float32))
                 for k in ("means", "dc", "shs", "opac", "scales", "rots")}
        for k in state:
            sc[k] = state[k][0]   # Adam updates the arrays the oracle renders from
        return raw, sc, state, synthetic_camera(Ws, Hs).as_dict(), gt_image(Hs, Ws, seed=2).numpy()

    Ws, Hs, Ps = args.width // 4, args.height // 4, args.gaussians // 16
    raw, sc, state, cam, gt = instance(Ps, Ws, Hs)
    iters, t_spent = 0, 0.0
    while (iters < 2 or t_spent < 8.0) and iters < 50:
        t0 = time.perf_counter()
        _cpu_step(orc, sc, cam, gt, state, lrs)
        t_spent += time.perf_counter() - t0
        iters += 1
    per_view = t_spent / iters
    orc.set_threads(1)
    t0 = time.perf_counter()
    _cpu_step(orc, sc, cam, gt, state, lrs)
    per_view_1 = time.perf_counter() - t0
    orc.set_threads(nthreads)
    full = None
    if 16.0 * per_view * 1.5 < 40.0:   # one full-size iteration (scene generation excluded), only when the sample predicts it fits the budget
        try:
            _r, sc_f, st_f, cam_f, gt_f = instance(args.gaussians, args.width, args.height)
            t0 = time.perf_counter()
            _cpu_step(orc, sc_f, cam_f, gt_f, st_f, lrs)
            full = {"ms_per_view": round(1e3 * (time.perf_counter() - t0), 1), "threads": nthreads, "iterations": 1,
                    "workload": f"{args.gaussians} Gaussians, {args.width}x{args.height}"}
            del sc_f, st_f
        except Exception as ex:
            full = {"error": str(ex)[:200]}
    # the oracle as the CHECKER on the sample: PSNR of the HIP image against the oracle image, maximum gradient error — on the
    # configuration that is TIMED (round 6): trainer.GaussianModel in --map-order (default: rows in Morton order, ties broken by tie_rank), the
    # forward / backward calls training_step_fused makes (raw parameters, activations inside the kernels), binning as the timed run has it
    parity = None
    try:
        import torch
        from gaussian_lic_amd import _lib, rasterizer as rz, trainer
        from gaussian_lic_amd.camera import synthetic_camera as _sc
        dev = torch.device("cuda", torch.cuda.current_device())
        camo = _sc(Ws, Hs).to_device(dev)
        scp = to_numpy(activate(raw))
        dL = pixel_grad(Hs, Ws).numpy()
        f = orc.forward(scp, cam)
        ob = orc.backward(scp, cam, f, dL)
        # the oracle differentiates w.r.t. the ACTIVATED parameters (as the reference's kernels): chain to the raw leaves like LibTorch's autograd
        leaves = {k: raw[k].detach().clone().float().requires_grad_(True) for k in ("opacity", "scaling", "rotation")}
        acts = [torch.sigmoid(leaves["opacity"]), torch.exp(leaves["scaling"]), torch.nn.functional.normalize(leaves["rotation"])]
        torch.autograd.backward(acts, [torch.from_numpy(np.ascontiguousarray(ob[k], np.float32)).reshape(a_.shape)
                                       for k, a_ in zip(("dL_dopacity", "dL_dscale", "dL_drot"), acts)])
        P_s = int(raw["xyz"].shape[0])
        oref = {"xyz": np.asarray(ob["dL_dmean3D"]).reshape(P_s, 3), "features_dc": np.asarray(ob["dL_ddc"]).reshape(P_s, 1, 3),
                "features_rest": np.asarray(ob["dL_dsh"]).reshape(tuple(raw["features_rest"].shape)), "opacity": leaves["opacity"].grad.numpy(),
                "scaling": leaves["scaling"].grad.numpy(), "rotation": leaves["rotation"].grad.numpy()}
        model = trainer.GaussianModel({k: (v.clone() if torch.is_tensor(v) else v) for k, v in raw.items()}, dev, order=args.map_order)
        e = torch.empty(0, device=dev)
        bg0 = torch.zeros(3, device=dev)
        lim = (float(camo.limx_neg), float(camo.limx_pos), float(camo.limy_neg), float(camo.limy_pos))
        with torch.no_grad():
            xyz, dc_, rest = model.xyz.detach(), model.features_dc.detach(), model.features_rest.detach()
            op, sc_, rot = model.opacity.detach(), model.scaling.detach(), model.rotation.detach()
            R, B, color, final_T, radii, geom, binning, img, sample = rz.rasterize_gaussians(
                bg0, xyz, e, op, sc_, rot, 1.0, e, camo.d_world_view_transform, camo.d_full_proj_transform, float(camo.tanfovx), float(camo.tanfovy),
                Hs, Ws, *lim, dc_, rest, model.sh_degree, camo.d_camera_center, False, False, False, raw_params=True, tie_rank=model.tie_rank)
            path = _lib.binning_path()
            out = {n: torch.empty_like(getattr(model, n).detach()) for n in model.NAMES}
            rz.rasterize_gaussians_backward(bg0, xyz, radii, e, sc_, rot, 1.0, e, camo.d_world_view_transform, camo.d_full_proj_transform,
                                            float(camo.tanfovx), float(camo.tanfovy), *lim, torch.from_numpy(dL).to(dev), dc_, rest, model.sh_degree,
                                            camo.d_camera_center, geom, R, binning, img, B, sample, 0.0, False, raw_params=True, out=out)
        order_idx = model.original_order()
        cimg = color.cpu().numpy().astype(np.float64)
        mse = float(np.mean((cimg - f["color"].astype(np.float64)) ** 2))
        img_err = np.abs(cimg - f["color"]) / max(float(np.abs(f["color"]).max()), 1e-30)
        worst, over, total = 0.0, 0, 0
        for n_ in model.NAMES:
            t_ = out[n_] if order_idx is None else out[n_][order_idx]
            ref = np.asarray(oref[n_], dtype=np.float64).reshape(-1)
            got = t_.cpu().numpy().astype(np.float64).reshape(-1)
            if ref.shape == got.shape and np.abs(ref).max() > 0:
                scale = np.abs(ref).max()
                if n_ == "rotation":   # (gradient w.r.t. the raw quaternion: the scale of the chain it belongs to, as the tests)
                    scale = max(scale, float(np.abs(oref["scaling"]).max()))
                err = np.abs(got - ref) / scale
                worst = max(worst, float(err.max()))
                over += int((err > 1e-4).sum()); total += err.size
        parity = {"psnr_image_vs_oracle_db": round(10.0 * np.log10(1.0 / max(mse, 1e-30)), 1), "image_max_rel_err": float(f"{img_err.max():.2e}"),
                  "image_elements_over_1e-4": int((img_err > 1e-4).sum()), "grad_max_rel_err": float(f"{worst:.2e}"),
                  "grad_elements_over_1e-4": over, "grad_elements": total, "instances_equal": int(R) == int(f["num_rendered"]),
                  "configuration": {"map_order": args.map_order, "tie_rank": model.tie_rank is not None, "binning_path": path[0],
                                    "calls": "rasterize_gaussians / _backward with raw_params, as trainer.training_step_fused"},
                  "note": "the TIMED configuration on the 1/16 sample against the C oracle: the library's default (strict) arithmetic of the blend kernels unless "
                          "GSLIC_FAST_MATH=1; six parameter gradients w.r.t. the raw leaves, un-permuted; relative to the tensor's max-abs.  The full-size "
                          "comparison with the reference's own kernels is tests/test_timed_path_reference_gpu.py"}
    except Exception as ex:  # the baseline leg must never take the bench line down
        parity = {"error": str(ex)[:200]}
    # BASELINE config 1 exactly: 10k random Gaussians, 640x480, SH degree 0 — the reference's own CPU-runnable case
    config1 = None
    try:
        raw1 = random_scene(10000, 640, 480, sh_degree=0, seed=0)
        sc1 = to_numpy(activate(raw1))
        cam1 = synthetic_camera(640, 480).as_dict()
        dL1 = pixel_grad(480, 640).numpy()
        orc.forward(sc1, cam1)
        t0 = time.perf_counter()
        for _ in range(5):
            f1 = orc.forward(sc1, cam1)
        t_f = (time.perf_counter() - t0) / 5
        t0 = time.perf_counter()
        for _ in range(5):
            orc.backward(sc1, cam1, f1, dL1)
        t_b = (time.perf_counter() - t0) / 5
        orc.set_threads(1)
        t0 = time.perf_counter()
        orc.forward(sc1, cam1)
        t_f1 = time.perf_counter() - t0
        orc.set_threads(nthreads)
        config1 = {"workload": "BASELINE config 1: 10000 random Gaussians, 640x480, SH degree 0", "forward_ms": round(1e3 * t_f, 2),
                   "forward_backward_ms": round(1e3 * (t_f + t_b), 2), "threads": nthreads, "forward_ms_1_thread": round(1e3 * t_f1, 2)}
    except Exception as ex:
        config1 = {"error": str(ex)[:200]}
    extrap = round(1.0 / (16.0 * per_view), 4)
    measured_full = isinstance(full, dict) and "ms_per_view" in full
    value = round(1e3 / full["ms_per_view"], 4) if measured_full else extrap
    sample_txt = (f"ONE iteration at the full size ({args.gaussians} Gaussians, {args.width}x{args.height}, SH degree 3: render fwd + 0.8 L1 + 0.2 (1 - SSIM) + bwd + "
                  f"masked Adam) on {nthreads} threads = {full['ms_per_view']} ms" if measured_full else
                  f"extrapolated: 1 / (16 x the 1/16-scale sample's {per_view * 1e3:.1f} ms/view) — the full-size iteration did not fit the time budget")
    return {"value": value, "unit": "views/s", "cores": nthreads, "kind": "port", "sample": sample_txt, "hip_vs_oracle": parity,
            "sample_1_16": {"workload": f"{Ps} Gaussians, {Ws}x{Hs}, SH degree 3, same step", "iterations": iters, "ms_per_view": round(1e3 * per_view, 1), "threads": nthreads,
                            "extrapolated_full_size_views_per_s": extrap, "ms_per_view_1_thread": round(1e3 * per_view_1, 1)},
            "full_size": full, "config1": config1}


if __name__ == "__main__":
    main()
