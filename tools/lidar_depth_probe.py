"""Measures the library's LiDAR depth image beside the torch route at the native and the bench size, in one process, alternating, median of five
rounds.

    timeout -k 10 300 python tools/lidar_depth_probe.py [--rounds 5] [--log profiles/lidar_depth.log]

Two sizes: 640 x 512 with a 24k-point sweep (the sensor's native image) and 1920 x 1080 with 160k points (the bench image); the points are
synthetic.lidar_scene's generator, identity camera.  Per size and footprint in {0, 3}, the two routes in turn within every round, each between two
device events:
    library  trainer.LidarDepth.add + resolve(footprint, margins): one memset, the z-buffer kernel, the resolve kernel (also timed on their own)
    torch    Camera.project_depth + trainer.free_space_bound, plus max_pool2d over the +inf-filled depth for the footprint
Before anything is timed the library's depth and near images are compared with the torch route's on the bits, so that a wrong run does not pass as
a fast one.  For resolve alone the achieved bytes per second are reported against the W * H * (8 + 4 * outputs) bytes it must move — from the
single event-bracketed call, and from 20 calls captured into one graph and replayed (no host between the launches; each call writes fresh outputs,
all reading the same z-buffer).  With --weighted (log it to profiles/lidar_weight.log) a further leg times resolve(weight=, dist2=) beside the plain
resolve at the same footprint and beside the torch route a host needs without it (weighted_leg below).  The process is
the one GPU step: run it under a time limit as above.  Prints one JSON line per size and appends it to --log."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

MARGINS = (0.1, 0.02)
REPLAY = 20   # resolve calls captured into one graph: the per-call time without host launch gaps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--log", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lidar_depth.log"))
    ap.add_argument("--weighted", action="store_true", help="add the weighted-resolve leg (resolve(weight=, dist2=) beside the plain resolve and the torch route)")
    a = ap.parse_args()
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import lidar_scene
    assert torch.cuda.is_available(), "lidar_depth_probe needs a GPU: a time taken anywhere else says nothing"
    dev = torch.device("cuda:0")
    med = statistics.median

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def torch_route(cam, pts, r):
        d = cam.project_depth(pts)
        if r:
            d_inf = torch.where(d > 0, d, torch.full_like(d, float("inf")))
            d = -torch.nn.functional.max_pool2d(-d_inf[None, None], 2 * r + 1, 1, r)[0, 0]
            d = torch.where(torch.isinf(d), torch.zeros_like(d), d)
        return d, trainer.free_space_bound(d, *MARGINS)

    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    for W, H, n in ((640, 512, 24_000), (1920, 1080, 160_000)):
        cam = synthetic_camera(W, H)
        pts = lidar_scene(n, W, H, sh_degree=0, seed=5)["xyz"].to(dev).contiguous()
        ld = trainer.LidarDepth(W, H, dev)
        out = dict(W=W, H=H, points=n, rounds=a.rounds, margins=list(MARGINS), device=torch.cuda.get_device_name(0))

        def lib_route(r):
            ld.clear()
            ld.add(cam, pts)
            return ld.resolve(footprint=r, margins=MARGINS)
        for r in (0, 3):
            got, (want_d, want_n) = lib_route(r), torch_route(cam, pts, r)
            torch.cuda.synchronize()
            assert torch.equal(got["depth"].view(torch.int32), want_d.view(torch.int32)), f"depth differs at footprint {r}"
            assert torch.equal(got["near"].view(torch.int32), want_n.view(torch.int32)), f"near differs at footprint {r}"
            out[f"measured_fraction_r{r}"] = round(float((want_d > 0).float().mean()), 4)
        ms = {}
        for _ in range(a.rounds):
            for r in (0, 3):
                ms.setdefault(f"library_r{r}", []).append(timed(lambda: lib_route(r)))
                ms.setdefault(f"torch_r{r}", []).append(timed(lambda: torch_route(cam, pts, r)))
                ld.clear()
                ms.setdefault("add", []).append(timed(lambda: ld.add(cam, pts)))
                ms.setdefault(f"resolve_r{r}", []).append(timed(lambda: ld.resolve(footprint=r, margins=MARGINS)))
        # resolve alone without the host between launches: REPLAY consecutive calls captured into one graph, replayed between two events
        ld.clear()
        ld.add(cam, pts)
        for r in (0, 3):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                ld.resolve(footprint=r, margins=MARGINS)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(REPLAY):
                    kept = ld.resolve(footprint=r, margins=MARGINS)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(kept["depth"].view(torch.int32), torch_route(cam, pts, r)[0].view(torch.int32)), f"graphed depth differs at footprint {r}"
            ms[f"resolve_r{r}_graphed_per_call"] = [timed(graph.replay) / REPLAY for _ in range(a.rounds)]
        for name, v in ms.items():
            out[f"{name}_event_ms"] = [round(x, 4) for x in v]
            out[f"{name}_event_ms_median"] = round(med(v), 4)
        for r in (0, 3):
            out[f"library_over_torch_r{r}"] = round(med(ms[f"library_r{r}"]) / med(ms[f"torch_r{r}"]), 3)
            must_move = W * H * (8 + 4 * 2)                       # the keys in, depth and near out
            out[f"resolve_r{r}_bytes"] = must_move
            out[f"resolve_r{r}_GBps"] = round(must_move / (med(ms[f"resolve_r{r}"]) * 1e-3) / 1e9, 1)
            out[f"resolve_r{r}_graphed_GBps"] = round(must_move / (med(ms[f"resolve_r{r}_graphed_per_call"]) * 1e-3) / 1e9, 1)
        if a.weighted:
            out.update(weighted_leg(a, trainer, cam, pts, ld, W, H, timed, med))
        line = json.dumps(out)
        print(line)
        with open(a.log, "a") as f:
            f.write(line + "\n")


WEIGHT = (0.05, 0.02, 0.25)   # sigma_abs, sigma_rel, falloff of the weighted leg


def weighted_leg(a, trainer, cam, pts, ld, W, H, timed, med):
    """--weighted: resolve(weight=, dist2=) beside (a) the plain resolve at the same footprint — what the two extra images cost — and (b) the torch
    route a host needs without it: resolve(index=True), then every point re-projected with project_depth's arithmetic, its pixel gathered by the
    index image, range_weight and the falloff — what a host saves.  (b)'s dist2 is compared exactly and its weight to 1e-6 relative before anything
    is timed (the bit-exact yardstick is tests/lidar_weight_ref.py, on the CPU).  Both write depth and near as well, so the three move comparable bytes."""
    import numpy as np
    dev = pts.device
    R_cw = torch.from_numpy(np.ascontiguousarray(cam.R_wc.T.astype(np.float32))).to(dev)
    t_cw = torch.from_numpy((-cam.R_wc.T @ cam.t_wc).astype(np.float32)).to(dev)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    ld.clear()
    ld.add(cam, pts)

    def lib_weighted(r):
        return ld.resolve(footprint=r, margins=MARGINS, weight=WEIGHT, dist2=True)

    def lib_plain(r):
        return ld.resolve(footprint=r, margins=MARGINS)

    def torch_weighted(r):
        im = ld.resolve(footprint=r, margins=MARGINS, index=True)
        pc = pts[:, 0:1] * R_cw[:, 0] + pts[:, 1:2] * R_cw[:, 1] + pts[:, 2:3] * R_cw[:, 2] + t_cw
        zs = torch.where(pc[:, 2] > 0, pc[:, 2], torch.ones_like(pc[:, 2]))
        px = torch.floor((pc[:, 0] * float(cam.fx)) / zs + float(cam.cx)).to(torch.int64)
        py = torch.floor((pc[:, 1] * float(cam.fy)) / zs + float(cam.cy)).to(torch.int64)
        hit = im["index"] >= 0
        gi = im["index"].clamp_min(0).to(torch.int64)
        dx, dy = px[gi] - xs, py[gi] - ys
        s2 = torch.where(hit, dx * dx + dy * dy, torch.full_like(dx, -1))
        w = trainer.range_weight(im["depth"], WEIGHT[0], WEIGHT[1]) * (1.0 / (1.0 + WEIGHT[2] * s2.clamp_min(0).to(torch.float32)))
        im["dist2"], im["weight"] = s2.to(torch.int32), torch.where(hit, w, torch.zeros_like(w))
        return im

    out, ms = dict(weight=list(WEIGHT)), {}
    for r in (0, 3):
        got, plain, want = lib_weighted(r), lib_plain(r), torch_weighted(r)
        torch.cuda.synchronize()
        assert torch.equal(got["depth"].view(torch.int32), plain["depth"].view(torch.int32)), f"weighted depth differs at footprint {r}"
        assert torch.equal(got["near"].view(torch.int32), plain["near"].view(torch.int32)), f"weighted near differs at footprint {r}"
        assert torch.equal(got["dist2"], want["dist2"]), f"dist2 differs from the torch route at footprint {r}"
        assert torch.allclose(got["weight"], want["weight"], rtol=1e-6, atol=0.0), f"weight differs from the torch route at footprint {r}"
        out[f"borrowed_fraction_r{r}"] = round(float((got["dist2"] > 0).float().mean()), 4)
    for _ in range(a.rounds):
        for r in (0, 3):
            ms.setdefault(f"resolve_weighted_r{r}", []).append(timed(lambda: lib_weighted(r)))
            ms.setdefault(f"resolve_plain_r{r}", []).append(timed(lambda: lib_plain(r)))
            ms.setdefault(f"torch_weight_route_r{r}", []).append(timed(lambda: torch_weighted(r)))
    for r in (0, 3):   # without the host between launches, as above
        for name, fn in (("resolve_weighted", lib_weighted), ("resolve_plain", lib_plain)):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                fn(r)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(REPLAY):
                    kept = fn(r)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(kept["depth"].view(torch.int32), lib_plain(r)["depth"].view(torch.int32)), f"graphed {name} depth differs at footprint {r}"
            ms[f"{name}_r{r}_graphed_per_call"] = [timed(graph.replay) / REPLAY for _ in range(a.rounds)]
    for name, v in ms.items():
        out[f"{name}_event_ms"] = [round(x, 4) for x in v]
        out[f"{name}_event_ms_median"] = round(med(v), 4)
    for r in (0, 3):
        out[f"weighted_over_plain_r{r}"] = round(med(ms[f"resolve_weighted_r{r}"]) / med(ms[f"resolve_plain_r{r}"]), 3)
        out[f"weighted_over_plain_r{r}_graphed"] = round(med(ms[f"resolve_weighted_r{r}_graphed_per_call"]) / med(ms[f"resolve_plain_r{r}_graphed_per_call"]), 3)
        out[f"weighted_over_torch_route_r{r}"] = round(med(ms[f"resolve_weighted_r{r}"]) / med(ms[f"torch_weight_route_r{r}"]), 3)
    return out


if __name__ == "__main__":
    main()
