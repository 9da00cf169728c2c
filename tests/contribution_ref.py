"""Shared by tests/test_contribution_{cpu,gpu}.py: the seeded scenes of the contribution-statistics tests and the float64 replay
of a forward's lists that the kernel is held against (no test in this file).

The replay follows the rule of include/gslic_hip.h (gslic_contribution_accumulate) in numpy float64 on the float32 values the lists hold:
walk a tile's range of point_list front to back, stop at the pixel's n_contrib, skip power > 0 and alpha < 1/255, alpha = min(0.99,
opacity exp(power)), w = alpha T, T <- T (1 - alpha)."""
import numpy as np
import torch

W_A, H_A, P_A = 40, 24, 96          # scene (a): 3 x 2 tiles, the right column and the bottom row of tiles are partial
W_B, H_B, P_B = 16, 16, 400         # scene (b): one tile, a list of several 64-entry batches, pixels that stop early
SEED_A, SEED_B = 5, 9
W_MIN = 0.05                        # the w_min of the counts (ContributionStats.W_MIN)
# Relative margin of the float32 kernel against the float64 replay (max_weight, and the band of the two counts).  Not fixed in advance but
# measured on one MI355X (the line test_contribution_gpu.py prints before it asserts; profiles/contribution_config3.log): the largest relative
# gap of max_w over the visible Gaussians was 4.80e-7 on scene (a) and 1.13e-6 on scene (b) (longer products of (1 - alpha) with alpha near
# 0.95).  The bar is 4x the larger one.
MARGIN = 4.5e-6


def _clone(raw):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in raw.items()}


def scene(name):
    """Raw parameters (CPU) and (W, H) of scene "a" | "b" | "c" (scene "d" is scene "a" in a Morton-ordered model)."""
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd.synthetic import random_scene
    if name == "a":
        return random_scene(P_A, W_A, H_A, sh_degree=0, seed=SEED_A), W_A, H_A
    if name == "c":   # every Gaussian behind the camera: no instance at all
        raw = random_scene(P_A, W_A, H_A, sh_degree=0, seed=SEED_A)
        raw["xyz"][:, 2] = -raw["xyz"][:, 2].abs() - 0.5
        return raw, W_A, H_A
    assert name == "b", name
    raw = random_scene(P_B, W_B, H_B, sh_degree=0, seed=SEED_B)
    g = torch.Generator().manual_seed(SEED_B + 1)
    z = raw["xyz"][:, 2].abs().clamp_min(1.0)           # in front of the camera, all of them, on the one tile
    raw["xyz"][:, 2] = z
    fx = 0.675 * W_B
    u, v = torch.rand(P_B, generator=g) * W_B, torch.rand(P_B, generator=g) * H_B
    raw["xyz"][:, 0] = (u - 0.4857 * W_B) * z / fx
    raw["xyz"][:, 1] = (v - 0.5215 * H_B) * z / fx
    raw["opacity"] = (1.0 + 2.0 * torch.rand(P_B, 1, generator=g)).contiguous()   # sigmoid: 0.73 .. 0.95
    return raw, W_B, H_B


def replay(means2D, conic_opacity, point_list, ranges, n_contrib, W, H, P, w_min=W_MIN, margin=MARGIN):
    """float64 replay.  Arrays as rasterizer.debug_export / the C oracle give them (means2D [P,2], conic_opacity [P,4], point_list [R],
    ranges [T,2], n_contrib [H,W]).  Returns per Gaussian: max_w, sum_w (float64), pairs (contributing pairs), n_hi / n_lo (pairs with
    w >= w_min (1 + margin) / w >= w_min (1 - margin): the kernel's count lies between them), and final_T [H,W]."""
    m2d = np.asarray(means2D, np.float64).reshape(P, 2)
    co = np.asarray(conic_opacity, np.float64).reshape(P, 4)
    pl = np.asarray(point_list).astype(np.int64).reshape(-1)
    rg = np.asarray(ranges).astype(np.int64).reshape(-1, 2)
    nc_img = np.asarray(n_contrib).astype(np.int64).reshape(H, W)
    gx = (W + 15) // 16
    out = dict(max_w=np.zeros(P), sum_w=np.zeros(P), pairs=np.zeros(P, np.int64), n_hi=np.zeros(P, np.int64), n_lo=np.zeros(P, np.int64),
               final_T=np.ones((H, W)))
    for t in range(rg.shape[0]):
        x0, y0 = (t % gx) * 16, (t // gx) * 16
        ys, xs = np.mgrid[y0:min(y0 + 16, H), x0:min(x0 + 16, W)]
        if ys.size == 0:
            continue
        nc = nc_img[ys, xs]
        T = np.ones(nc.shape)
        lo, hi = rg[t]
        for k in range(int(min(hi - lo, nc.max()))):
            g = pl[lo + k]
            dx, dy = m2d[g, 0] - xs, m2d[g, 1] - ys
            power = -0.5 * (co[g, 0] * dx * dx + co[g, 2] * dy * dy) - co[g, 1] * dx * dy
            alpha = np.minimum(0.99, co[g, 3] * np.exp(np.minimum(power, 0.0)))
            hit = (k < nc) & ~(power > 0.0) & ~(alpha < 1.0 / 255.0)
            if not hit.any():
                continue
            w = np.where(hit, alpha * T, 0.0)
            T = np.where(hit, T * (1.0 - alpha), T)
            out["max_w"][g] = max(out["max_w"][g], w.max())
            out["sum_w"][g] += w.sum()
            out["pairs"][g] += int(hit.sum())
            out["n_hi"][g] += int((hit & (w >= w_min * (1.0 + margin))).sum())
            out["n_lo"][g] += int((hit & (w >= w_min * (1.0 - margin))).sum())
        out["final_T"][ys, xs] = T
    return out


def band_share(rep):
    """Share of the visible Gaussians (pairs > 0) whose two counts differ — the replay's own ambiguity at w_min; the tests need <= 2 %."""
    vis = rep["pairs"] > 0
    return float((rep["n_hi"] != rep["n_lo"])[vis].sum()) / max(int(vis.sum()), 1)


def oracle_lists(name):
    """The lists of a scene from the C oracle (CPU only): what replay() takes, for choosing seeds and w_min without a GPU."""
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import activate, to_numpy
    from oracle.oracle import Oracle
    raw, W, H = scene(name)
    ref = Oracle(np.float32).forward(to_numpy(activate(raw)), synthetic_camera(W, H).as_dict())
    return dict(means2D=ref["pre"]["means2D"], conic_opacity=ref["pre"]["conic_opacity"], point_list=ref["bins"]["point_list"],
                ranges=ref["bins"]["ranges"], n_contrib=ref["n_contrib"], W=W, H=H, P=raw["xyz"].shape[0])
