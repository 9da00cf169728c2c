"""Shared by tests/test_freespace_{cpu,gpu}.py: the float64 replay the free-space kernel is held against and the seeded near-bound image of the
toleranced test (no test in this file).

replay() is contribution_ref.replay's walk (imported for the base statistics; the walk is restated here as densify_ref.replay_error restates it,
because the per-pair weights never leave that function) extended by the rule of gslic_contribution_accumulate_free_space (include/gslic_hip.h):
pixel p is measured iff near[p] > 0, and a contributing pair (p, g) adds its w to meas_sum[g] when p is measured and also to free_sum[g] when
z_g < near[p].  The weights are float64; the PREDICATE is evaluated on the float32 values (the exported depths and the image as given), so it
is exactly the kernel's and needs no band."""
import numpy as np
import torch

import contribution_ref as cr

# The random near-bound image of the toleranced test: per scene the interval the measured pixels' bounds are drawn from, inside the depth range of
# the contributing Gaussians as the C oracle gives it (scene (a) 1.07 .. 29.6; scene (b) 1.0 .. 10.2, where the pixels stop early and most of the
# weight lies in front of 6).  Seed and intervals were chosen on the CPU so that at least 10 % of the contributing pairs fall into each of the
# three classes on both scenes — with the oracle's lists (unmeasured, in front, not in front): (a) 0.389 / 0.313 / 0.298, (b) 0.359 / 0.460 /
# 0.181.  test_freespace_cpu.py asserts the condition on the oracle's lists, the GPU test on the device's.
BOUND_SEED = 23
BOUND_RANGE = {"a": (1.0, 30.0), "b": (1.0, 6.0)}
UNMEASURED = 0.40          # share of the pixels that read 0
MIN_CLASS_SHARE = 0.10

# Relative margin of free_sum / meas_sum against this replay: the largest absolute gap relative to the reference tensor's maximum
# (densify_ref.max_gap).  Not fixed in advance: measured on one MI355X (the line test_freespace_gpu.py prints before it asserts;
# DESIGN.md section 8) and set to 4x the larger of the two scenes' gaps, the project's rule for contribution_ref.MARGIN and densify_ref.ERR_MARGIN.
#   scene (a): free_sum 7.094e-8, meas_sum 2.589e-8 (maxima 38.29 / 55.50);  scene (b): free_sum 2.465e-8, meas_sum 1.607e-8 (maxima 47.04 / 47.04)
FREE_GAP_A, FREE_GAP_B = 7.094e-8, 2.465e-8      # the larger of the two sums' gaps per scene
FREE_MARGIN = 2.9e-7                             # 4 x 7.094e-8 = 2.84e-7


def bound_image(name):
    """float32 [H, W] (CPU): about 40 % zeros, three pixels each of NaN, -1.5 and +inf, the rest uniform over BOUND_RANGE[name]."""
    W, H = (cr.W_B, cr.H_B) if name == "b" else (cr.W_A, cr.H_A)
    g = torch.Generator().manual_seed(BOUND_SEED)
    u, v = torch.rand(H, W, generator=g), torch.rand(H, W, generator=g)
    lo, hi = BOUND_RANGE[name]
    near = (lo + (hi - lo) * v).to(torch.float32)
    near[u < UNMEASURED] = 0.0
    odd = torch.randperm(H * W, generator=g)[:9]
    flat = near.view(-1)
    flat[odd[0:3]] = float("nan")
    flat[odd[3:6]] = -1.5
    flat[odd[6:9]] = float("inf")
    return near


def replay(means2D, conic_opacity, point_list, ranges, n_contrib, W, H, P, depths, near):
    """float64 replay with the free-space rule.  depths float32 [P] as exported, near float32 [H, W].  Returns a dict: free_sum, meas_sum, sum_w
    (float64 [P]) and classes = the numbers of contributing pairs (unmeasured, measured and in front, measured and not in front)."""
    m2d = np.asarray(means2D, np.float64).reshape(P, 2)
    co = np.asarray(conic_opacity, np.float64).reshape(P, 4)
    pl = np.asarray(point_list).astype(np.int64).reshape(-1)
    rg = np.asarray(ranges).astype(np.int64).reshape(-1, 2)
    nc_img = np.asarray(n_contrib).astype(np.int64).reshape(H, W)
    z = np.asarray(depths, np.float32).reshape(P)
    nb = np.asarray(near, np.float32).reshape(H, W)
    with np.errstate(invalid="ignore"):
        measured_img = nb > np.float32(0.0)          # NaN, 0 and negative values: not measured; +inf: measured
    gx = (W + 15) // 16
    out = dict(free_sum=np.zeros(P), meas_sum=np.zeros(P), sum_w=np.zeros(P))
    classes = np.zeros(3, np.int64)
    for t in range(rg.shape[0]):
        x0, y0 = (t % gx) * 16, (t // gx) * 16
        ys, xs = np.mgrid[y0:min(y0 + 16, H), x0:min(x0 + 16, W)]
        if ys.size == 0:
            continue
        nc = nc_img[ys, xs]
        T = np.ones(nc.shape)
        lo, hi = rg[t]
        meas = measured_img[ys, xs]
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
            with np.errstate(invalid="ignore"):
                front = meas & (z[g] < nb[ys, xs])   # float32 < float32
            out["sum_w"][g] += w.sum()
            out["meas_sum"][g] += np.where(meas, w, 0.0).sum()    # w or 0, summed in sum_w's order: free <= meas <= sum_w holds exactly
            out["free_sum"][g] += np.where(front, w, 0.0).sum()
            classes += np.array([int((hit & ~meas).sum()), int((hit & front).sum()), int((hit & meas & ~front).sum())])
    out["classes"] = classes
    return out


def class_shares(rep):
    c = rep["classes"].astype(np.float64)
    return c / max(c.sum(), 1.0)


def oracle_depths(name):
    """float32 [P]: the view depths of a scene from the C oracle (CPU only), beside contribution_ref.oracle_lists."""
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import activate, to_numpy
    from oracle.oracle import Oracle
    raw, W, H = cr.scene(name)
    ref = Oracle(np.float32).forward(to_numpy(activate(raw)), synthetic_camera(W, H).as_dict())
    return np.asarray(ref["pre"]["depths"], np.float32)


def max_gap(got, ref):
    """Largest absolute gap relative to the reference tensor's largest magnitude."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))
