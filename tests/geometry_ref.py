"""Shared by tests/test_geometry_{cpu,gpu}.py: scene (e) of the geometry-image tests and the float64 replay of a forward's lists that
gslic_geometry_images is held against (no test in this file).

The replay follows the rule of include/gslic_hip.h (gslic_geometry_images) in numpy float64 on the float32 values the lists hold, in the style of
contribution_ref.replay: walk a tile's range of point_list front to back, stop at the pixel's n_contrib, skip power > 0 and alpha < 1/255,
alpha = min(0.99, opacity exp(power)), w = alpha T, D += z alpha T, A += w, top = the strictly largest w (the frontmost wins a tie),
T <- T (1 - alpha), the median = the first entry whose blending takes T below one half.

Scenes: contribution_ref's a, b, c (and d = a in a Morton-ordered model) plus scene (e) below.  Scenes a and b cannot exercise a_min,
depth_median = 0 or top_row = -1: on the C oracle's lists every pixel of a and b has a contributor, 958 / 960 and 256 / 256 pixels reach the
median and no covered pixel has A < 0.05.  Scene (e) is scene a with every raw opacity lowered by a constant, every raw scaling lowered by a
constant and every second Gaussian moved behind the camera.  The opacity constant alone cannot give the three classes below: scene a's largest
Gaussians cover the whole image, so on the C oracle's lists a shift of -3.0 .. -4.5 leaves 0 % of the pixels without a contributor (86.6 % / 13.4 %
at -3.0), and at -6.0, the first shift with more than 10 % uncovered (12.7 %), no pixel reaches the median any more.  Smaller Gaussians uncover
pixels while the opaque ones stay opaque.  Shares of scene (e)'s 960 pixels on the C oracle's lists (tests/test_geometry_cpu.py asserts each
class >= 10 %):
    OPACITY_SHIFT_E = -0.5, SCALE_SHIFT_E = -1.0:  no contributor 16.1 %, covered but median not reached 73.3 %, median reached 10.5 %;
    22.6 % of the pixels are covered with A < 0.05 and 19.3 % more have 0.05 <= A < 0.15 (the second a_min of the GPU test moves those)
Ambiguous pixels (AMBIG = 1e-4 relative) on the oracle's lists: 0 on a, b and e for top_row, depth_median and depth_norm (a_min 0.05 and 0.15)."""
import numpy as np
import torch

import contribution_ref as cr

A_MIN = 0.05                 # the a_min of the tests (trainer.geometry_images' default)
A_MIN_2 = 0.15               # the second a_min of the GPU test: it moves >= 5 % of scene (e)'s pixels across the threshold
AMBIG = 1e-4                 # a pixel is ambiguous when the deciding quantity lies within this (relative) of its threshold
AMBIG_CAP = 0.02             # at most this share of a scene's pixels may be excluded as ambiguous (a condition, not a measurement)
OPACITY_SHIFT_E = -0.5
SCALE_SHIFT_E = -1.0
# Relative bar (conftest.rel_err) of the float32 kernel against the float64 replay for opacity, top_weight and depth_norm.  Not fixed in advance
# but measured on one MI355X (the line test_geometry_gpu.py prints before it asserts; profiles/geometry_config3.log): the largest gap was
# 3.19e-7 (depth_norm on scene b; opacity 2.91e-7 on scene a, top_weight 1.42e-7 on scene a).  The bar is 4x that — contribution_ref.MARGIN's
# headroom for box-to-box expf and ordering differences — and far below the project's 1e-4.
TOL = 1.3e-6
IMAGES = ("transmittance", "opacity", "depth_sum", "depth_norm", "depth_median", "top_row", "top_weight")


def scene(name):
    """Raw parameters (CPU) and (W, H): contribution_ref.scene for a | b | c, and scene "e"."""
    if name != "e":
        return cr.scene(name)
    raw, W, H = cr.scene("a")
    raw = cr._clone(raw)
    raw["opacity"] = (raw["opacity"] + OPACITY_SHIFT_E).contiguous()
    raw["scaling"] = (raw["scaling"] + SCALE_SHIFT_E).contiguous()
    raw["xyz"][1::2, 2] = -raw["xyz"][1::2, 2].abs() - 0.5
    return raw, W, H


def oracle_forward(name):
    """(lists as replay() takes them, the C oracle's float32 final_T [H,W]) of a scene — CPU only."""
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import activate, to_numpy
    from oracle.oracle import Oracle
    raw, W, H = scene(name)
    ref = Oracle(np.float32).forward(to_numpy(activate(raw)), synthetic_camera(W, H).as_dict())
    L = dict(means2D=ref["pre"]["means2D"], conic_opacity=ref["pre"]["conic_opacity"], depths=ref["pre"]["depths"],
             point_list=ref["bins"]["point_list"], ranges=ref["bins"]["ranges"], n_contrib=ref["n_contrib"], W=W, H=H, P=raw["xyz"].shape[0])
    return L, ref["final_T"]


def empty_lists(W, H, P):
    """The lists of a forward with R = 0."""
    z = np.zeros
    return dict(means2D=z((P, 2)), conic_opacity=z((P, 4)), depths=z(P), point_list=z(0, np.int64),
                ranges=z((((W + 15) // 16) * ((H + 15) // 16), 2), np.int64), n_contrib=z((H, W), np.int64), W=W, H=H, P=P)


def replay(means2D, conic_opacity, depths, point_list, ranges, n_contrib, W, H, P, a_min=A_MIN, margin=AMBIG):
    """float64 replay.  Arrays as rasterizer.debug_export / the C oracle give them (means2D [P,2], conic_opacity [P,4], depths [P], point_list [R],
    ranges [T,2], n_contrib [H,W]).  Returns [H,W] arrays: the seven images (top_row int64), reached (the median was reached), median_row (the
    entry of the median, -1), n_pairs (contributors of the pixel), and the ambiguity masks amb_top (the two largest weights differ by at most
    `margin` relative), amb_median (some T after a blended entry lies within `margin` relative of 0.5), amb_norm (A within `margin` relative of
    a_min)."""
    m2d = np.asarray(means2D, np.float64).reshape(P, 2)
    co = np.asarray(conic_opacity, np.float64).reshape(P, 4)
    zg = np.asarray(depths, np.float64).reshape(P)
    pl = np.asarray(point_list).astype(np.int64).reshape(-1)
    rg = np.asarray(ranges).astype(np.int64).reshape(-1, 2)
    nc_img = np.asarray(n_contrib).astype(np.int64).reshape(H, W)
    gx = (W + 15) // 16
    f, i, b = (lambda v=0.0: np.full((H, W), v)), (lambda v: np.full((H, W), v, np.int64)), (lambda: np.zeros((H, W), bool))
    out = dict(transmittance=f(1.0), opacity=f(), depth_sum=f(), depth_median=f(), top_row=i(-1), top_weight=f(), reached=b(), median_row=i(-1),
               n_pairs=i(0), amb_top=b(), amb_median=b())
    for t in range(rg.shape[0]):
        x0, y0 = (t % gx) * 16, (t // gx) * 16
        ys, xs = np.mgrid[y0:min(y0 + 16, H), x0:min(x0 + 16, W)]
        if ys.size == 0:
            continue
        nc = nc_img[ys, xs]
        shp = nc.shape
        T, A, D, zmed, wtop, w2 = np.ones(shp), np.zeros(shp), np.zeros(shp), np.zeros(shp), np.zeros(shp), np.zeros(shp)
        top, mrow, pairs = np.full(shp, -1, np.int64), np.full(shp, -1, np.int64), np.zeros(shp, np.int64)
        found, ambm = np.zeros(shp, bool), np.zeros(shp, bool)
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
            D = D + np.where(hit, zg[g] * alpha * T, 0.0)
            A = A + w
            pairs += hit
            new = hit & (w > wtop)
            w2 = np.where(new, wtop, np.maximum(w2, w))      # the second largest weight so far
            top = np.where(new, g, top)
            wtop = np.where(new, w, wtop)
            T = np.where(hit, T * (1.0 - alpha), T)
            ambm |= hit & (np.abs(T - 0.5) <= margin * 0.5)
            cross = hit & ~found & (T < 0.5)
            zmed = np.where(cross, zg[g], zmed)
            mrow = np.where(cross, g, mrow)
            found |= cross
        for key, v in (("transmittance", T), ("opacity", A), ("depth_sum", D), ("depth_median", zmed), ("top_row", top), ("top_weight", wtop),
                       ("reached", found), ("median_row", mrow), ("n_pairs", pairs), ("amb_top", (pairs > 1) & (wtop - w2 <= margin * wtop)),
                       ("amb_median", ambm)):
            out[key][ys, xs] = v
    A = out["opacity"]
    out["depth_norm"] = np.where(A >= a_min, out["depth_sum"] / np.where(A > 0, A, 1.0), 0.0)
    out["amb_norm"] = np.abs(A - a_min) <= margin * a_min
    return out


def classes(rep):
    """Shares of the pixels (no contributor, covered but median not reached, median reached)."""
    n = float(rep["n_pairs"].size)
    none = rep["n_pairs"] == 0
    return float(none.sum()) / n, float((~none & ~rep["reached"]).sum()) / n, float(rep["reached"].sum()) / n


def ambiguous_shares(rep):
    """Shares of the pixels that are ambiguous for (top_row, depth_median, depth_norm)."""
    n = float(rep["n_pairs"].size)
    return tuple(float(rep[k].sum()) / n for k in ("amb_top", "amb_median", "amb_norm"))
