"""Cameras other than camera.synthetic_camera for the parity tests.  A plain helper: no fixtures, no GPU.

synthetic_camera has fx = fy and a principal point within 3 % of the centre, so in every other test focal_x == focal_y and the four clamp limits
are nearly symmetric: exchanging fx and fy (or cx and cy, or two of the limits) anywhere between the Python call sites and the kernels changes
no bit those tests look at.  The cameras below have fx / fy of 1.3 one way and 0.72 the other, and a principal point well off the centre.

variant_scene re-projects a scene of the existing generators, so the new camera sees the pixel-space distribution the synthetic camera saw (the
10 % overhang beyond the image and the 2 % of points behind the camera included); the generators themselves (the benchmark's scenes) are untouched.
test_camera_variants_cpu.py holds the reference side to the pinhole model under these cameras and shows that the bars of
test_camera_variants_gpu.py reject a focal-length swap; profiles/camera_variants.txt has the figures."""
import functools
import math

import numpy as np

# name -> (fx / W, fy / W, cx / W, cy / H, znear, zfar)
CAMERAS = {
    "aniso": (0.675, 0.52, 0.4857, 0.5215, 0.01, 100.0),
    "offcentre": (0.675, 0.675, 0.30, 0.68, 0.01, 100.0),
    "combined": (0.58, 0.81, 0.62, 0.37, 0.1, 40.0),
}
SYNTHETIC = (0.675, 0.675, 0.4857, 0.5215)      # camera.synthetic_camera's ratios, restated: what the generators place their points with


def intrinsics(name, W, H):
    """(fx, fy, cx, cy) of a variant in pixels, float64."""
    fx, fy, cx, cy, _zn, _zf = CAMERAS[name]
    return fx * W, fy * W, cx * W, cy * H


def variant_camera(name, W, H, view=None):
    """camera.Camera with the variant's intrinsics and depth range at the pose of camera.resolve_view(view)."""
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd.camera import Camera, resolve_view
    fx, fy, cx, cy = intrinsics(name, W, H)
    zn, zf = CAMERAS[name][4:]
    pose = resolve_view(view)
    if pose is None:
        return Camera(W, H, fx, fy, cx, cy, znear=zn, zfar=zf)
    return Camera(W, H, fx, fy, cx, cy, pose[0], pose[1], znear=zn, zfar=zf)


def reproject(xyz, W, H, name):
    """xyz (torch [P,3], placed by a generator with the synthetic intrinsics) -> torch float32 [P,3] whose projection through the variant's
    intrinsics is the pixel (u, v) the synthetic camera gave the point, at the same depth.  float64, rounded to fp32 once."""
    import torch
    p = xyz.double().numpy()
    sfx, sfy, scx, scy = SYNTHETIC[0] * W, SYNTHETIC[1] * W, SYNTHETIC[2] * W, SYNTHETIC[3] * H
    fx, fy, cx, cy = intrinsics(name, W, H)
    z = p[:, 2]
    zs = np.where(z == 0.0, 1.0, z)                      # (a point exactly on the camera plane has no pixel: it stays where it is)
    u, v = p[:, 0] * sfx / zs + scx, p[:, 1] * sfy / zs + scy
    x = np.where(z == 0.0, p[:, 0], (u - cx) * z / fx)
    y = np.where(z == 0.0, p[:, 1], (v - cy) * z / fy)
    return torch.from_numpy(np.stack([x, y, z], 1)).float().contiguous()


def variant_scene(kind, P, W, H, deg, seed, name, view=None, sigma_scale=1.0):
    """conftest.make_scene under a variant camera: (raw torch params, activated numpy dict for the oracle, camera dict, Camera).  The scene of
    the existing generator, re-projected (reproject), then moved into the pose's frame and scaled as make_scene does.  `scaling` stays as
    generated."""
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd.camera import resolve_view
    from gaussian_lic_amd.synthetic import activate, lidar_scene, place_scene, random_scene, to_numpy
    cam = variant_camera(name, W, H, view)
    raw = (random_scene if kind == "random" else lidar_scene)(P, W, H, sh_degree=deg, seed=seed)
    raw["xyz"] = reproject(raw["xyz"], W, H, name)
    pose = resolve_view(view)
    if pose is not None and pose[2]:
        raw = place_scene(raw, pose[0], pose[1])
    if sigma_scale != 1.0:
        raw["scaling"] = (raw["scaling"] + math.log(sigma_scale)).contiguous()
    return raw, to_numpy(activate(raw)), cam.as_dict(), cam


def swapped_focal(cam):
    """The camera dict of `cam` as a call site that exchanged fx and fy would hand it over: tanfovx / tanfovy and the four limits computed with
    the two focal lengths exchanged, `proj` (and so means2D) untouched.  Only the cov2D Jacobian and its clamp window are wrong."""
    w, h = float(cam.image_width), float(cam.image_height)
    fx, fy, cx, cy = float(cam.fy), float(cam.fx), float(cam.cx), float(cam.cy)      # exchanged
    d = dict(cam.as_dict())
    f32 = np.float32
    d["tanfovx"] = float(f32(np.tan(f32(f32(2.0 * math.atan(w / (2.0 * fx))) * f32(0.5)))))
    d["tanfovy"] = float(f32(np.tan(f32(f32(2.0 * math.atan(h / (2.0 * fy))) * f32(0.5)))))
    d["limx_neg"], d["limx_pos"] = float(f32(-0.15 * w / fx - cx / fx)), float(f32(1.15 * w / fx - cx / fx))
    d["limy_neg"], d["limy_pos"] = float(f32(-0.15 * h / fy - cy / fy)), float(f32(1.15 * h / fy - cy / fy))
    return d


# ---------------------------------------------------------------------------------------------------------------- the parity cases and their bars
TOL = 1e-4                 # images (conftest.assert_close_flips' default) and gradients (test_parity_gpu.py): of the tensor's max-abs
GRADS = ("dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmean3D", "dL_dcov3D", "dL_ddc", "dL_dsh", "dL_dscale", "dL_drot")
SHAPES = {
    "random_3000_70x50_d2": ("random", 3000, 70, 50, 2, None),          # ragged image
    "random_10000_320x240_d3": ("random", 10000, 320, 240, 3, None),
    "lidar_8000_200x150_d3_se3a": ("lidar", 8000, 200, 150, 3, "se3_a"),  # placed
}
ROWWISE_SHAPE = "random_10000_320x240_d3"      # the shape on which the GPU test also runs the row-wise bar of tests/rowwise.py
# (shape, variant) -> seed.  The seed is the first of 0, 1, 2, ... on which the REFERENCE alone leaves headroom (test_camera_variants_cpu.py::
# test_reference_headroom, a condition on the inputs): the fp32 oracle against the fp64 oracle has at most half of assert_close_flips'
# max_flip_frac of the colour and final_T elements beyond TOL, and at most half of rowwise.OUTLIER_SHARE of each gradient tensor's rows as
# outliers.  Tried seeds and their figures (image elements beyond TOL of colour / final_T; the largest outlier share in units of the cap):
SEEDS = {
    ("random_3000_70x50_d2", "aniso"): 0,        # seed 0: 0 / 0, share 0.39 (dL_dopacity)
    ("random_3000_70x50_d2", "offcentre"): 0,    # seed 0: 0 / 0, share 0.49 (dL_dopacity)
    ("random_3000_70x50_d2", "combined"): 0,     # seed 0: 0 / 0, share 0.48 (dL_dopacity)
    # 230400 colour and 76800 final_T elements: at most 2 and 0 may lie beyond TOL.  Seeds 0 ... 9 (colour / final_T): 8/4, 3/1, 3/0, 3/1,
    # 285/156, 10/2, 3/1, 6/2, 0/1, 0/1 (outlier shares 0.00 ... 0.32); seed 10: 0 / 0, share 0.13 (dL_dopacity)
    ("random_10000_320x240_d3", "combined"): 10,
    # 90000 and 30000 elements: none may.  Seeds 0, 1: 3/1, 3/1 (one pixel 6e-3 of max-abs; shares 0.06); seed 2: 0 / 0, share 0.00
    ("lidar_8000_200x150_d3_se3a", "combined"): 2,
}
PARITY_CASES = list(SEEDS)
MUTANT_CASES = [("random_3000_70x50_d2", "aniso"), ("random_3000_70x50_d2", "combined"), ("random_10000_320x240_d3", "combined")]


def build_case(shape, name, seed=None):
    """(raw, sc, camd, cam, P, W, H) of one of PARITY_CASES (seed: another seed than the recorded one, for the seed search)."""
    kind, P, W, H, deg, view = SHAPES[shape]
    raw, sc, camd, cam = variant_scene(kind, P, W, H, deg, SEEDS[(shape, name)] if seed is None else seed, name, view=view)
    return raw, sc, camd, cam, P, W, H


def flip_counts(a, b, tol=TOL):
    """(elements beyond tol of max-abs, elements, max error in units of max-abs): the measure of conftest.assert_close_flips."""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    err = np.abs(a - b) / max(np.abs(b).max(), 1e-30)
    return int((err > tol).sum()), int(b.size), float(err.max())


def image_excess(a, b, tol=TOL, max_flip_frac=2e-5, flip_bound=6e-3):
    """By what factor (a, b) exceeds assert_close_flips' defaults: the larger of count / allowed count and max error / flip_bound (> 1 = rejected)."""
    bad, n, emax = flip_counts(a, b, tol)
    return max(bad / max(1, int(max_flip_frac * n)), emax / flip_bound)


def gradient_errors(got, ref, sc):
    """{tensor: max |got - ref| / scale}: the first gradient bar of test_parity_gpu.py::test_forward_backward_parity.  scale = the reference
    tensor's max-abs; for dL_drot (exactly 0 for isotropic Gaussians) at least the magnitude of the cancelling terms."""
    out = {}
    for k in GRADS:
        a_, b_ = np.asarray(got[k], np.float64).reshape(-1), np.asarray(ref[k], np.float64).reshape(-1)
        scale = np.abs(b_).max() if b_.size else 0.0
        if k == "dL_drot":
            scale = max(scale, float(np.abs(ref["dL_dscale"]).max() * sc["scales"].max()))
        out[k] = float((np.abs(a_ - b_) / max(scale, 1e-30)).max()) if b_.size else 0.0
    return out


def rowwise_excess(cmp, factor):
    """By what factor a comparison of rowwise.compare exceeds rowwise.failures' conditions: the larger of the worst judged stratum ratio / factor
    and the worst outlier count / allowed count (> 1 = rejected)."""
    import rowwise as rw
    worst = max((r for r, _s, _q in rw.max_ratio(cmp).values()), default=0.0) / factor
    cap = max((sg["outliers"] / (rw.OUTLIER_SHARE * sg["rows"]) for _l, sg, _sr in cmp), default=0.0)
    return max(worst, cap)


def outlier_share(cmp):
    """The largest outlier count of a comparison in units of the outlier cap (rowwise.OUTLIER_SHARE of the tensor's rows), and its tensor."""
    import rowwise as rw
    return max(((sg["outliers"] / (rw.OUTLIER_SHARE * sg["rows"]), label) for label, sg, _sr in cmp), default=(0.0, ""))


# ---------------------------------------------------------------------------------------------------------------------------- LiDAR clouds
@functools.lru_cache(maxsize=None)
def variant_cloud(name, W, H, n, view=None, seed=0, plant=True):
    """lidar_depth_ref.cloud on a variant camera: (points float32 [n,3] in the world frame of variant_camera(name, W, H, view), notes).  Random
    returns around the image (a fifth outside it), depth in [0.5, 20); from n = 63 on the rows of lidar_depth_ref.planted (built on the
    variant's identity camera) stand at scattered indices."""
    import lidar_depth_ref as lr
    cam = variant_camera(name, W, H, view)
    fx, fy, cx, cy = float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy)
    rng = np.random.default_rng(1000 * seed + 17 * n + W)
    u, v = rng.uniform(-0.1 * W, 1.1 * W, n), rng.uniform(-0.1 * H, 1.1 * H, n)
    z = rng.uniform(0.5, 20.0, n)
    pc = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1) if n else np.zeros((0, 3))
    notes = dict(planted=None)
    if n >= 63 and plant:
        pl, pn = lr.planted(variant_camera(name, W, H, None))
        at = np.sort(rng.permutation(n)[:pl.shape[0]])
        pc[at] = pl.astype(np.float64)
        notes = dict(planted=at, equal_z=(int(at[pn["equal_z"][0]]), int(at[pn["equal_z"][1]])))
    with np.errstate(all="ignore"):
        world = pc @ np.asarray(cam.R_wc, np.float64).T + np.asarray(cam.t_wc, np.float64) if view is not None else pc
    pts = np.ascontiguousarray(world.astype(np.float32))
    pts.setflags(write=False)
    return pts, notes


@functools.lru_cache(maxsize=None)
def variant_zbuffer(name, W, H, n, view=None):
    """The reference z-buffer (lidar_depth_ref.zbuffer_add) of variant_cloud(name, W, H, n, view) seen from its camera (read-only)."""
    import lidar_depth_ref as lr
    cam = variant_camera(name, W, H, view)
    R, t = lr.pose_f32(cam)
    zb = lr.zbuffer_add(lr.empty(W, H), variant_cloud(name, W, H, n, view)[0], R, t, cam.fx, cam.fy, cam.cx, cam.cy, W, H)
    zb.setflags(write=False)
    return zb
