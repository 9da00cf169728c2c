"""CPU-only: the reference side of tests/test_camera_variants_gpu.py under the cameras of tests/camera_variants.py (fx != fy, a principal
point well off the centre, another depth range).

a. the double-precision oracle's means2D / depths / conic against the pinhole model written out in numpy, with every side of the asymmetric
   clamp window exercised;  b. the finite-difference checks of the two camera gradients once more under `combined` at a general pose;
c. the three bars of the GPU parity test reject an oracle whose Jacobian uses fx and fy exchanged, by a wide margin;  d. the fp32 oracle alone
   leaves headroom under those bars on every GPU case's seed;  e. the numpy LiDAR z-buffer reference equals Camera.project_depth.
profiles/camera_variants.txt has the figures of c. and d."""
import numpy as np
import pytest
import torch

import camera_variants as cv
import lidar_depth_ref as lr
import rowwise as rw
from conftest import assert_close_flips, clamp_masked_visible
from depth_camera_helpers import PROJ_IDX, VIEW_IDX, oracle_backward_depth_camera, oracle_depth

VARIANTS = list(cv.CAMERAS)


def test_variants_are_what_they_claim():
    """The intrinsics of the table, a Camera that carries them, and no variant that survives an exchange of fx and fy or of the limits."""
    W, H = 70, 50
    for name, (fx, fy, cx, cy, zn, zf) in cv.CAMERAS.items():
        cam = cv.variant_camera(name, W, H, "se3_a")
        assert (float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy)) == tuple(float(np.float32(v)) for v in (fx * W, fy * W, cx * W, cy * H))
        assert float(cam.znear) == float(np.float32(zn)) and float(cam.zfar) == float(np.float32(zf))
        from gaussian_lic_amd.camera import synthetic_camera
        np.testing.assert_array_equal(cam.world_view_transform, synthetic_camera(W, H, "se3_a").world_view_transform)
    for name in ("aniso", "combined"):
        fx, fy = cv.CAMERAS[name][:2]
        assert max(fx / fy, fy / fx) > 1.25
    for name in ("offcentre", "combined"):
        cam = cv.variant_camera(name, W, H)
        assert abs(abs(cam.limx_neg) - abs(cam.limx_pos)) > 0.2 and abs(abs(cam.limy_neg) - abs(cam.limy_pos)) > 0.2
    a, c = cv.CAMERAS["aniso"], cv.CAMERAS["combined"]
    assert a[0] > a[1] and c[0] < c[1]                        # one ratio each way


def test_reprojection_keeps_the_pixel_distribution():
    """variant_scene's points land, through the variant's intrinsics, on the pixels the generator placed them at; depth and extents unchanged."""
    from gaussian_lic_amd.synthetic import random_scene
    W, H, P = 70, 50, 2000
    base = random_scene(P, W, H, sh_degree=1, seed=3)
    p0 = base["xyz"].double().numpy()
    for name in VARIANTS:
        raw, sc, camd, cam = cv.variant_scene("random", P, W, H, 1, 3, name)
        p = raw["xyz"].double().numpy()
        fx, fy, cx, cy = cv.intrinsics(name, W, H)
        u0, v0 = p0[:, 0] * 0.675 * W / p0[:, 2] + 0.4857 * W, p0[:, 1] * 0.675 * W / p0[:, 2] + 0.5215 * H
        u, v = p[:, 0] * fx / p[:, 2] + cx, p[:, 1] * fy / p[:, 2] + cy
        far = np.abs(p[:, 2]) > 0.05                          # (a point almost on the camera plane has no stable pixel)
        assert np.abs(u - u0)[far].max() < 1e-3 * W and np.abs(v - v0)[far].max() < 1e-3 * W
        assert np.array_equal(p[:, 2], p0[:, 2]) and torch.equal(raw["scaling"], base["scaling"])
        assert (u[far] < 0).any() and (u[far] > W).any() and (v[far] < 0).any() and (v[far] > H).any() and (p[:, 2] < 0).any()


# ---------------------------------------------------------------------------------------------------------------- a. the pinhole model
# a camera moved 1.2 m INTO the identity-frame scene (place=False) and rolled, and Gaussians three times as large: the near part of the scene
# spreads beyond each of the four 15 % margins and still reaches the image, so each side of the clamp window holds visible Gaussians
# (offcentre 95 / 31 / 172 / 36 and combined 107 / 30 / 82 / 201 beyond limx_neg / limx_pos / limy_neg / limy_pos)
CLAMP_VIEW, CLAMP_SIGMA = dict(ypr=(3.0, -2.0, 15.0), t=(0.05, -0.05, 1.2), place=False), 3.0


def _pinhole(sc, camd, fx, fy, cx, cy):
    """means2D [P,2], depths [P], conic [P,3] and (tx/tz, ty/tz) from the pinhole model, float64.  Nothing here is taken from the oracle."""
    V = np.asarray(camd["view"], np.float64).reshape(4, 4).T
    Rv, tv = V[:3, :3], V[:3, 3]
    p = np.asarray(sc["means"], np.float64)
    t = p @ Rv.T + tv
    tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        means2D = np.stack([fx * tx / tz + cx - 0.5, fy * ty / tz + cy - 0.5], 1)
        q = np.asarray(sc["rots"], np.float64)
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], 1),
                      np.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], 1),
                      np.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1)], 1)          # [P,3,3]
        s = np.asarray(sc["scales"], np.float64)
        Sigma = np.einsum("pij,pj,pkj->pik", R, s * s, R)
        J = np.zeros((p.shape[0], 2, 3))
        J[:, 0, 0], J[:, 0, 2] = fx / tz, -fx * tx / (tz * tz)
        J[:, 1, 1], J[:, 1, 2] = fy / tz, -fy * ty / (tz * tz)
        JW = J @ Rv
        cov = np.einsum("pij,pjk,plk->pil", JW, Sigma, JW)
        a, b, c = cov[:, 0, 0] + 0.3, cov[:, 0, 1], cov[:, 1, 1] + 0.3
        det = a * c - b * b
        conic = np.stack([c / det, -b / det, a / det], 1)
        return means2D, tz, conic, tx / tz, ty / tz


@pytest.mark.parametrize("view,sigma", [(None, 1.0), (CLAMP_VIEW, CLAMP_SIGMA)], ids=["identity", "side_view_sigma3"])
@pytest.mark.parametrize("name", VARIANTS)
def test_oracle_matches_the_pinhole_model(oracle64, name, view, sigma):
    W, H, P = 70, 50, 2000
    raw, sc, camd, cam = cv.variant_scene("random", P, W, H, 3, 0, name, view=view, sigma_scale=sigma)
    pre = oracle64.forward(sc, camd)["pre"]
    fx, fy, cx, cy = cv.intrinsics(name, W, H)
    means2D, depths, conic, rx, ry = _pinhole(sc, camd, fx, fy, cx, cy)
    inside = (rx >= camd["limx_neg"]) & (rx <= camd["limx_pos"]) & (ry >= camd["limy_neg"]) & (ry <= camd["limy_pos"])
    rows = (pre["radii"] > 0) & inside
    assert int(rows.sum()) > 1000
    for what, got, want in (("means2D", pre["means2D"], means2D), ("depths", pre["depths"], depths), ("conic", pre["conic_opacity"][:, :3], conic)):
        g, w = np.asarray(got, np.float64)[rows], want[rows]
        err = float(np.abs(g - w).max() / np.abs(w).max())
        print(f"{name} {what}: {err:.2e} of max-abs over {int(rows.sum())} rows")
        assert err < 1e-5, (name, what, err)
    # a swapped focal length would be far outside that: the same model with fx and fy exchanged
    _m, _d, conic_sw, _rx, _ry = _pinhole(sc, camd, fy, fx, cx, cy)
    if fx != fy:
        assert float(np.abs(conic_sw[rows] - conic[rows]).max() / np.abs(conic[rows]).max()) > 0.05


@pytest.mark.parametrize("name", ["offcentre", "combined"])
def test_every_side_of_the_clamp_window_is_exercised(oracle64, name):
    """Visible Gaussians beyond each of the four limits on their own (conftest.clamp_masked_visible with the other three limits opened)."""
    W, H, P = 70, 50, 2000
    raw, sc, camd, cam = cv.variant_scene("random", P, W, H, 3, 0, name, view=CLAMP_VIEW, sigma_scale=CLAMP_SIGMA)
    radii = oracle64.forward(sc, camd)["pre"]["radii"]
    wide = dict(limx_neg=-np.inf, limx_pos=np.inf, limy_neg=-np.inf, limy_pos=np.inf)
    counts = {side: clamp_masked_visible(sc, dict(camd, **dict(wide, **{side: camd[side]})), radii) for side in wide}
    print(name, counts)
    assert all(n >= 10 for n in counts.values()), counts
    assert sum(counts.values()) >= clamp_masked_visible(sc, camd, radii) > 0
    assert abs(camd["limx_neg"]) != abs(camd["limx_pos"]) and abs(camd["limy_neg"]) != abs(camd["limy_pos"])


# ---------------------------------------------------------------------------------------------------------------- b. finite differences
def _f64(sc):
    return {k: (np.asarray(v, np.float64) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v) for k, v in sc.items()}


def _fd_scene():
    """Scene size and seed of test_camera_grad.py::test_oracle_camera_gradient_matches_finite_differences, under `combined` at se3_a."""
    W, H = 64, 48
    raw, sc, camd, cam = cv.variant_scene("random", 60, W, H, 3, 4, "combined", view="se3_a")
    camd = dict(camd)
    for k in ("view", "proj", "campos"):
        camd[k] = np.asarray(camd[k], np.float64).copy()
    return W, H, _f64(sc), camd


def _finite_differences(orc, sc, camd, g, loss, groups):
    """Step, skip rule, tolerance and floor of the two tests named above.  Returns the number of entries checked."""
    l0, f0 = loss(camd)
    checked = 0
    for name, key, idxs in groups:
        scale = max(float(np.abs(g[name]).max()), 1e-12)
        for i in idxs:
            h = 1e-6 * max(1.0, abs(float(camd[key].reshape(-1)[i])))
            cp, cm = dict(camd), dict(camd)
            cp[key] = camd[key].copy(); cp[key].reshape(-1)[i] += h
            cm[key] = camd[key].copy(); cm[key].reshape(-1)[i] -= h
            lp, fp = loss(cp)
            lm, fm = loss(cm)
            if fp["num_rendered"] != f0["num_rendered"] or fm["num_rendered"] != f0["num_rendered"]:
                continue  # a tile decision moved inside the step: the finite difference straddles a discontinuity
            fd = (lp - lm) / (2 * h)
            assert abs(fd - float(g[name][i])) <= 2e-4 * scale + 1e-7, (name, i, fd, float(g[name][i]))
            checked += 1
        for i in range(g[name].size):   # rows that carry no gradient stay exactly zero
            if i not in idxs:
                assert g[name][i] == 0.0
    return checked


GROUPS = (("dL_dviewmatrix", "view", VIEW_IDX), ("dL_dprojmatrix", "proj", PROJ_IDX), ("dL_dcampos", "campos", [0, 1, 2]))


def test_oracle_camera_gradient_matches_finite_differences_combined(oracle64):
    W, H, sc, camd = _fd_scene()
    dL = np.random.default_rng(0).standard_normal((3, H, W))

    def loss(c):
        f = oracle64.forward(sc, c)
        return float((np.asarray(f["color"], np.float64) * dL).sum()), f

    g = oracle64.backward(sc, camd, loss(camd)[1], dL, camera_grads=True)
    assert _finite_differences(oracle64, sc, camd, g, loss, GROUPS) >= 20


def test_composed_camera_gradient_matches_finite_differences_combined(oracle64):
    W, H, sc, camd = _fd_scene()
    rng = np.random.default_rng(0)
    dL, gD = rng.standard_normal((3, H, W)), rng.standard_normal((H, W))

    def loss(c):
        f = oracle64.forward(sc, c)
        depth, _ = oracle_depth(oracle64, f, W, H)
        return float((np.asarray(f["color"], np.float64) * dL).sum() + (np.asarray(depth, np.float64) * gD).sum()), f

    g = oracle_backward_depth_camera(oracle64, sc, camd, loss(camd)[1], dL, gD)
    assert np.abs(g["direct"]).max() >= 1e-2 * np.abs(g["dL_dviewmatrix"][[2, 6, 10, 14]]).max()
    assert _finite_differences(oracle64, sc, camd, g, loss, GROUPS) >= 20


# ---------------------------------------------------------------------------------------------------------------- c. / d. the bars
_cache = {}


def _case(shape, name, oracle32, oracle64):
    """Scene, both oracles' forward and backward of one parity case (kept for the module: c. and d. share them)."""
    if (shape, name) not in _cache:
        from gaussian_lic_amd.synthetic import pixel_grad
        raw, sc, camd, cam, P, W, H = cv.build_case(shape, name)
        dL = pixel_grad(H, W, seed=1).numpy()
        f32, f64 = oracle32.forward(sc, camd), oracle64.forward(sc, camd)
        _cache[(shape, name)] = dict(sc=sc, camd=camd, cam=cam, P=P, dL=dL, f32=f32, f64=f64, vis=(f32["pre"]["radii"] > 0) & (f64["pre"]["radii"] > 0),
                                     g32=oracle32.backward(sc, camd, f32, dL), g64=oracle64.backward(sc, camd, f64, dL))
    return _cache[(shape, name)]


@pytest.mark.parametrize("shape,name", cv.MUTANT_CASES)
def test_bars_reject_a_swapped_focal_length(oracle32, oracle64, shape, name):
    """The fp32 oracle on a camera whose tanfov and limits were computed with fx and fy exchanged (means2D right, Jacobian wrong) against the
    correct fp32 oracle: the image bar, the first gradient bar and the row-wise bar each reject it, by at least ten times their bound."""
    c = _case(shape, name, oracle32, oracle64)
    bad_cam = cv.swapped_focal(c["cam"])
    assert np.array_equal(bad_cam["proj"], c["camd"]["proj"]) and bad_cam["tanfovx"] != c["camd"]["tanfovx"]
    m = oracle32.forward(c["sc"], bad_cam)
    both = c["vis"] & (m["pre"]["radii"] > 0)                  # (the wrong extents cull other rows)
    np.testing.assert_array_equal(m["pre"]["means2D"][both], c["f32"]["pre"]["means2D"][both])
    gm = oracle32.backward(c["sc"], bad_cam, m, c["dL"])
    for k in ("color", "final_T"):
        with pytest.raises(AssertionError):
            assert_close_flips(m[k], c["f32"][k], what=k)
    x_img = min(cv.image_excess(m[k], c["f32"][k]) for k in ("color", "final_T"))
    errs = cv.gradient_errors(gm, c["g32"], c["sc"])
    x_grad = max(errs.values()) / cv.TOL
    cmp = rw.compare(gm, c["g32"], c["g64"], c["vis"], c["P"])
    assert rw.failures(cmp, rw.FACTOR)
    x_row = cv.rowwise_excess(cmp, rw.FACTOR)
    print(f"\nmutant {shape} {name}: image bar x{x_img:.0f}  gradient bar x{x_grad:.0f} (weakest tensor x{min(errs.values()) / cv.TOL:.0f})  "
          f"row-wise bar x{x_row:.0f}")
    assert x_img >= 10 and x_grad >= 10 and x_row >= 10, (x_img, x_grad, x_row)
    assert min(errs.values()) > cv.TOL, errs                  # not one gradient tensor passes


@pytest.mark.parametrize("shape,name", cv.PARITY_CASES)
def test_reference_headroom(oracle32, oracle64, shape, name):
    """The condition on the inputs that chose the seeds of camera_variants.SEEDS: the fp32 oracle against the fp64 oracle uses at most half of
    assert_close_flips' flip allowance on the images and at most half of the row-wise outlier cap on every gradient tensor."""
    c = _case(shape, name, oracle32, oracle64)
    for k in ("color", "final_T"):
        bad, n, emax = cv.flip_counts(c["f32"][k], c["f64"][k])
        print(f"\n{shape} {name} seed {cv.SEEDS[(shape, name)]} {k}: {bad} of {n} beyond {cv.TOL} (max {emax:.2e}); allowed {0.5 * 2e-5 * n:.2f}")
        assert bad <= 0.5 * 2e-5 * n, (k, bad, n)
    cmp = rw.assert_rowwise(c["g32"], c["g32"], c["g64"], c["vis"], c["P"], rw.FACTOR, what=f"{shape} {name}")
    share, label = cv.outlier_share(cmp)
    print(f"{shape} {name}: largest outlier share {share:.2f} of the cap ({label})")
    for label, sg, _ in cmp:
        assert sg["outliers"] <= 0.5 * rw.OUTLIER_SHARE * sg["rows"], (label, sg["outliers"], sg["rows"], rw.worst_rows(sg))


# ---------------------------------------------------------------------------------------------------------------- e. the LiDAR reference
@pytest.mark.parametrize("W,H", [(37, 23), (5, 3)])
@pytest.mark.parametrize("name", VARIANTS)
def test_lidar_reference_equals_project_depth(name, W, H):
    """test_lidar_depth_cpu.py::test_reference_equals_project_depth_at_footprint_0 on the variant cameras: clouds and planted points built on
    the variant, 4097 points, the identity pose and a general one."""
    seen = 0
    for view in (None, "se3_c"):
        cam = cv.variant_camera(name, W, H, view)
        pts, _notes = cv.variant_cloud(name, W, H, 4097, view)
        want = cam.project_depth(torch.from_numpy(pts.copy())).numpy()
        got = lr.resolve(cv.variant_zbuffer(name, W, H, 4097, view), W, H)
        assert np.array_equal(got["depth"].view(np.int32), want.view(np.int32)), (name, view)
        assert np.array_equal(got["index"] == -1, want == 0) and got["n_measured"] == int((want > 0).sum())
        seen += got["n_measured"]
        # the image depends on which focal length goes with which axis: the same cloud through exchanged intrinsics is another image
        if name != "offcentre":
            R, t = lr.pose_f32(cam)
            sw = lr.resolve(lr.zbuffer_add(lr.empty(W, H), pts, R, t, cam.fy, cam.fx, cam.cx, cam.cy, W, H), W, H)
            assert not np.array_equal(sw["depth"], got["depth"])
    assert seen > 0
