"""CPU-only: the camera-pose gradient under LiDAR depth supervision (gslic_rasterize_backward_depth_camera) — argument validation before any
device work, the composition the GPU tests hold the kernels to (depth_camera_helpers.oracle_backward_depth_camera) against central finite
differences of the double-precision oracle, and the Python signatures."""
import ctypes
import inspect

import numpy as np
import pytest

from conftest import make_scene
from depth_camera_helpers import PROJ_IDX, VIEW_IDX, oracle_backward_depth_camera, oracle_depth


def _prm(_lib, P=10, D=3, no_color=0):
    return _lib.RasterParams(P, D, 15, 64, 48, 1.0, 1.0, -1, 1, -1, 1, 1.0, 0, 0, no_color, 0)


def test_depth_camera_entry_point_validates_without_gpu():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    L = _lib.lib()
    dummy = ctypes.c_void_p(16)   # never dereferenced: every call below fails before any device work

    def bwd(prm, dL_ddepth, cam=(dummy, dummy, dummy)):
        return L.gslic_rasterize_backward_depth_camera(ctypes.byref(prm), 5, 5, *([None] * 12), *([dummy] * 4), dummy, dL_ddepth,
                                                       *([dummy] * 10), 0.0, *cam, None)

    for k in range(3):
        cam = [dummy, dummy, dummy]
        cam[k] = None
        assert bwd(_prm(_lib), dummy, cam) == -1 and b"camera-gradient output" in L.gslic_last_error()
    assert bwd(_prm(_lib), None) == -1 and b"dL_ddepth" in L.gslic_last_error()
    assert bwd(_prm(_lib, no_color=1), dummy) == -1 and b"no_color" in L.gslic_last_error()
    assert bwd(_prm(_lib, D=5), dummy) == -1 and b"degree" in L.gslic_last_error()
    assert "gslic_rasterize_backward_depth_camera" in _lib.EXPORTS


def test_pose_functions_take_a_depth_target():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import rasterizer, trainer
    for fn in (trainer.pose_gradient, trainer.training_step_with_pose):
        prm = inspect.signature(fn).parameters
        assert prm["gt_depth"].default is None and prm["lambda_depth"].default == 0.0
    assert inspect.signature(rasterizer.rasterize_gaussians_backward_depth).parameters["camera_grads"].default is False


def _f64(sc):
    return {k: (np.asarray(v, np.float64) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v) for k, v in sc.items()}


def _loss(orc, sc, cam, dL, gD):
    """<dL, colour> + <g_D, depth> on the double-precision oracle."""
    f = orc.forward(sc, cam)
    depth, _ = oracle_depth(orc, f, cam["W"], cam["H"])
    return float((np.asarray(f["color"], np.float64) * dL).sum() + (np.asarray(depth, np.float64) * gD).sum()), f


def _direct_is_material(g):
    row2 = np.abs(g["dL_dviewmatrix"][[2, 6, 10, 14]]).max()
    assert np.abs(g["direct"]).max() >= 1e-2 * row2, (g["direct"], g["dL_dviewmatrix"])


def test_composed_camera_gradient_matches_finite_differences(oracle64):
    """Scene, seeds, step, skip rule, tolerance and floor of test_camera_grad.py::test_oracle_camera_gradient_matches_finite_differences, with
    the depth term added to the loss."""
    W, H = 64, 48
    raw, sc, camd, cam = make_scene("random", 60, W, H, 3, 4)
    sc = _f64(sc)
    camd = dict(camd)
    for k in ("view", "proj", "campos"):
        camd[k] = np.asarray(camd[k], np.float64).copy()
    rng = np.random.default_rng(0)
    dL = rng.standard_normal((3, H, W))
    gD = rng.standard_normal((H, W))
    l0, f0 = _loss(oracle64, sc, camd, dL, gD)
    g = oracle_backward_depth_camera(oracle64, sc, camd, f0, dL, gD)
    _direct_is_material(g)
    checked = 0
    for name, key, idxs in (("dL_dviewmatrix", "view", VIEW_IDX), ("dL_dprojmatrix", "proj", PROJ_IDX), ("dL_dcampos", "campos", [0, 1, 2])):
        scale = max(float(np.abs(g[name]).max()), 1e-12)
        for i in idxs:
            h = 1e-6 * max(1.0, abs(float(camd[key].reshape(-1)[i])))
            cp, cm = dict(camd), dict(camd)
            cp[key] = camd[key].copy(); cp[key].reshape(-1)[i] += h
            cm[key] = camd[key].copy(); cm[key].reshape(-1)[i] -= h
            lp, fp = _loss(oracle64, sc, cp, dL, gD)
            lm, fm = _loss(oracle64, sc, cm, dL, gD)
            if fp["num_rendered"] != f0["num_rendered"] or fm["num_rendered"] != f0["num_rendered"]:
                continue  # a tile decision moved inside the step: the finite difference straddles a discontinuity
            fd = (lp - lm) / (2 * h)
            print(f"{name}[{i}] fd {fd:.9e} analytic {float(g[name][i]):.9e}")
            assert abs(fd - float(g[name][i])) <= 2e-4 * scale + 1e-7, (name, i, fd, float(g[name][i]))
            checked += 1
        for i in range(g[name].size):   # rows that carry no gradient stay exactly zero
            if i not in idxs:
                assert g[name][i] == 0.0
    assert checked >= 20
    # the test has teeth: without the direct term, row 2 of the view gradient is off by far more than the tolerance
    no_direct = g["dL_dviewmatrix"].copy()
    no_direct[[2, 6, 10, 14]] -= g["direct"]
    assert np.abs(no_direct - g["dL_dviewmatrix"]).max() > 10 * (2e-4 * float(np.abs(g["dL_dviewmatrix"]).max()) + 1e-7)


def _camera_f64(cam, R_cw, t_cw):
    """The camera dict of `cam` (intrinsics, limits) at the world-to-camera pose [R_cw | t_cw], every matrix in float64."""
    V = np.eye(4); V[:3, :3] = R_cw; V[:3, 3] = t_cw
    Pm = np.asarray(cam.projection_matrix, np.float64).T
    d = dict(cam.as_dict())
    d["view"] = np.ascontiguousarray(V.T).reshape(16).copy()
    d["proj"] = np.ascontiguousarray((Pm @ V).T).reshape(16).copy()
    d["campos"] = (-R_cw.T @ t_cw).copy()
    return d


@pytest.mark.parametrize("view,extra,seed", [(0, (0.0, 0.0, 0.0), 4), (6, (0.06, -0.04, 0.03), 5), (7, (-0.05, 0.0, 0.08), 6)])
def test_depth_pose_gradient_chain_matches_finite_differences(oracle64, view, extra, seed):
    """Poses, scene, step sizes, tolerance and floor of test_camera_grad.py::test_pose_gradient_chain_matches_finite_differences: Camera.pose_gradient
    on the composed camera gradient of the colour + depth loss against central differences over the six se(3) coordinates."""
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd.camera import se3_exp, synthetic_camera
    W, H = 64, 48
    raw, sc, camd0, _ = make_scene("random", 80, W, H, 3, seed)
    sc = _f64(sc)
    cam = synthetic_camera(W, H, view)
    cam.apply_pose_increment([0.0, 0.0, 0.0, *extra])
    R_cw, t_cw = cam.R_wc.T.copy(), -cam.R_wc.T @ cam.t_wc
    camd = _camera_f64(cam, R_cw, t_cw)
    rng = np.random.default_rng(1)
    dL = rng.standard_normal((3, H, W))
    gD = rng.standard_normal((H, W))
    l0, f0 = _loss(oracle64, sc, camd, dL, gD)
    g = oracle_backward_depth_camera(oracle64, sc, camd, f0, dL, gD)
    _direct_is_material(g)
    cam.world_view_transform = camd["view"].reshape(4, 4)          # (float64 matrices for the chain)
    analytic = cam.pose_gradient(g["dL_dviewmatrix"], g["dL_dprojmatrix"], g["dL_dcampos"])
    scale = max(float(np.abs(analytic).max()), 1e-12)
    checked = 0

    def fd(i, h):
        ls, ok = [], True
        for sgn in (+1.0, -1.0):
            xi = np.zeros(6); xi[i] = sgn * h
            E = se3_exp(xi)
            cd = _camera_f64(cam, E[:3, :3] @ R_cw, E[:3, :3] @ t_cw + E[:3, 3])
            l, f = _loss(oracle64, sc, cd, dL, gD)
            ok = ok and f["num_rendered"] == f0["num_rendered"]
            ls.append(l)
        return (ls[0] - ls[1]) / (2 * h), ok

    for i in range(6):
        # the loss is piecewise smooth in the pose (depth-order swaps, alpha cuts): two step sizes that disagree straddle a jump — skipped
        f1, ok1 = fd(i, 1e-7)
        f2, ok2 = fd(i, 2.5e-8)
        if not (ok1 and ok2) or abs(f1 - f2) > 1e-3 * scale:
            continue
        print(f"xi[{i}] fd {f1:.9e} analytic {analytic[i]:.9e}")
        assert abs(f1 - analytic[i]) <= 5e-4 * scale + 1e-7, (i, f1, analytic[i])
        checked += 1
    assert checked >= 4
