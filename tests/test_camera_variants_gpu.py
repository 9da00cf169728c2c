"""-m gpu: the HIP path under cameras with fx != fy and an off-centre principal point (tests/camera_variants.py).

Every other GPU test looks through camera.synthetic_camera, where focal_x == focal_y and the clamp window is nearly symmetric: an exchange of
fx and fy, of cx and cy or of two limits — in the preprocess Jacobian, its backward and clamp masks, the camera-pose gradient, the focal
derivation of the host entry points, the four adjacent float arguments of the LiDAR z-buffer and extend kernels, or any Python / C++ call
site handing them over — would change no bit those tests see.  Here the same comparisons run under the three variants; the bars are those of
the tests named in each section, and test_camera_variants_cpu.py shows that they reject a focal swap and that the reference alone leaves
headroom on every seed used (camera_variants.SEEDS)."""
import ctypes

import numpy as np
import pytest
import torch

import camera_variants as cv
import lidar_depth_ref as lr
import lidar_weight_ref as wr
import rowwise as rw
from conftest import assert_close_flips, rel_err
from depth_camera_helpers import CAM, oracle_backward_depth_camera
from gpu_helpers import bits, gpu
from test_depth_gpu import _mode, bwd, fwd_depth, oracle_backward_depth, oracle_depth

pytestmark = pytest.mark.gpu

TOL = cv.TOL


# ------------------------------------------------------------------------------------------------------------- a. forward / backward parity
@pytest.mark.parametrize("shape,name", cv.PARITY_CASES)
def test_forward_backward_parity(oracle32, oracle64, shape, name):
    """test_parity_gpu.py::test_forward_backward_parity under a variant camera; on the 320x240 shape also the row-wise bar of
    test_rowwise_gradients_gpu.py (strict path)."""
    from gpu_helpers import hip_backward, hip_forward, npy
    from gaussian_lic_amd.synthetic import pixel_grad
    raw, sc, camd, cam, P, W, H = cv.build_case(shape, name)
    ref = oracle32.forward(sc, camd)
    with _mode(True):
        got = hip_forward(raw, cam, export=("tiles_touched", "means2D", "depths", "conic_opacity", "sorted_keys", "point_list", "ranges", "n_contrib"))
        dL = pixel_grad(H, W, seed=1)
        ggot = hip_backward(got, dL)
    d = got["dbg"]
    # ---- integer stage boundaries and the canonical fp32 chain: bit-exact
    np.testing.assert_array_equal(npy(got["radii"]), ref["pre"]["radii"])
    np.testing.assert_array_equal(npy(d["tiles_touched"]).astype(np.uint32), ref["pre"]["tiles_touched"])
    assert got["R"] == ref["num_rendered"] > 0
    np.testing.assert_array_equal(npy(d["sorted_keys"]).view(np.uint64), ref["bins"]["keys"])
    np.testing.assert_array_equal(npy(d["point_list"]).astype(np.uint32), ref["bins"]["point_list"])
    np.testing.assert_array_equal(npy(d["ranges"]).astype(np.uint32), ref["bins"]["ranges"])
    np.testing.assert_array_equal(npy(d["n_contrib"]).astype(np.int64), ref["n_contrib"].astype(np.int64))
    vis = ref["pre"]["radii"] > 0
    np.testing.assert_array_equal(npy(d["means2D"])[vis], ref["pre"]["means2D"][vis])
    np.testing.assert_array_equal(npy(d["depths"])[vis], ref["pre"]["depths"][vis])
    np.testing.assert_array_equal(npy(d["conic_opacity"])[vis], ref["pre"]["conic_opacity"][vis])
    # ---- images
    for k in ("color", "final_T"):
        bad, n, emax = cv.flip_counts(npy(got[k]), ref[k])
        print(f"\n[{shape} {name}] {k}: {bad} of {n} beyond {TOL}, max {emax:.2e} of max-abs")
        assert_close_flips(npy(got[k]), ref[k], what=k)
    # ---- gradients: the first bar
    gref = oracle32.backward(sc, camd, ref, dL.numpy())
    errs = cv.gradient_errors(ggot, gref, sc)
    print(f"[{shape} {name}] gradients: " + "  ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e < TOL, f"{k}: max rel err {e:.3e}"
        assert np.all(ggot[k].reshape(P, -1)[~vis] == 0), f"{k}: invisible rows must be exact zeros"
    # ---- gradients: the row-wise bar
    if shape == cv.ROWWISE_SHAPE:
        f64 = oracle64.forward(sc, camd)
        g64 = oracle64.backward(sc, camd, f64, dL.numpy())
        cmp = rw.compare(ggot, gref, g64, vis & (f64["pre"]["radii"] > 0), P)
        print(rw.format_table(cmp, f"{shape} {name} colour-strict: HIP and the fp32 oracle against the fp64 oracle"))
        print("worst judged ratio: " + rw.worst_line(cmp))
        assert {label for label, _, _ in cmp} >= {"dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmean3D", "dL_dcov3D", "dL_dscale", "dL_ddc", "dL_dsh"}
        bad = rw.failures(cmp, rw.FACTOR, what=f"{shape} {name}")
        assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------------------------- b. camera gradient
CAM_TOL = 2e-4       # of max-abs per output: test_camera_grad.py and test_depth_camera_gpu.py
CHAIN_TOL = 2e-3     # the chained six numbers: test_camera_grad.py::test_hip_pose_gradient_matches_oracle_and_descends
CAMERA_SHAPE = (40, 64, 48, 1, 5)      # the smallest shape of both tests (P < 64: one partly filled wave)


def _check_camera_outputs(cam, out, exp, what):
    for got, name in zip(out[9:], CAM):
        r = np.asarray(exp[name], np.float64)
        g = got.cpu().numpy().astype(np.float64)
        e = float(np.abs(g - r).max()) / max(float(np.abs(r).max()), 1e-30)
        print(f"[{what}] {name}: rel err vs oracle {e:.3e}")
        assert e < CAM_TOL, (name, g, r)
        assert np.all(g[r == 0.0] == 0.0)
    chain = cam.pose_gradient(out[9], out[10], out[11])
    want = cam.pose_gradient(exp["dL_dviewmatrix"], exp["dL_dprojmatrix"], exp["dL_dcampos"])
    e = float(np.abs(chain - want).max()) / max(float(np.abs(want).max()), 1e-30)
    print(f"[{what}] pose gradient {chain}: rel err vs oracle {e:.3e}")
    assert np.abs(want).max() > 0 and e < CHAIN_TOL, (chain, want)


@pytest.mark.parametrize("view", ["se3_a", "se3_c"])
def test_camera_gradients_match_oracle(oracle32, view):
    """gslic_rasterize_backward_camera and gslic_rasterize_backward_depth_camera under `combined`: the comparisons of
    test_camera_grad.py::test_hip_camera_gradient_matches_oracle and test_depth_camera_gpu.py::test_depth_camera_gradient_matches_oracle, and
    Camera.pose_gradient's six numbers of both."""
    from gpu_helpers import hip_forward
    from gaussian_lic_amd import rasterizer as rz
    from gaussian_lic_amd.synthetic import pixel_grad
    P, W, H, deg, seed = CAMERA_SHAPE
    raw, sc, camd, cam = cv.variant_scene("random", P, W, H, deg, seed, "combined", view=view)
    dL = pixel_grad(H, W, seed=1)
    gD = torch.randn(H, W, generator=torch.Generator().manual_seed(11)).float()
    ref_f = oracle32.forward(sc, camd)
    assert int((ref_f["pre"]["radii"] > 0).sum()) >= 10
    # ---- colour
    exp = oracle32.backward(sc, camd, ref_f, dL.numpy(), camera_grads=True)
    f = hip_forward(raw, cam)
    act, rs = f["act"], f["rs"]
    e = torch.empty(0, device=gpu())
    geom, binning, img, sample = f["bufs"]
    call = lambda **kw: rz.rasterize_gaussians_backward(rs.bg, act["means"], f["radii"], e, act["scales"], act["rots"], 1.0, e, rs.viewmatrix, rs.projmatrix,
                                                        rs.tanfovx, rs.tanfovy, rs.limx_neg, rs.limx_pos, rs.limy_neg, rs.limy_pos, dL.to(gpu()),
                                                        act["dc"], act["shs"], act["D"], rs.campos, geom, f["R"], binning, img, f["B"], sample, 0.0,
                                                        False, **kw)
    out, plain = call(camera_grads=True), call()
    for a, b in zip(out[:9], plain):   # the ordinary gradients are the same (another instantiation of the kernel: fma contraction may differ)
        if a.numel():
            assert float((a - b).abs().max()) <= 1e-5 * max(float(b.abs().max()), 1e-30)
    _check_camera_outputs(cam, out, exp, f"colour {view}")
    # ---- colour + depth
    exp = oracle_backward_depth_camera(oracle32, sc, camd, ref_f, dL.numpy(), gD.numpy())
    assert np.abs(exp["direct"]).max() >= 1e-2 * np.abs(exp["dL_dviewmatrix"][[2, 6, 10, 14]]).max()
    with _mode(True):
        fd = fwd_depth(raw, cam)
        t = fd["t"]
        g, bn, im, sm = fd["bufs"]
        dcall = lambda cg: rz.rasterize_gaussians_backward_depth(rs.bg, t["means"], fd["radii"], t["scales"], t["rots"], 1.0, rs.viewmatrix, rs.projmatrix,
                                                                 rs.tanfovx, rs.tanfovy, rs.limx_neg, rs.limx_pos, rs.limy_neg, rs.limy_pos,
                                                                 dL.to(gpu()), gD.to(gpu()), t["dc"], t["shs"], t["D"], rs.campos, g, fd["R"], bn, im,
                                                                 fd["B"], sm, camera_grads=cg)
        out, plain = dcall(True), dcall(False)
        torch.cuda.synchronize()
    assert len(out) == 12 and len(plain) == 9
    for a, b in zip(out[:9], plain):
        if a.numel():
            assert float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30) <= 1e-5
    _check_camera_outputs(cam, out, exp, f"colour + depth {view}")
    dV = out[9].cpu().numpy()
    assert np.all(dV[[3, 7, 11, 15]] == 0.0) and np.all(out[10].cpu().numpy()[[2, 6, 10, 14]] == 0.0)   # view row 3, projection row 2


# ------------------------------------------------------------------------------------------------------------------------- c. depth render
def test_depth_forward_backward_match_oracle(oracle32):
    """test_depth_gpu.py's strict bars (test_depth_forward_matches_oracle, test_depth_backward_matches_oracle) at its smallest shape, under
    `combined` at the pose of rowwise.POSE."""
    from gpu_helpers import npy
    from gaussian_lic_amd.synthetic import pixel_grad
    kind, P, W, H, deg, seed = "random", 3000, 70, 50, 2, 5
    raw, sc, camd, cam = cv.variant_scene(kind, P, W, H, deg, seed, "combined", view=rw.POSE)
    dL = pixel_grad(H, W, seed=1)
    gD = torch.randn(H, W, generator=torch.Generator().manual_seed(11)).float()
    with _mode(True):
        f = fwd_depth(raw, cam)
        got = bwd(f, dL, gD)
        g_col = bwd(f, dL)
    ref = oracle32.forward(sc, camd)
    exp_depth, _ = oracle_depth(oracle32, ref, W, H)
    depth = npy(f["depth"])
    assert float(np.abs(depth).max()) > 0
    print(f"\ndepth: rel err {rel_err(depth, exp_depth):.2e}")
    assert rel_err(depth, exp_depth) < TOL
    exp = oracle_backward_depth(oracle32, sc, camd, ref, dL.numpy(), gD.numpy())
    vis = ref["pre"]["radii"] > 0
    errs = cv.gradient_errors(got, exp, sc)
    print("depth backward: " + "  ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    for k, e in errs.items():
        assert np.all(got[k].reshape(P, -1)[~vis] == 0), f"{k}: invisible rows must be exact zeros"
        assert e < TOL, f"{k}: max rel err {e:.3e}"
    assert rel_err(g_col["dL_dmean3D"], exp["dL_dmean3D"]) > 100 * TOL     # the depth term has teeth


# ----------------------------------------------------------------------------------------------------------------------- d. LiDAR z-buffer
MARGINS, WEIGHT = (0.1, 0.02), (0.05, 0.02, 0.25)


def _abi_images(cam, pts, W, H, r):
    """gslic_lidar_zbuffer_add + _resolve + _resolve_weighted through the C ABI: (z-buffer uint64 [H*W], plain images, weighted images) as numpy,
    the counts as ints."""
    from gaussian_lic_amd import _lib
    L, dev, N = _lib.lib(), gpu(), W * H
    R, t = lr.pose_f32(cam)
    d_p, d_R, d_t = (torch.from_numpy(np.array(a)).to(dev) for a in (pts, R, t))
    zb = torch.empty(N, dtype=torch.int64, device=dev)
    _lib.check(L.gslic_lidar_zbuffer_add(len(pts), _lib.ptr(d_p), _lib.ptr(d_R), _lib.ptr(d_t), float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy),
                                         W, H, _lib.ptr(zb), 1, 0, _lib.current_stream_ptr()))
    f32 = lambda: torch.empty(H, W, dtype=torch.float32, device=dev)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    a = dict(depth=f32(), index=i32(H, W), near=f32(), n_measured=i32(1))
    _lib.check(L.gslic_lidar_zbuffer_resolve(W, H, _lib.ptr(zb), r, MARGINS[0], MARGINS[1], _lib.ptr(a["depth"]), _lib.ptr(a["index"]), _lib.ptr(a["near"]),
                                             _lib.ptr(a["n_measured"]), _lib.current_stream_ptr()))
    b = dict(depth=f32(), index=i32(H, W), near=f32(), n_measured=i32(1), weight=f32(), dist2=i32(H, W))
    _lib.check(L.gslic_lidar_zbuffer_resolve_weighted(W, H, _lib.ptr(zb), r, MARGINS[0], MARGINS[1], *WEIGHT, _lib.ptr(b["depth"]), _lib.ptr(b["index"]),
                                                      _lib.ptr(b["near"]), _lib.ptr(b["n_measured"]), _lib.ptr(b["weight"]), _lib.ptr(b["dist2"]),
                                                      _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    host = lambda d: {k: (int(v) if k == "n_measured" else v.cpu().numpy()) for k, v in d.items()}
    return zb.cpu().numpy().view(np.uint64), host(a), host(b)


def _same_images(got, ref, ref_w=None):
    """Every image on bits, and the count."""
    for k in ("depth", "near"):
        assert np.array_equal(got[k].view(np.int32), ref[k].view(np.int32)), k
    assert np.array_equal(got["index"], ref["index"]) and int(got["n_measured"]) == ref["n_measured"]
    if ref_w is not None:
        assert np.array_equal(got["weight"].view(np.int32), ref_w["weight"].view(np.int32)) and np.array_equal(got["dist2"], ref_w["dist2"])
        assert np.array_equal(got["depth"].view(np.int32), ref_w["depth"].view(np.int32)) and np.array_equal(got["index"], ref_w["index"])
        assert int(got["n_measured"]) == ref_w["n_measured"]


@pytest.mark.parametrize("W,H", [(37, 23), (64, 64)])
@pytest.mark.parametrize("name", list(cv.CAMERAS))
def test_lidar_zbuffer_matches_reference(name, W, H):
    """Clouds and planted points built on the variant camera; 257 points from the identity pose and 4097 from se3_c; footprints 1 and 3."""
    measured = 0
    for n, view in ((257, None), (4097, "se3_c")):
        cam = cv.variant_camera(name, W, H, view)
        pts, _notes = cv.variant_cloud(name, W, H, n, view)
        ref_zb = cv.variant_zbuffer(name, W, H, n, view)
        for r in (1, 3):
            zb, plain, weighted = _abi_images(cam, pts, W, H, r)
            assert np.array_equal(zb, ref_zb), (name, n, view)
            ref = lr.resolve(ref_zb, W, H, r, *MARGINS)
            ref_w = wr.resolve_weighted(ref_zb, W, H, r, *WEIGHT)
            _same_images(plain, ref)
            _same_images(weighted, ref, ref_w)
            measured += ref["n_measured"]
    assert measured > 0


def test_lidar_depth_wrapper_hands_the_intrinsics_over():
    """trainer.LidarDepth.add reads camera.fx, camera.fy, camera.cx, camera.cy itself: one sweep through it under `combined`."""
    from gaussian_lic_amd import trainer
    W, H, n, view, r = 37, 23, 4097, "se3_c", 3
    cam = cv.variant_camera("combined", W, H, view)
    pts, _notes = cv.variant_cloud("combined", W, H, n, view)
    ld = trainer.LidarDepth(W, H, gpu())
    assert ld.add(cam, torch.from_numpy(pts.copy()).to(gpu())) == 0
    ref_zb = cv.variant_zbuffer("combined", W, H, n, view)
    assert np.array_equal(ld._zbuf.cpu().numpy().view(np.uint64), ref_zb)
    out = ld.resolve(footprint=r, margins=MARGINS, index=True, count=True, weight=WEIGHT, dist2=True)
    _same_images({k: v.cpu().numpy() for k, v in out.items()}, lr.resolve(ref_zb, W, H, r, *MARGINS), wr.resolve_weighted(ref_zb, W, H, r, *WEIGHT))
    want = cam.project_depth(torch.from_numpy(pts.copy()))
    assert torch.equal(bits(trainer.lidar_depth_image(cam, torch.from_numpy(pts.copy()).to(gpu()))).cpu(), bits(want)) and bool(want.any())


# ------------------------------------------------------------------------------------------------------------------------------- e. extend
def _frame(n, W, H, seed, cam):
    """test_extend.py's synthetic LiDAR frame in the camera frame of `cam`, moved into the world frame of its pose: (points, colours, sensor
    depths, R_cw, t_cw) as float32."""
    from test_extend import _lidar_frame
    pts, col, rsp = _lidar_frame(n, W, H, seed, float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy))
    R_wc, t_wc = np.asarray(cam.R_wc, np.float64), np.asarray(cam.t_wc, np.float64)
    world = (pts.astype(np.float64) @ R_wc.T + t_wc).astype(np.float32)
    return world, col, rsp, R_wc.T.astype(np.float32), (-R_wc.T @ t_wc).astype(np.float32)


def _check_rows(rows, exp, shape=lambda a, b: a.reshape(b.shape)):
    for key in ("xyz", "rest", "rotation"):
        np.testing.assert_array_equal(rows[key], shape(exp[key], rows[key]))       # exact: copies / constants, ascending order
    for key in ("dc", "opacity", "scaling"):
        assert rel_err(rows[key], shape(exp[key], rows[key])) < 1e-6, key


@pytest.mark.parametrize("name,view", [("aniso", None), ("combined", "se3_c")])
def test_extend_matches_oracle(oracle32, name, view):
    """gslic_extend_select / gslic_extend_emit against the oracle's extend (test_extend.py::test_extend_matches_oracle_and_appends_in_place's
    comparison) on a 70x50 image with 4000 returns: the same survivors, the same rows, and the extents of focal = (fx + fy) / 2."""
    from gpu_helpers import hip_extend_rows
    W, H, n = 70, 50, 4000
    cam = cv.variant_camera(name, W, H, view)
    fx, fy, cx, cy = (float(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy))
    pts, col, rsp, R_cw, t_cw = _frame(n, W, H, 3, cam)
    T = np.random.default_rng(1).random((H, W)).astype(np.float32)
    T[:, : W // 3] = 0.001                                  # a part of the image already opaque
    keep = oracle32.extend_select(pts, rsp, R_cw, t_cw, fx, fy, cx, cy, W, H, T)
    exp = oracle32.extend_emit(keep, pts, col, rsp, 1.0, 0.5 * (fx + fy), 15)
    k, rows = hip_extend_rows(pts, col, rsp, R_cw, t_cw, (fx, fy, cx, cy), W, H, T)
    assert k == int(keep.sum()) and k > 500
    np.testing.assert_array_equal(rows["xyz"], pts[keep])   # ascending index on both sides, distinct points: the same indices
    _check_rows(rows, exp)
    want = np.log(rsp[keep].astype(np.float64) / (0.5 * (fx + fy)))
    assert np.abs(rows["scaling"] - want[:, None]).max() < 1e-5
    assert abs(np.log(fx / (0.5 * (fx + fy)))) > 0.1        # fx or fy alone would be far outside that
    # the selection depends on which focal length goes with which axis
    assert not np.array_equal(oracle32.extend_select(pts, rsp, R_cw, t_cw, fy, fx, cx, cy, W, H, T), keep)


def test_model_extend_hands_the_intrinsics_over(oracle32):
    """Once through trainer.GaussianModel.extend under `combined`: the survivors and the appended rows are the oracle's."""
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.rasterizer import render
    W, H, P, n = 70, 50, 300, 4000   # a third of the pixels already opaque (the oracle's transmittance): about 1000 of the returns survive
    raw, sc, camd, cam = cv.variant_scene("random", P, W, H, 3, 51, "combined", view="se3_a")
    dev = gpu()
    cam.to_device(dev)
    model = trainer.GaussianModel(raw, dev)
    model.training_setup()
    fx, fy, cx, cy = (float(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy))
    pts, col, rsp, R_cw, t_cw = _frame(n, W, H, 3, cam)
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        final_T = render(cam, model, bg, no_color=True)[1].cpu().numpy()
    k = model.extend(cam, torch.from_numpy(pts).to(dev), torch.from_numpy(col).to(dev), torch.from_numpy(rsp).to(dev), torch.from_numpy(R_cw),
                     torch.from_numpy(t_cw), (fx, fy, cx, cy))
    keep = oracle32.extend_select(pts, rsp, R_cw, t_cw, fx, fy, cx, cy, W, H, final_T)
    assert k == int(keep.sum()) and k > 300 and model.P == P + k
    exp = oracle32.extend_emit(keep, pts, col, rsp, 1.0, 0.5 * (fx + fy), 15)
    rows = {key: getattr(model, attr).detach()[P:].cpu().numpy() for attr, key in (("xyz", "xyz"), ("features_dc", "dc"), ("features_rest", "rest"),
                                                                                 ("opacity", "opacity"), ("scaling", "scaling"), ("rotation", "rotation"))}
    _check_rows(rows, exp)


# --------------------------------------------------------------------------------------------------------------------- g. the C++ fused host
def test_fused_lidar_depth_cpp_host_combined(tmp_path):
    """The run of test_lidar_depth_gpu.py::test_fused_lidar_depth_cpp_host under `combined`: gslic::LidarDepth (handed fx, fy, cx, cy by the
    program) feeding FusedStep::step and accumulate_free_space gives the Python host's images, parameters, moments and accumulators, bit for bit."""
    import functools
    import fused_check_io as fio
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.synthetic import gt_image, lidar_scene
    from test_lidar_depth_gpu import LAMBDA_DEPTH, NP, NPTS, SH, SW
    exe = fio.build("fused_lidar_depth")
    dev = gpu()
    footprint, w_min = 0, trainer.ContributionStats.W_MIN
    m = trainer.GaussianModel(cv.variant_scene("random", NP, SW, SH, 3, 3, "combined")[0], dev)
    m.training_setup()
    cam = cv.variant_camera("combined", SW, SH).to_device(dev)
    gt, bg = gt_image(SH, SW).to(dev), torch.zeros(3, device=dev)
    points = cv.reproject(lidar_scene(NPTS, SW, SH, sh_degree=0, seed=21)["xyz"], SW, SH, "combined")
    R, t = lr.pose_f32(cam)
    d = str(tmp_path)
    fio.write_inputs(d, m, cam, gt=gt, points=points,
                     lidar=np.concatenate([R, t, np.array([cam.fx, cam.fy, cam.cx, cam.cy, MARGINS[0], MARGINS[1], LAMBDA_DEPTH, w_min], np.float32)]))
    ld = trainer.LidarDepth(SW, SH, dev)
    ld.add(cam, points.to(dev))
    im = ld.resolve(footprint=footprint, margins=MARGINS, index=True, count=True)
    assert torch.equal(bits(im["depth"]).cpu(), bits(cam.project_depth(points)))
    trainer.training_step_fused(m, cam, gt, bg, gt_depth=im["depth"], lambda_depth=LAMBDA_DEPTH)
    st = trainer.ContributionStats(m)
    st.accumulate(cam, w_min=w_min, free_space=im["near"])
    r = fio.run(exe, d, str(NP), str(SW), str(SH), "3", str(NPTS), str(footprint))
    assert f"lidar measured {int(im['n_measured'])} base 0" in r.stdout
    rd = functools.partial(fio.read, d)
    assert torch.equal(rd("lidar_depth.f32", np.int32), bits(im["depth"]).cpu().reshape(-1)) and int(im["n_measured"]) > 100
    assert torch.equal(rd("lidar_near.f32", np.int32), bits(im["near"]).cpu().reshape(-1))
    assert torch.equal(rd("lidar_index.i32", np.int32), im["index"].cpu().reshape(-1))
    assert int(rd("lidar_count.i32", np.int32)[0]) == int(im["n_measured"])
    P = m.P
    for n, f in (("xyz", "xyz"), ("features_dc", "dc"), ("features_rest", "rest"), ("opacity", "opacity"), ("scaling", "scaling"), ("rotation", "rotation")):
        for pre, src in (("", m._buf), ("m_", m._m), ("v_", m._v)):
            assert torch.equal(rd(pre + f + ".f32", np.int32), bits(src[n][:P]).cpu().reshape(-1)), pre + f
    assert torch.equal(rd("max_w.i32", np.int32), st._max[:P].cpu()) and torch.equal(rd("n_pix.i32", np.int32), st._npix[:P].cpu())
    assert torch.equal(rd("sum_w.i64", np.int64), st.sum_fixed().cpu())
    assert torch.equal(rd("free_sum.i64", np.int64), st.free_fixed().cpu()) and torch.equal(rd("meas_sum.i64", np.int64), st.measured_fixed().cpu())
    assert bool(st.free_fixed().any()) and bool(st.measured_fixed().any())
    st.detach()


# --------------------------------------------------------------------------------------------------------------------- f. reference kernels
@pytest.mark.parametrize("mode", ["default", "fast"])
def test_hip_matches_reference_kernels_combined(mode):
    """test_vs_reference_kernels_gpu.py::test_hip_matches_reference_kernels under `combined`: random, P = 8192 (a multiple of 256), 320x240,
    degree 3, both arithmetic modes; the same bars and the same skip when the checker library was not built."""
    from gpu_helpers import hip_backward, hip_forward, npy
    from gaussian_lic_amd import _lib
    from gaussian_lic_amd.synthetic import pixel_grad
    from oracle.ref_build import refkernels
    if not refkernels.available():
        pytest.skip("oracle/_ref/libref_hip.so not built")
    rk = refkernels.RefKernels()
    kind, P, W, H, deg, seed = "random", 8192, 320, 240, 3, cv.SEEDS[(cv.ROWWISE_SHAPE, "combined")]
    fast = mode == "fast"
    raw, sc, camd, cam = cv.variant_scene(kind, P, W, H, deg, seed, "combined")
    dL = pixel_grad(H, W, seed=1)
    ref = rk.run(sc, camd, dL.numpy())
    prev = _lib.set_math_mode(not fast)
    try:
        got = hip_forward(raw, cam, export=("tiles_touched", "means2D", "depths", "conic_opacity", "point_list", "ranges", "n_contrib"))
        g = hip_backward(got, dL)
    finally:
        _lib.set_math_mode(prev)
    d = got["dbg"]
    vis = ref["radii"] > 0
    np.testing.assert_array_equal(npy(got["radii"]), ref["radii"])
    np.testing.assert_array_equal(npy(d["tiles_touched"]).astype(np.uint32), ref["tiles_touched"])
    assert got["R"] == ref["R"] > 0
    np.testing.assert_array_equal(npy(d["point_list"]).astype(np.uint32), ref["point_list"])
    np.testing.assert_array_equal(npy(d["ranges"]).astype(np.uint32), ref["ranges"])
    np.testing.assert_array_equal(npy(d["means2D"])[vis], ref["means2D"][vis])
    np.testing.assert_array_equal(npy(d["depths"])[vis], ref["depths"][vis])
    np.testing.assert_array_equal(npy(d["conic_opacity"])[vis], ref["conic_opacity"][vis])
    names = ("dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmean3D", "dL_dcov3D", "dL_ddc", "dL_dsh", "dL_dscale")
    if fast:
        assert_close_flips(npy(got["color"]), ref["color"], TOL, "color")
        assert_close_flips(npy(got["final_T"]), ref["final_T"], TOL, "final_T")
        for k in names:
            assert_close_flips(g[k], ref[k], TOL, k, flip_bound=2e-2)
    else:
        np.testing.assert_array_equal(npy(got["color"]), ref["color"])
        np.testing.assert_array_equal(npy(got["final_T"]), ref["final_T"])
        np.testing.assert_array_equal(npy(d["n_contrib"]).astype(np.uint32), ref["n_contrib"])
        for k in names:
            assert rel_err(g[k].reshape(-1), ref[k].reshape(-1)) < TOL, k
    scale = max(np.abs(ref["dL_drot"]).max(), np.abs(ref["dL_dscale"]).max() * sc["scales"].max())
    assert np.abs(g["dL_drot"] - ref["dL_drot"]).max() / scale < TOL
