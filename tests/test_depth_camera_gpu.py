"""-m gpu: the camera-pose gradient under LiDAR depth supervision — gslic_rasterize_backward_depth_camera against the composed oracle
(depth_camera_helpers), its degenerate cases, trainer.pose_gradient / training_step_with_pose with gt_depth, and the C++ host's
gslic::FusedStep::pose_gradient(cam, gt, gt_depth, lambda_depth)."""
import numpy as np
import pytest
import torch

import fused_check_io as fio
from conftest import make_scene
from depth_camera_helpers import CAM, GRADS, oracle_backward_depth_camera, oracle_depth
from gpu_helpers import gpu
from test_depth_gpu import DEPTH_CASES, POSE

pytestmark = pytest.mark.gpu

# the three scenes of test_depth_gpu.DEPTH_CASES at the general pose POSE (row 2 of V differs from column 2, V[2] and V[6] non-zero), and
# one with P < 64 (a single, partly filled wave on the generic 256-thread path)
CASES = [c + (POSE,) for c in DEPTH_CASES] + [("random", 40, 64, 48, 1, 5, POSE)]
CAM_TOL = 2e-4      # of max-abs per output: the bar test_camera_grad.py holds the colour camera gradient to
# Fast arithmetic against strict arithmetic.  Measured gap max|fast - strict| / max|strict| of gslic_rasterize_backward_camera (the colour-only
# camera backward, whose kernels this change leaves instruction for instruction as they were) on the four CASES, forward and backward in the
# mode: dL_dviewmatrix 2.8e-6 / 9.6e-7 / 1.5e-7 / 6.1e-7, dL_dprojmatrix 7.7e-7 / 5.0e-7 / 3.6e-7 / 5.7e-7,
# dL_dcampos 3.5e-7 / 2.4e-7 / 0 / 6.0e-7  ->  largest 2.775e-6; the bound is twice that.
FAST_GAP_MEASURED = 2.775e-6
FAST_TOL = 2 * FAST_GAP_MEASURED


class _mode:
    """gslic_set_math_mode for the duration of a block (strict = the default)."""

    def __init__(self, strict):
        self.strict = strict

    def __enter__(self):
        from gaussian_lic_amd import _lib
        self.prev = _lib.set_math_mode(self.strict)

    def __exit__(self, *a):
        from gaussian_lic_amd import _lib
        _lib.set_math_mode(self.prev)


def _fwd_depth(raw, cam):
    from gpu_helpers import settings_from
    from gaussian_lic_amd import rasterizer as rz
    from gaussian_lic_amd.synthetic import activate
    dev = gpu()
    t = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in activate(raw).items()}
    rs = settings_from(cam, t["D"], dev)
    out = rz.rasterize_gaussians_depth(rs.bg, t["means"], t["opac"], t["scales"], t["rots"], rs.scale_modifier, rs.viewmatrix, rs.projmatrix,
                                      rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, rs.limx_neg, rs.limx_pos, rs.limy_neg, rs.limy_pos,
                                      t["dc"], t["shs"], t["D"], rs.campos)
    R, B, color, final_T, depth, radii, geom, binning, img, sample = out
    torch.cuda.synchronize()
    return dict(R=R, B=B, color=color, depth=depth, radii=radii, bufs=(geom, binning, img, sample), t=t, rs=rs)


def _bwd(f, dL_dpix, dL_ddepth, camera=True):
    """gslic_rasterize_backward_depth_camera (camera=True) / gslic_rasterize_backward_depth on f's buffers; dL_ddepth None: the colour-only
    gslic_rasterize_backward_camera.  Returns the tuple of device tensors."""
    from gaussian_lic_amd import rasterizer as rz
    t, rs = f["t"], f["rs"]
    dev = gpu()
    geom, binning, img, sample = f["bufs"]
    if dL_ddepth is None:
        e = torch.empty(0, device=dev)
        g = rz.rasterize_gaussians_backward(rs.bg, t["means"], f["radii"], e, t["scales"], t["rots"], rs.scale_modifier, e, rs.viewmatrix,
                                            rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.limx_neg, rs.limx_pos, rs.limy_neg, rs.limy_pos,
                                            dL_dpix.to(dev), t["dc"], t["shs"], t["D"], rs.campos, geom, f["R"], binning, img, f["B"], sample,
                                            0.0, False, camera_grads=camera)
    else:
        g = rz.rasterize_gaussians_backward_depth(rs.bg, t["means"], f["radii"], t["scales"], t["rots"], rs.scale_modifier, rs.viewmatrix,
                                                  rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.limx_neg, rs.limx_pos, rs.limy_neg, rs.limy_pos,
                                                  dL_dpix.to(dev), dL_ddepth.to(dev), t["dc"], t["shs"], t["D"], rs.campos, geom, f["R"], binning,
                                                  img, f["B"], sample, camera_grads=camera)
    torch.cuda.synchronize()
    return g


def _grads(H, W):
    from gaussian_lic_amd.synthetic import pixel_grad
    return pixel_grad(H, W, seed=1), torch.randn(H, W, generator=torch.Generator().manual_seed(11)).float()


def _rel(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max()) / max(float(np.abs(ref).max()), 1e-30)


# ------------------------------------------------------------------------------------------------------------------ 4. against the oracle
@pytest.mark.parametrize("kind,P,W,H,deg,seed,view", CASES)
def test_depth_camera_gradient_matches_oracle(oracle32, kind, P, W, H, deg, seed, view):
    raw, sc, camd, cam = make_scene(kind, P, W, H, deg, seed, view=view)
    dL, gD = _grads(H, W)
    with _mode(True):
        f = _fwd_depth(raw, cam)
        out = _bwd(f, dL, gD)
        plain = _bwd(f, dL, gD, camera=False)
        again = _bwd(f, dL, gD)
    assert len(out) == 12 and len(plain) == 9
    ref_f = oracle32.forward(sc, camd)
    exp = oracle_backward_depth_camera(oracle32, sc, camd, ref_f, dL.numpy(), gD.numpy())
    # the direct term is material here: a kernel that dropped it would miss the bar below
    assert np.abs(exp["direct"]).max() >= 1e-2 * np.abs(exp["dL_dviewmatrix"][[2, 6, 10, 14]]).max()
    for a, b, n in zip(out[:9], plain, GRADS):   # the nine ordinary gradients: another instantiation of the chain kernel (fma contraction may differ)
        if a.numel():
            d = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)
            print(f"[{kind} P={P}] {n}: vs gslic_rasterize_backward_depth {d:.3e}")
            assert d <= 1e-5, (n, d)
    for got, name in zip(out[9:], CAM):
        r = np.asarray(exp[name], np.float64)
        g = got.cpu().numpy().astype(np.float64)
        print(f"[{kind} P={P}] {name}: rel err vs oracle {_rel(g, r):.3e}")
        assert _rel(g, r) < CAM_TOL, (name, g, r)
        assert np.all(g[r == 0.0] == 0.0)
    g = out[9].cpu().numpy()
    assert np.all(g[[3, 7, 11, 15]] == 0.0) and np.all(out[10].cpu().numpy()[[2, 6, 10, 14]] == 0.0)   # view row 3, projection row 2
    for a, b in zip(out, again):   # 8a. run-to-run bit reproducibility (fixed-order reduction, no atomics)
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------ 5. fast arithmetic
@pytest.mark.parametrize("kind,P,W,H,deg,seed,view", CASES)
def test_depth_camera_gradient_fast_mode(kind, P, W, H, deg, seed, view):
    """gslic_set_math_mode(0) against the strict-mode result of the same call (forward and backward in the mode).  Bound: twice the largest gap
    measured for the colour-only camera backward on the same scenes (FAST_TOL above; the depth channel adds one more flipped-cut-off pathway
    per pair)."""
    raw, sc, camd, cam = make_scene(kind, P, W, H, deg, seed, view=view)
    dL, gD = _grads(H, W)
    with _mode(True):
        strict = _bwd(_fwd_depth(raw, cam), dL, gD)
    with _mode(False):
        fast = _bwd(_fwd_depth(raw, cam), dL, gD)
    for a, b, name in zip(fast[9:], strict[9:], CAM):
        d = _rel(a.cpu().numpy(), b.cpu().numpy())
        print(f"[{kind} P={P}] {name}: fast vs strict {d:.3e}")
        assert d <= FAST_TOL, (name, d)


# ------------------------------------------------------------------------------------------------------------------ 6. / 7. degenerate inputs
@pytest.mark.parametrize("strict", [True, False])
def test_zero_depth_gradient_is_the_colour_camera_backward(strict):
    W, H = 330, 250
    raw, sc, camd, cam = make_scene("random", 20000, W, H, 3, 3, view=POSE)
    dL, _ = _grads(H, W)
    with _mode(strict):
        f = _fwd_depth(raw, cam)
        zero = _bwd(f, dL, torch.zeros(H, W))
        colour = _bwd(f, dL, None)
    assert len(zero) == len(colour) == 12
    for a, b, n in zip(zero, colour, GRADS + CAM):
        assert torch.equal(a, b), n
    assert bool(zero[9].any())


def test_depth_only_gradient_reaches_view_and_projection_not_campos():
    W, H = 320, 240
    raw, sc, camd, cam = make_scene("random", 20000, W, H, 3, 8, view=POSE)
    _, gD = _grads(H, W)
    f = _fwd_depth(raw, cam)
    out = _bwd(f, torch.zeros(3, H, W), gD)
    dV, dP, dC = (t.cpu().numpy() for t in out[9:])
    assert np.all(dC == 0.0)
    assert np.all(dV[[2, 6, 10, 14]] != 0.0) and np.any(dP != 0.0)


def test_empty_map_gives_zero_camera_gradients():
    from gaussian_lic_amd import rasterizer as rz
    dev = gpu()
    W, H = 64, 48
    z = lambda *s: torch.zeros(*s, device=dev)
    e8 = torch.empty(0, dtype=torch.uint8, device=dev)
    out = rz.rasterize_gaussians_backward_depth(z(3), z(0, 3), torch.zeros(0, dtype=torch.int32, device=dev), z(0, 3), z(0, 4), 1.0, z(16), z(16), 1.0,
                                                1.0, -1.0, 1.0, -1.0, 1.0, z(3, H, W), z(H, W), z(0, 1, 3), z(0, 15, 3), 3, z(3), e8, 0, e8, e8, 0, e8,
                                                camera_grads=True)
    assert len(out) == 12 and all(not bool(t.any()) for t in out[9:])
    # the C entry point itself: P == 0 zeroes the three outputs
    import ctypes
    from gaussian_lic_amd import _lib
    L = _lib.lib()
    cam = [torch.full((n,), 7.0, device=dev) for n in (16, 16, 3)]
    prm = _lib.RasterParams(0, 3, 15, W, H, 1.0, 1.0, -1, 1, -1, 1, 1.0, 0, 0, 0, 0)
    rc = L.gslic_rasterize_backward_depth_camera(ctypes.byref(prm), 0, 0, *([None] * 12), *([None] * 4), None, None, *([None] * 10), 0.0,
                                                 *[ctypes.c_void_p(t.data_ptr()) for t in cam], _lib.current_stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and all(not bool(t.any()) for t in cam)


def test_depth_camera_backward_refuses_buffers_of_a_plain_forward():
    from gpu_helpers import hip_forward
    from gaussian_lic_amd import _lib
    raw, sc, camd, cam = make_scene("random", 2000, 96, 64, 3, 2)
    a = hip_forward(raw, cam)
    f = dict(R=a["R"], B=a["B"], radii=a["radii"], bufs=a["bufs"], t=a["act"], rs=a["rs"])
    with pytest.raises(_lib.GslicError, match="rendered no depth"):
        _bwd(f, torch.zeros(3, 64, 96), torch.ones(64, 96))


# ------------------------------------------------------------------------------------------------------------------ 8b. capacity overflow
def test_overflowed_depth_forward_leaves_zero_camera_gradients():
    """After a capacity-mode depth forward that overflowed (a reported status, not a fault) nothing of the step is valid: the per-Gaussian outputs are
    left untouched and the three camera outputs are exact zeros — the launch's memset, with no partial row summed.  The geometry buffer is the
    one a completed step has just used, so its scratch holds that step's partial rows: they must not reach the outputs.  (The colour-only
    gslic_rasterize_backward_camera zeroes its outputs the same way and then adds whatever rows the scratch holds: zeros on a fresh scratch.)"""
    from gaussian_lic_amd import rasterizer as rz
    from gaussian_lic_amd.synthetic import activate
    dev = gpu()
    P, W, H = 20000, 320, 240
    raw, sc, camd, cam = make_scene("random", P, W, H, 3, 6, view=POSE)
    cam.to_device(dev)
    act = {k: (v.to(dev).contiguous() if torch.is_tensor(v) else v) for k, v in activate(raw).items()}
    scal = (float(cam.tanfovx), float(cam.tanfovy), float(cam.limx_neg), float(cam.limx_pos), float(cam.limy_neg), float(cam.limy_pos))
    bg = torch.zeros(3, device=dev)
    dL, gD = _grads(H, W)
    dL, gD = dL.to(dev), gD.to(dev)
    vm, pm, cp = cam.d_world_view_transform, cam.d_full_proj_transform, cam.d_camera_center

    def forward(bufs):
        return rz.rasterize_gaussians_depth_capacity(bufs, bg, act["means"], act["opac"], act["scales"], act["rots"], 1.0, vm, pm, *scal, act["dc"],
                                                     act["shs"], act["D"], cp)

    def backward(fw, out):
        cR, cB, _c, _T, _d, radii, geom, binning, img, sample = fw
        return rz.rasterize_gaussians_backward_depth(bg, act["means"], radii, act["scales"], act["rots"], 1.0, vm, pm, *scal, dL, gD, act["dc"],
                                                     act["shs"], act["D"], cp, geom, cR, binning, img, cB, sample, 0.0, False, out=out,
                                                     camera_grads=True)

    mk_out = lambda: {k: torch.full(s, 7.0, device=dev) for k, s in (("xyz", (P, 3)), ("features_dc", (P, 1, 3)), ("features_rest", (P, 15, 3)),
                                                                      ("opacity", (P, 1)), ("scaling", (P, 3)), ("rotation", (P, 4)))}
    big = rz.CapacityBuffers(P, W, H, 2_000_000, 100_000, dev, depth=True)
    good = backward(forward(big), mk_out())
    R, B, bits, done = big.read_status()
    assert bits == 0 and done == 1 and bool(good[9].any())
    for cap_R, cap_B, bit in ((R // 2, B + 100, 1), (R + 1000, B // 2, 2)):
        small = rz.CapacityBuffers(P, W, H, cap_R, cap_B, dev, depth=True)
        small.geom = big.geom                      # (sized by P alone) the scratch with the completed step's partial rows
        fw = forward(small)
        out = mk_out()
        res = backward(fw, out)
        torch.cuda.synchronize()
        _r, _b, bits, done = small.read_status()
        assert bits & bit and done == 0, (cap_R, cap_B, bits)
        for k, t in out.items():
            assert bool((t == 7.0).all()), f"{k} was written although the forward had overflowed"
        for t, n in zip(res[9:], CAM):
            assert not bool(t.any()), f"{n}: stale partial rows were summed after an overflowed forward"


# ------------------------------------------------------------------------------------------------------------------ 9. / 10. the trainer
LAMBDA_D = 0.1


def _pose_case(view, P, W, H):
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.rasterizer import render
    from gaussian_lic_amd.synthetic import gt_image
    raw, sc, _camd, _cam = make_scene("random", P, W, H, 3, 12)
    dev = gpu()
    cam = synthetic_camera(W, H, view).to_device(dev)
    model = trainer.GaussianModel(raw, dev)
    gt, bg = gt_image(H, W).to(dev), torch.zeros(3, device=dev)
    # the depth target: the scene rendered from a pose displaced 0.1 m along the optical axis, so that the depth residual has one sign almost
    # everywhere and the depth term, not the colour term, dominates dL/drho_z
    cam_t = synthetic_camera(W, H, view)
    cam_t.apply_pose_increment([0.0, 0.0, 0.1, 0.0, 0.0, 0.0]).to_device(dev)
    with torch.no_grad():
        gtd = render(cam_t, model, bg, return_depth=True)[5].detach().clone().contiguous()
    assert int((gtd > 0).sum()) > 1000
    return raw, sc, cam, model, gt, gtd, bg


def _total(terms):
    return 0.8 * float(terms[0]) + 0.2 * (1.0 - float(terms[1])) + LAMBDA_D * float(terms[2])


@pytest.mark.parametrize("view,P,W,H", [(0, 20000, 320, 240), (7, 3000, 160, 120)])
def test_depth_pose_gradient_matches_oracle_and_descends(oracle32, view, P, W, H):
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    raw, sc, cam, model, gt, gtd, bg = _pose_case(view, P, W, H)
    dev = gpu()
    camd = cam.as_dict()
    g, terms = trainer.pose_gradient(model, cam, gt, bg, gt_depth=gtd, lambda_depth=LAMBDA_D)
    g_col, terms_col = trainer.pose_gradient(model, cam, gt, bg)
    assert terms.numel() == 3 and terms_col.numel() == 2 and float(terms[2]) > 0
    # the oracle on the same loss: dL/dimage and dL/ddepth from the loss kernels' definitions, the composed camera gradient, the same chain
    f = oracle32.forward(sc, camd)
    n = float(f["color"].size)
    gtn, gtdn = gt.cpu().numpy(), gtd.cpu().numpy()
    m, d1, d2, d3 = oracle32.ssim_forward(f["color"][None], gtn[None])
    dL = (0.8 / n) * np.sign(f["color"] - gtn).astype(np.float32) + oracle32.ssim_backward(f["color"][None], gtn[None], np.full_like(m, -0.2 / n), d1, d2, d3)[0]
    depth, _ = oracle_depth(oracle32, f, W, H)
    mask = gtdn > 0
    dLd = np.where(mask, (LAMBDA_D / max(int(mask.sum()), 1)) * np.sign(depth - gtdn), 0.0).astype(np.float32)
    ref = oracle_backward_depth_camera(oracle32, sc, camd, f, dL, dLd)
    want = cam.pose_gradient(ref["dL_dviewmatrix"], ref["dL_dprojmatrix"], ref["dL_dcampos"])
    print(f"view {view}: with depth {g}\n colour only {g_col}\n oracle {want}")
    assert float(np.abs(g - want).max()) <= 2e-3 * max(float(np.abs(want).max()), 1e-30), (g, want)
    # the depth term moves the component along the optical axis (by far more than the bar above)
    assert abs(g[2] - g_col[2]) > 2e-2 * float(np.abs(g).max()), (g, g_col)
    # the joint map + pose step: the same camera gradient, and the map update of training_step_fused(gt_depth=...) on a twin model
    model_b = trainer.GaussianModel(raw, dev); model_b.training_setup()
    model_c = trainer.GaussianModel(raw, dev); model_c.training_setup()
    cam_b = synthetic_camera(W, H, view).to_device(dev)
    t_b, v_b, g_joint = trainer.training_step_with_pose(model_b, cam_b, gt, bg, pose_lr=0.0, gt_depth=gtd, lambda_depth=LAMBDA_D)
    t_c, v_c = trainer.training_step_fused(model_c, cam, gt, bg, adam_in_backward=False, gt_depth=gtd, lambda_depth=LAMBDA_D)
    assert float(np.abs(g_joint - g).max()) <= 1e-5 * max(float(np.abs(g).max()), 1e-30)
    assert torch.equal(v_b, v_c) and torch.equal(t_b, t_c)
    # (the camera instantiation of the chain kernel: gradients to 1e-5 of max-abs, as test_camera_grad.py allows between instantiations.  The first
    # Adam step from zero moments is lr (1 - b1) g / (sqrt(1 - b2) |g| + eps) = +-3.17 lr wherever |g| >> eps: the updated parameters agree except
    # where a gradient at rounding level changes sign, and never differ by more than two such steps.)
    for name, gb, gc in zip(model_b.NAMES, model_b._grad_slab.grads(model_b), model_c._grad_slab.grads(model_c)):
        if gb.numel():
            assert float((gb - gc).abs().max()) <= 1e-5 * max(float(gc.abs().max()), 1e-30), name
    lrs = dict(zip(model_b.NAMES, model_b.optimizer.lrs))
    for name in model_b.NAMES:
        pb, pc, p0 = getattr(model_b, name).detach(), getattr(model_c, name).detach(), getattr(model, name).detach()
        if not pb.numel():
            continue
        assert not torch.equal(pb, p0), name                                       # the map was updated ...
        diff = (pb - pc).abs()
        assert float(diff.max()) <= 2 * 3.17 * lrs[name] * 1.01, (name, float(diff.max()))   # ... as the fused depth step updates it
        assert float((diff > 0.01 * 3.17 * lrs[name]).float().mean()) < 1e-3, name
    loss0 = _total(terms)
    step = 1e-3 / max(float(np.linalg.norm(g)), 1e-30)            # a 1e-3 (m, rad) move along -gradient
    cam.apply_pose_increment(-step * g).to_device(dev)
    _g2, terms2 = trainer.pose_gradient(model, cam, gt, bg, gt_depth=gtd, lambda_depth=LAMBDA_D)
    assert _total(terms2) < loss0, (loss0, _total(terms2))


def test_pose_gradient_without_depth_is_the_colour_only_path():
    """gt_depth=None, or lambda_depth=0: what the colour-only entry point gives (forward, loss kernels, gslic_rasterize_backward_camera, the chain)."""
    from gaussian_lic_amd import rasterizer as rz
    from gaussian_lic_amd import trainer
    raw, sc, cam, model, gt, gtd, bg = _pose_case(7, 3000, 160, 120)
    g_none, t_none = trainer.pose_gradient(model, cam, gt, bg, gt_depth=None, lambda_depth=LAMBDA_D)
    g_zero, t_zero = trainer.pose_gradient(model, cam, gt, bg, gt_depth=gtd, lambda_depth=0.0)
    e = torch.empty(0, device=gpu())
    fl = trainer._default_fused_loss()
    with torch.no_grad():
        xyz, dc, rest = model.xyz.detach(), model.features_dc.detach(), model.features_rest.detach()
        op, scl, rot = model.opacity.detach(), model.scaling.detach(), model.rotation.detach()
        scal = (float(cam.tanfovx), float(cam.tanfovy))
        lims = (float(cam.limx_neg), float(cam.limx_pos), float(cam.limy_neg), float(cam.limy_pos))
        (R, B, image, _T, radii, geom, binning, img, sample) = rz.rasterize_gaussians(
            bg, xyz, e, op, scl, rot, 1.0, e, cam.d_world_view_transform, cam.d_full_proj_transform, *scal, cam.image_height, cam.image_width, *lims,
            dc, rest, model.sh_degree, cam.d_camera_center, False, False, False, raw_params=True)
        dL, terms = fl.forward_backward(image, gt)
        terms = terms.clone()
        out = rz.rasterize_gaussians_backward(bg, xyz, radii, e, scl, rot, 1.0, e, cam.d_world_view_transform, cam.d_full_proj_transform, *scal, *lims,
                                              dL, dc, rest, model.sh_degree, cam.d_camera_center, geom, R, binning, img, B, sample, model.lambda_erank,
                                              False, raw_params=True, camera_grads=True)
    want = cam.pose_gradient(out[9], out[10], out[11])
    assert np.array_equal(g_none, want) and np.array_equal(g_zero, want)
    assert t_none.numel() == 2 and torch.equal(t_none, terms) and torch.equal(t_zero, terms)


# ------------------------------------------------------------------------------------------------------------------ the C++ host
def test_fused_cpp_host_depth_pose_gradient(tmp_path):
    """gslic::FusedStep::pose_gradient(cam, gt, gt_depth, lambda_depth) (C++: depth forward, colour and depth loss calls,
    gslic_rasterize_backward_depth_camera, the se(3) chain on the host) against trainer.pose_gradient(gt_depth=...): the six numbers agree to
    1e-5 of max-abs, the bar test_shim_gpu.py::test_fused_cpp_host_pose_gradient holds the colour-only pair to; the three terms to float printing.
    The driver is built when missing (a build failure fails)."""
    from gaussian_lic_amd import trainer
    exe = fio.build("fused_depth_pose")
    P, W, H, deg = 20000, 320, 240, 3
    raw, sc, cam, model, gt, gtd, bg = _pose_case(7, P, W, H)
    d = str(tmp_path)
    fio.write_inputs(d, raw, cam, gt=gt, gt_depth=gtd)
    r = fio.run(exe, d, str(P), str(W), str(H), str(deg), repr(LAMBDA_D))
    line = lambda key: np.array([float(v) for v in [l for l in r.stdout.splitlines() if l.startswith(key)][-1].split()[1:]])
    got, got_terms = line("pose_gradient"), line("terms")
    want, terms = trainer.pose_gradient(model, cam, gt, bg, gt_depth=gtd, lambda_depth=LAMBDA_D)
    print(f"C++ {got}\nPython {want}")
    assert float(np.abs(got - want).max()) <= 1e-5 * max(float(np.abs(want).max()), 1e-30), (got, want)
    assert np.allclose(got_terms, terms.cpu().numpy(), rtol=1e-5)
