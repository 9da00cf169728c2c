"""-m gpu: LiDAR depth supervision on the fused single-GPU step — the depth loss kernel (gslic_depth_l1_loss_forward_backward), the fused-Adam
depth backward (gslic_rasterize_backward_depth_adam), the capacity-mode depth forward (gslic_rasterize_forward_depth_capacity),
trainer.training_step_fused / GraphedStep with gt_depth, and the C++ host's gslic::FusedStep::step with a depth target."""
import numpy as np
import pytest
import torch

import fused_check_io as fio
from conftest import make_scene
from gpu_helpers import assert_same_state, gpu, model_state, training_model

pytestmark = pytest.mark.gpu

# a general SE(3) pose (scene moved rigidly into its frame): row 2 of the view matrix is not its column 2
POSE = dict(ypr=(25.0, -12.0, 8.0), t=(0.4, -0.3, 0.6), place=True)
LAMBDA_D = 0.5


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


def _lidar_target(raw, cam, scale=1.1, stride=5):
    """A sparse LiDAR depth image: every stride-th point of the scene, pushed out to `scale` times its distance, projected (Camera.project_depth)."""
    pts = raw["xyz"][::stride].float() * scale
    return cam.project_depth(pts).to(gpu())


def _setup(kind, P, W, H, deg, seed, view=None):
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd.synthetic import gt_image
    raw, sc, camd, cam = make_scene(kind, P, W, H, deg, seed, view=view)
    dev = gpu()
    cam.to_device(dev)
    gtd = _lidar_target(raw, cam)
    assert int((gtd > 0).sum()) > 100
    return raw, cam, gt_image(H, W, seed=seed).to(dev), gtd, torch.zeros(3, device=dev)


# ---------------------------------------------------------------------------------------------------- 1. the loss kernel
@pytest.mark.parametrize("H,W", [(240, 320), (77, 131), (1, 5000)])
def test_depth_loss_kernel_matches_autograd(H, W):
    from gaussian_lic_amd import loss
    dev = gpu()
    g = torch.Generator().manual_seed(H * 7 + W)
    depth = (torch.rand(H, W, generator=g) * 10.0).to(dev)
    gt = (torch.rand(H, W, generator=g) * 10.0)
    gt[torch.rand(H, W, generator=g) < 0.6] = 0.0                         # unmeasured pixels
    gt = gt.to(dev)
    eq = (torch.rand(H, W, generator=g) < 0.05).to(dev) & (gt > 0)
    depth = torch.where(eq, gt, depth)                                    # sign(0) = 0 on some measured pixels
    for lam in (LAMBDA_D, 1.0, 0.03):
        d = depth.clone().requires_grad_(True)
        (lam * loss.depth_l1(d, gt)).backward()
        ref_term = float(loss.depth_l1(depth, gt))
        fl = loss.FusedLoss(0.2)
        dL, term = fl.depth_forward_backward(depth, gt, lam)
        assert torch.equal(dL, d.grad), lam
        assert abs(float(term) - ref_term) <= 1e-6 * abs(ref_term)
        t1 = term.clone()
        dL2, term2 = fl.depth_forward_backward(depth, gt, lam)
        assert torch.equal(t1, term2) and torch.equal(dL2, d.grad)
    # no measurement at all: term 0, zero gradient
    fl = loss.FusedLoss(0.2)
    dL, term = fl.depth_forward_backward(depth, torch.zeros_like(gt), 1.0)
    assert float(term) == 0.0 and not bool(dL.any())


# ---------------------------------------------------------------------------------------------------- 2. fused Adam is bit-identical
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("kind,P,W,H,deg,seed,view", [("random", 25000, 320, 240, 3, 71, None), ("lidar", 20000, 640, 480, 0, 72, None),
                                                      ("random", 20000, 320, 240, 3, 73, POSE)])
def test_fused_depth_adam_is_bit_identical(strict, kind, P, W, H, deg, seed, view):
    from gaussian_lic_amd import trainer
    raw, cam, gt, gtd, bg = _setup(kind, P, W, H, deg, seed, view)
    with _mode(strict):
        a, b = training_model(raw), training_model(raw)
        for _ in range(4):
            ta, va = trainer.training_step_fused(a, cam, gt, bg, gt_depth=gtd, lambda_depth=LAMBDA_D, adam_in_backward=True)
            tb, vb = trainer.training_step_fused(b, cam, gt, bg, gt_depth=gtd, lambda_depth=LAMBDA_D, adam_in_backward=False)
            assert torch.equal(va, vb) and bool(va.any())
            assert ta.numel() == 3 and torch.equal(ta, tb)
    assert_same_state(model_state(a), model_state(b))


# ---------------------------------------------------------------------------------------------------- 3. against the autograd depth step
@pytest.mark.parametrize("strict", [True, False])
def test_fused_depth_step_matches_autograd_depth_step(strict):
    from gaussian_lic_amd import trainer
    raw, cam, gt, gtd, bg = _setup("random", 30000, 320, 240, 3, 61)
    with _mode(strict):
        a, b = training_model(raw), training_model(raw)
        loss, vis = trainer.training_step(a, cam, gt, bg, do_step=False, raw_render=False, gt_depth=gtd, lambda_depth=LAMBDA_D)
        ref = [p.grad.clone() for p in a.parameters()]
        captured = {}
        b.optimizer.step = lambda grads=None: captured.setdefault("g", [g.clone() for g in grads])
        terms, vis2 = trainer.training_step_fused(b, cam, gt, bg, adam_in_backward=False, gt_depth=gtd, lambda_depth=LAMBDA_D)
    assert torch.equal(vis, vis2)
    fl = trainer._default_fused_loss()
    assert terms.numel() == 3 and float(terms[2]) > 0
    assert abs(float(fl.value(terms, LAMBDA_D)) - float(loss)) < 2e-6
    for name, g_ref, g in zip(a.NAMES, ref, captured["g"]):
        scale = float(g_ref.abs().max())
        if name == "rotation":
            scale = max(scale, 1e-6)
        err = float((g.reshape(g_ref.shape) - g_ref).abs().max()) / max(scale, 1e-30)
        assert err < 5e-5, (name, err)


# ---------------------------------------------------------------------------------------------------- 4. off means off
@pytest.mark.parametrize("adam_in_backward", [True, False])
def test_depth_off_is_the_colour_only_fused_step(adam_in_backward):
    from gaussian_lic_amd import trainer
    raw, cam, gt, gtd, bg = _setup("random", 20000, 320, 240, 3, 62)
    ref, none_, zero = training_model(raw), training_model(raw), training_model(raw)
    for _ in range(3):
        t0, v0 = trainer.training_step_fused(ref, cam, gt, bg, adam_in_backward=adam_in_backward)
        t1, v1 = trainer.training_step_fused(none_, cam, gt, bg, adam_in_backward=adam_in_backward, gt_depth=None, lambda_depth=LAMBDA_D)
        t2, v2 = trainer.training_step_fused(zero, cam, gt, bg, adam_in_backward=adam_in_backward, gt_depth=gtd, lambda_depth=0.0)
        assert t0.numel() == t1.numel() == t2.numel() == 2
        assert torch.equal(v0, v1) and torch.equal(v0, v2)
    s = model_state(ref)
    assert_same_state(s, model_state(none_))
    assert_same_state(s, model_state(zero))


# ---------------------------------------------------------------------------------------------------- 5. capacity-mode depth forward
def _fwd_args(m, cam):
    xyz, dc, rest = m.xyz.detach(), m.features_dc.detach(), m.features_rest.detach()
    op, sc, rot = m.opacity.detach(), m.scaling.detach(), m.rotation.detach()
    scal = (float(cam.tanfovx), float(cam.tanfovy), float(cam.limx_neg), float(cam.limx_pos), float(cam.limy_neg), float(cam.limy_pos))
    return xyz, dc, rest, op, sc, rot, scal


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("kind,P,W,H,deg,seed,view", [("random", 25000, 320, 240, 3, 81, None), ("lidar", 30000, 640, 480, 3, 82, POSE)])
def test_capacity_depth_forward_is_the_depth_forward(strict, kind, P, W, H, deg, seed, view):
    from gaussian_lic_amd import rasterizer as rz
    raw, cam, gt, gtd, bg = _setup(kind, P, W, H, deg, seed, view)
    m = training_model(raw)
    xyz, dc, rest, op, sc, rot, scal = _fwd_args(m, cam)
    with _mode(strict), torch.no_grad():
        R, B, color, final_T, depth, radii = rz.rasterize_gaussians_depth(
            bg, xyz, op, sc, rot, 1.0, cam.d_world_view_transform, cam.d_full_proj_transform, scal[0], scal[1], H, W, *scal[2:], dc, rest, deg,
            cam.d_camera_center, raw_params=True)[:6]
        bufs = rz.CapacityBuffers(P, W, H, R + 1000, B + 100, gpu(), depth=True)
        cR, cB, c2, T2, d2, r2 = rz.rasterize_gaussians_depth_capacity(bufs, bg, xyz, op, sc, rot, 1.0, cam.d_world_view_transform,
                                                                       cam.d_full_proj_transform, *scal, dc, rest, deg, cam.d_camera_center,
                                                                       raw_params=True)[:6]
        r_, b_, bits, good = bufs.read_status()
    assert cR >= R + 1000 and cB >= B + 100
    assert (r_, b_, bits, good) == (R, B, 0, 1)
    for x, y in ((color, c2), (final_T, T2), (depth, d2), (radii, r2)):
        assert torch.equal(x, y)


def test_capacity_depth_overflow_is_a_noop():
    """Too small a depth capacity: the status words report it, nothing is written out of bounds and the fused depth backward leaves parameters and
    moments untouched."""
    from gaussian_lic_amd import rasterizer as rz
    from gaussian_lic_amd.loss import FusedLoss
    raw, cam, gt, gtd, bg = _setup("random", 25000, 320, 240, 3, 83)
    P, W, H = 25000, 320, 240
    m = training_model(raw)
    m.optimizer.fused_descriptor()   # (creates the zero moments)
    before = model_state(m)
    xyz, dc, rest, op, sc, rot, scal = _fwd_args(m, cam)
    fl = FusedLoss(0.2)
    with torch.no_grad():
        R, B = rz.rasterize_gaussians_depth(bg, xyz, op, sc, rot, 1.0, cam.d_world_view_transform, cam.d_full_proj_transform, scal[0], scal[1], H, W,
                                            *scal[2:], dc, rest, 3, cam.d_camera_center, raw_params=True)[:2]
    assert R > 4000 and B > 8
    for cap_R, cap_B, bit in ((R // 4, B + 100, 1), (R + 1000, B // 4, 2)):
        bufs = rz.CapacityBuffers(P, W, H, cap_R, cap_B, gpu(), depth=True)
        with torch.no_grad():
            (cR, cB, image, _T, depth, radii, geom, binning, img, sample) = rz.rasterize_gaussians_depth_capacity(
                bufs, bg, xyz, op, sc, rot, 1.0, cam.d_world_view_transform, cam.d_full_proj_transform, *scal, dc, rest, 3, cam.d_camera_center,
                raw_params=True)
            dL, _ = fl.forward_backward(image, gt)
            dLd, _ = fl.depth_forward_backward(depth, gtd, LAMBDA_D)
            rz.rasterize_gaussians_backward_depth(bg, xyz, radii, sc, rot, 1.0, cam.d_world_view_transform, cam.d_full_proj_transform, *scal, dL, dLd,
                                                  dc, rest, 3, cam.d_camera_center, geom, cR, binning, img, cB, sample, 0.0, False, raw_params=True,
                                                  adam=m.optimizer.fused_descriptor())
        _r, _b, bits, good = bufs.read_status()
        assert bits & bit and good == 0, (cap_R, cap_B, bits)
        assert_same_state(before, model_state(m))


# ---------------------------------------------------------------------------------------------------- 6. GraphedStep with depth
@pytest.mark.parametrize("use_graph", [False, True])
def test_graphed_depth_step_equals_eager_depth_steps(use_graph):
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import gt_image
    raw, cam, gt, gtd, bg = _setup("random", 30000, 320, 240, 3, 91)
    W, H = 320, 240
    cams = [synthetic_camera(W, H, k).to_device(gpu()) for k in range(3)]
    gts = [gt_image(H, W, seed=40 + k).to(gpu()) for k in range(3)]
    gtds = [_lidar_target(raw, c, scale=1.05 + 0.05 * k) for k, c in enumerate(cams)]
    a, b = training_model(raw), training_model(raw)
    gs = trainer.GraphedStep(a, cams[0], gts[0], bg, use_graph=use_graph, gt_depth=gtds[0], lambda_depth=LAMBDA_D)
    eager_terms, graphed_terms = [], []
    for k in (0, 1, 2, 1):
        graphed_terms.append(gs.step(cams[k], gts[k], gtds[k]).clone())
        eager_terms.append(trainer.training_step_fused(b, cams[k], gts[k], bg, gt_depth=gtds[k], lambda_depth=LAMBDA_D)[0].clone())
    assert gs.check() == 0
    for x, y in zip(graphed_terms, eager_terms):
        assert x.numel() == 3 and torch.equal(x, y)
    assert_same_state(model_state(a), model_state(b))


@pytest.mark.parametrize("use_graph", [False, True])
def test_graphed_depth_step_repeats_overflowed_steps_with_their_own_targets(use_graph):
    from gaussian_lic_amd import rasterizer as rz
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import gt_image
    dev = gpu()
    P, W, H = 40000, 320, 240
    raw, sc, camd, cam0 = make_scene("random", P, W, H, 3, 8)
    cams = [synthetic_camera(W, H, k).to_device(dev) for k in range(8)]
    gts = [gt_image(H, W, seed=10 + k).to(dev) for k in range(8)]
    gtds = [_lidar_target(raw, c) for c in cams]
    bg = torch.zeros(3, device=dev)
    probe, e, Rs = training_model(raw), torch.empty(0, device=dev), []
    with torch.no_grad():
        for c in cams:
            Rs.append(rz.rasterize_gaussians(bg, probe.xyz.detach(), e, probe.opacity.detach(), probe.scaling.detach(), probe.rotation.detach(), 1.0, e,
                                             c.d_world_view_transform, c.d_full_proj_transform, float(c.tanfovx), float(c.tanfovy), H, W,
                                             float(c.limx_neg), float(c.limx_pos), float(c.limy_neg), float(c.limy_pos), probe.features_dc.detach(),
                                             probe.features_rest.detach(), 3, c.d_camera_center, False, False, False, raw_params=True)[0])
    cap_R = (max(Rs) + sorted(Rs)[len(Rs) // 2]) // 2      # the larger views do not fit
    fits = [r <= cap_R - 64 for r in Rs]
    assert any(fits) and not all(fits)
    model = training_model(raw)
    first = fits.index(True)
    gs = trainer.GraphedStep(model, cams[first], gts[first], bg, check_every=0, cap_R=cap_R, use_graph=use_graph, gt_depth=gtds[first],
                             lambda_depth=LAMBDA_D)
    for k in range(8):
        gs.step(cams[k], gts[k], gtds[k])
    issued, mask, _max_R, _max_B = gs.bufs.read_window()
    failed = [k for k in range(8) if (mask >> k) & 1]
    assert issued == 8 and failed
    assert gs.check() == len(failed) and gs.recaptures >= 1
    eager = training_model(raw)
    for k in [k for k in range(8) if k not in failed] + failed:
        trainer.training_step_fused(eager, cams[k], gts[k], bg, gt_depth=gtds[k], lambda_depth=LAMBDA_D)
    assert_same_state(model_state(model), model_state(eager))

    # a depth target modified in place after its (overflowed) step was issued: the repeat refuses
    model2 = training_model(raw)
    gs2 = trainer.GraphedStep(model2, cams[first], gts[first], bg, check_every=0, cap_R=cap_R, use_graph=use_graph, gt_depth=gtds[first],
                              lambda_depth=LAMBDA_D)
    k_bad = int(np.argmax(Rs))
    tgt = gtds[k_bad].clone()
    gs2.step(cams[k_bad], gts[k_bad], tgt)
    tgt.mul_(2.0)
    with pytest.raises(RuntimeError, match="depth target .* modified in place"):
        gs2.check()


# ---------------------------------------------------------------------------------------------------- 7. the C++ host
@pytest.mark.parametrize("deg", [3, 0])
def test_fused_depth_cpp_host(tmp_path, deg):
    """gslic::FusedStep::step(cam, gt, gt_depth, lambda_depth) issues the C-ABI calls of training_step_fused(gt_depth=, lambda_depth=): image, depth,
    terms and parameters after four steps are bit-identical to the Python host's.  The driver is built when missing (a build failure fails)."""
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    exe = fio.build("fused_depth")
    P, W, H, iters = 30000, 320, 240, 4
    raw, cam, gt, gtd, bg = _setup("random", P, W, H, deg, 44)
    d = str(tmp_path)
    fio.write_inputs(d, raw, cam, gt=gt, gt_depth=gtd)
    r = fio.run(exe, d, str(P), str(W), str(H), str(deg), str(iters), repr(LAMBDA_D))
    model = training_model(raw)
    fl = trainer._default_fused_loss()
    losses = []
    for _ in range(iters):
        terms, _vis = trainer.training_step_fused(model, cam, gt, bg, gt_depth=gtd, lambda_depth=LAMBDA_D)
        losses.append(float(fl.value(terms, LAMBDA_D)))
    rd = lambda name, shape: fio.read(d, name + ".f32", np.float32).numpy().reshape(shape)
    np.testing.assert_array_equal(rd("terms", (3,)), terms.cpu().numpy())
    names = [("xyz", model.xyz), ("scaling", model.scaling), ("rotation", model.rotation), ("opacity", model.opacity), ("dc", model.features_dc)]
    if deg > 0:
        names.append(("rest", model.features_rest))
    for name, t in names:
        np.testing.assert_array_equal(rd(name, tuple(t.shape)), t.detach().cpu().numpy(), err_msg=name)
    printed = [float(l.split()[3]) for l in r.stdout.splitlines() if l.startswith("iter ")]
    assert len(printed) == iters and np.allclose(printed, losses, rtol=1e-5)


# ---------------------------------------------------------------------------------------------------- 8. supervision works on the fused path
def test_fused_depth_supervision_pulls_the_map_toward_the_target_depth():
    import math
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.loss import depth_l1
    from gaussian_lic_amd.rasterizer import render
    dev = gpu()
    W, H = 160, 120
    raw, sc, camd, cam = make_scene("random", 3000, W, H, 3, 10)
    cam.to_device(dev)
    bg = torch.zeros(3, device=dev)
    tgt = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in raw.items()}
    tgt["xyz"] = (raw["xyz"] * 1.2).contiguous()
    tgt["scaling"] = (raw["scaling"] + math.log(1.2)).contiguous()
    with torch.no_grad():
        gt, _, _, _, _, gtd = render(cam, trainer.GaussianModel(tgt, dev), bg, return_depth=True)

    def run(lam):
        m = training_model(raw)
        with torch.no_grad():
            d0 = float(depth_l1(render(cam, m, bg, return_depth=True)[5], gtd))
        for _ in range(50):
            trainer.training_step_fused(m, cam, gt, bg, gt_depth=gtd, lambda_depth=lam)
        with torch.no_grad():
            d1 = float(depth_l1(render(cam, m, bg, return_depth=True)[5], gtd))
        return d0, d1

    s_on, e_on = run(1.0)
    s_off, e_off = run(0.0)
    assert s_on == s_off and s_on > 0
    assert e_on < s_on and e_on < e_off, (s_on, e_on, e_off)


# ---------------------------------------------------------------------------------------------------- 9. N > 1 refuses
def test_fused_depth_step_refuses_multi_gpu(monkeypatch):
    from gaussian_lic_amd import trainer
    raw, cam, gt, gtd, bg = _setup("random", 5000, 160, 120, 3, 5)
    m = training_model(raw)
    before = model_state(m)
    monkeypatch.setattr(trainer, "_dist_on", lambda: True)
    with pytest.raises(NotImplementedError, match="N > 1"):
        trainer.training_step_fused(m, cam, gt, bg, gt_depth=gtd, lambda_depth=LAMBDA_D)
    assert_same_state(before, model_state(m))
