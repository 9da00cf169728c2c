"""-m gpu: the trainable per-view exposure — the two kernels (gslic_exposure_apply / gslic_exposure_backward) against the numpy restatement of
their rule (tests/exposure_ref.py: apply and dL_dimage on bits, dL_dE inside the worst-case bound of any summation order, the Adam update against
the float64 rule), loss.apply_exposure, and the exposure through every step path: training_step_fused, GraphedStep eager and captured, the C++
host, and a run that has to learn a known exposure."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import exposure_ref as ref
import fused_check_io as fio
from conftest import make_scene
from gpu_helpers import assert_same_state, bits, gpu, model_state, training_model

pytestmark = pytest.mark.gpu

LAM = 0.2
LAMBDA_D = 0.5
FINAL_THREADS = 256   # EX_THREADS of csrc/exposure.hip: the workgroup that adds the partial rows
# the smallest shapes that can break the vector path, the tail and the two-level reduction; the last one has more partial rows than the finalising
# workgroup has threads, and not a power of two of them (test_shapes_cover_the_kernels_constants reads that off the library)
SHAPES = [(1, 1), (1, 63), (33, 17), (70, 50), (160, 120), (523, 1031)]


def _L():
    from gaussian_lic_amd import _lib
    return _lib


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu())


@functools.lru_cache(maxsize=None)
def _case(H, W):
    """The inputs of a shape and their float64 reference, computed once and left unchanged."""
    E, x, g = ref.case(H, W, 1000 * H + W)
    dimg64, dE64, mag = ref.backward64(E, x, g)
    return dict(E=E, x=x, g=g, dE64=dE64, mag=mag)


def _apply(E, x):
    from gaussian_lic_amd import loss
    return loss.exposure_apply(x, E, torch.empty_like(x))


def _backward(E, x, g, adam=None, partials=None):
    """The export by hand: (dL_dimage, dL_dE [12], partials)."""
    from gaussian_lic_amd import loss
    H, W = x.shape[1:]
    if partials is None:
        partials = torch.empty(int(_L().lib().gslic_exposure_partials_count(H, W)), device=gpu())
    dimg, dE = torch.empty_like(x), torch.empty(12, device=gpu())
    loss.exposure_backward(x, E, g, dimg, partials, dE, adam)
    return dimg, dE, partials


def test_shapes_cover_the_kernels_constants():
    count = _L().lib().gslic_exposure_partials_count
    pix = next(n for n in range(1, 1 << 16) if count(1, n + 1) > 12)      # pixels per workgroup, read off the library
    assert pix % 4 == 0 and count(1, pix) == 12
    H, W = SHAPES[-1]
    rows = count(H, W) // 12
    assert rows == -(-H * W // pix) and rows > FINAL_THREADS and rows & (rows - 1) and H <= 1080 and W <= 1920
    assert (H * W) % 4 != 0 and (H * W) % pix != 0                        # a group of four that crosses the end, in a partly filled workgroup
    assert any(h * w > pix and (h * w) % 4 == 0 for h, w in SHAPES)      # the 16-byte path over more than one workgroup


# ---------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("H,W", SHAPES)
def test_apply_and_dimage_are_the_float32_rule_bit_for_bit(H, W):
    c = _case(H, W)
    E, x, g = _dev(c["E"]), _dev(c["x"]), _dev(c["g"])
    out = _apply(E, x)
    dimg, _dE, _p = _backward(E, x, g)
    assert np.array_equal(out.cpu().numpy().view(np.int32), ref.apply32(c["E"], c["x"]).view(np.int32))
    assert np.array_equal(dimg.cpu().numpy().view(np.int32), ref.dimage32(c["E"], c["g"]).view(np.int32))
    assert torch.equal(bits(_apply(_dev(ref.IDENTITY), x)), bits(x))      # [I | 0] returns the image's own bits
    # images that are only dword-aligned take the other access path: the same bits, dL_dE included (the pixels are cut by H * W alone)
    pad = lambda t: torch.cat([torch.zeros(1, device=gpu()), t.reshape(-1)])[1:].view(t.shape)
    xo, go = pad(x), pad(g)
    assert xo.data_ptr() % 16 == 4
    assert torch.equal(bits(_apply(E, xo)), bits(out))
    dimg_o, dE_o, _p = _backward(E, xo, go)
    assert torch.equal(bits(dimg_o), bits(dimg)) and torch.equal(bits(dE_o), bits(_dE))


@pytest.mark.parametrize("H,W", SHAPES)
def test_dE_is_inside_the_worst_case_bound_and_reproducible(H, W):
    c = _case(H, W)
    E, x, g = _dev(c["E"]), _dev(c["x"]), _dev(c["g"])
    _dimg, dE, partials = _backward(E, x, g)
    got = dE.cpu().numpy().astype(np.float64).reshape(3, 4)
    # |err| <= n 2^-24 sum_p |g x|: the worst case of any order of n float32 additions of rounded products; derived, not measured
    bound = H * W * 2.0 ** -24 * c["mag"]
    err = np.abs(got - c["dE64"])
    print("dL_dE error / bound per entry:", (err / np.maximum(bound, 1e-300)).round(4).tolist())
    assert (err <= bound).all(), (err, bound)
    # the same bits again, on the same scratch and on a freshly allocated one that holds something else
    _d2, dE2, _p2 = _backward(E, x, g, partials=partials)
    _d3, dE3, _p3 = _backward(E, x, g, partials=torch.full_like(partials, float("nan")))
    assert torch.equal(bits(dE2), bits(dE)) and torch.equal(bits(dE3), bits(dE))


def test_adam_update_against_the_float64_rule_on_two_alternating_views():
    """Five steps, views 1, 0, 1, 0, 1 of three rows.  The float64 trajectory runs free from the same start on the gradients the kernel reports
    (float32 values), with the scalars the float32 values the descriptor holds; per element and step
    |dp - dp_ref| <= 16 2^-24 |dp_ref| + 2^-24 |p|: the handful of float32 operations of the rule, and the rounding of the final subtraction."""
    from gaussian_lic_amd import trainer
    H, W = 70, 50
    rng = np.random.default_rng(11)
    ex = trainer.Exposure(3, gpu(), lr=0.01)
    start = rng.uniform(-1.5, 1.5, (3, 3, 4)).astype(np.float32)
    ex.params.copy_(_dev(start))
    lr, b1, b2, eps = (float(np.float32(a)) for a in (ex.lr, ex.betas[0], ex.betas[1], ex.eps))
    p64, m64, v64, t64 = start.astype(np.float64).reshape(3, 12), np.zeros((3, 12)), np.zeros((3, 12)), [0, 0, 0]
    for step in range(5):
        view = (step + 1) % 2
        _E, x, g = ref.case(H, W, 50 + step)
        x, g = _dev(x), _dev(g * (10.0 ** (step - 2)))                     # gradients over several orders of magnitude
        before = ex.params.clone()
        before_state = (ex.m.clone(), ex.v.clone(), ex.steps.clone())
        _dimg, dE, _p = _backward(ex.params[view], x, g, adam=ex._descriptor(ex._views[view:view + 1]))
        gk = dE.cpu().numpy().astype(np.float64)
        was = p64[view].copy()
        p64[view], m64[view], v64[view], t64[view] = ref.adam64(p64[view], m64[view], v64[view], t64[view], gk, lr, b1, b2, eps)
        dp = ex.params[view].reshape(12).cpu().numpy().astype(np.float64) - before[view].reshape(12).cpu().numpy().astype(np.float64)
        dp_ref = p64[view] - was
        tol = 16 * 2.0 ** -24 * np.abs(dp_ref) + 2.0 ** -24 * np.abs(before[view].reshape(12).cpu().numpy().astype(np.float64))
        print("step", step, "max |dp - dp_ref| / tol:", float((np.abs(dp - dp_ref) / tol).max()))
        assert (np.abs(dp - dp_ref) <= tol).all(), step
        assert np.abs(dp).min() > 0                                          # every entry moved
        for other in set(range(3)) - {view}:                                 # the other rows: not a bit touched
            assert torch.equal(bits(ex.params[other]), bits(before[other]))
            assert torch.equal(bits(ex.m[other]), bits(before_state[0][other])) and torch.equal(bits(ex.v[other]), bits(before_state[1][other]))
            assert int(ex.steps[other]) == int(before_state[2][other])
    assert ex.steps.tolist() == [2, 3, 0] == t64
    # a set skip word turns the update off and still writes dL_dE
    frozen = ex.clone()
    skip = torch.tensor([2], dtype=torch.int32, device=gpu())
    _dimg, dE, _p = _backward(ex.params[0], x, g, adam=ex._descriptor(ex._views[0:1], skip))
    assert torch.equal(bits(ex.params), bits(frozen.params)) and ex.steps.tolist() == [2, 3, 0] and bool(dE.abs().sum() > 0)


def test_apply_exposure_autograd_is_the_two_exports_bit_for_bit():
    from gaussian_lic_amd import loss
    c = _case(33, 17)
    E, x, g = _dev(c["E"]), _dev(c["x"]), _dev(c["g"])
    Et, xt = E.clone().requires_grad_(True), x.clone().requires_grad_(True)
    out = loss.apply_exposure(xt, Et)
    assert torch.equal(bits(out.detach()), bits(_apply(E, x)))
    out.backward(g)
    dimg, dE, _p = _backward(E, x, g)
    assert torch.equal(bits(xt.grad), bits(dimg)) and torch.equal(bits(Et.grad.reshape(12)), bits(dE))
    # a batched image keeps its shape
    out4 = loss.apply_exposure(x[None], E)
    assert tuple(out4.shape) == (1,) + tuple(x.shape) and torch.equal(bits(out4[0]), bits(out.detach()))


# ---------------------------------------------------------------------------------------------------- the steps
P_, W_, H_, DEG = 1536, 160, 120, 3


@functools.lru_cache(maxsize=None)
def _setup(seed=5):
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import gt_image
    raw, sc, camd, cam = make_scene("random", P_, W_, H_, DEG, seed)
    cam.to_device(gpu())
    cams = [cam, synthetic_camera(W_, H_, 1).to_device(gpu())]
    gts = [gt_image(H_, W_, seed=seed + k).to(gpu()) for k in range(2)]
    gtd = cam.project_depth(raw["xyz"][::5].float() * 1.1).to(gpu())
    return raw, cams, gts, gtd, torch.zeros(3, device=gpu())


def _exposure(lr=0.01, seed=3):
    """Two rows near the identity (a brighter and a darker view), so that the compensated image stays an image."""
    from gaussian_lic_amd import trainer
    ex = trainer.Exposure(2, gpu(), lr=lr)
    rng = np.random.default_rng(seed)
    ex.params.add_(_dev(rng.uniform(-0.1, 0.1, (2, 3, 4)).astype(np.float32)))
    return ex


def _exposure_state(ex):
    return dict(params=ex.params.cpu().clone(), m=ex.m.cpu().clone(), v=ex.v.cpu().clone(), steps=ex.steps.cpu().clone(), grad=ex.grad.cpu().clone())


def _same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), k


def test_fused_step_without_update_leaves_the_gradient_of_the_exports_called_by_hand():
    from gaussian_lic_amd import loss, trainer
    raw, cams, gts, gtd, bg = _setup()
    model, ex = training_model(raw), _exposure()
    before, ex_before = model_state(model), _exposure_state(ex)
    terms, vis = trainer.training_step_fused(model, cams[0], gts[0], bg, fused_loss=loss.FusedLoss(LAM), exposure=ex, view=1, do_step=False)
    with torch.no_grad():
        rr = trainer._RawRaster(model, cams[0], bg, False)
        image, _depth, _radii = rr.forward()
        out = _apply(ex.params[1], image)
        dL_dout, terms_hand = loss.FusedLoss(LAM).forward_backward(out, gts[0])
        _dimg, dE, _p = _backward(ex.params[1], image, dL_dout)
    assert torch.equal(bits(ex.grad.reshape(12)), bits(dE)) and bool(dE.abs().min() > 0)
    assert torch.equal(bits(terms), bits(terms_hand)) and bool(vis.any())
    assert_same_state(before, model_state(model))
    after = _exposure_state(ex)
    after.pop("grad"); ex_before.pop("grad")
    _same_bits(after, ex_before)                                             # do_step=False updates nothing


def test_identity_exposure_with_zero_rate_is_the_step_without_it():
    from gaussian_lic_amd import trainer
    raw, cams, gts, gtd, bg = _setup()
    a, b = training_model(raw), training_model(raw)
    ex = trainer.Exposure(2, gpu(), lr=0.0)
    for k in (0, 1):
        ta, va = trainer.training_step_fused(a, cams[k], gts[k], bg, exposure=ex, view=k)
        tb, vb = trainer.training_step_fused(b, cams[k], gts[k], bg)
        assert torch.equal(ta, tb) and torch.equal(va, vb)
    assert_same_state(model_state(a), model_state(b))                        # `==` on the floats: a zero's sign may differ through 0 * g
    assert torch.equal(ex.params, torch.eye(3, 4, device=gpu()).expand(2, 3, 4)) and ex.steps.tolist() == [1, 1]
    assert bool(ex.grad.abs().sum() > 0)


@pytest.mark.parametrize("combo", ["weight", "depth", "grad_stats"])
def test_fused_step_combinations_equal_the_call_made_by_hand_in_pieces(combo):
    from gaussian_lic_amd import loss, trainer
    raw, cams, gts, gtd, bg = _setup()
    cam, gt = cams[0], gts[0]
    a, b = training_model(raw), training_model(raw)
    ex_a, ex_b = _exposure(), _exposure()
    w = (torch.rand(H_, W_, generator=torch.Generator().manual_seed(1)) * 1.2).to(gpu()) if combo == "weight" else None
    dw = (torch.rand(H_, W_, generator=torch.Generator().manual_seed(2)) * 3.0).to(gpu()) if combo == "depth" else None
    depth = combo == "depth"
    gs_a = trainer.GradientStats(a) if combo == "grad_stats" else None
    gs_b = trainer.GradientStats(b) if combo == "grad_stats" else None
    kw = dict(weight=w)
    if depth:
        kw.update(gt_depth=gtd, lambda_depth=LAMBDA_D, depth_weight=dw)
    fl_a, fl_b = loss.FusedLoss(LAM), loss.FusedLoss(LAM)
    for _ in range(2):
        terms_a, vis_a = trainer.training_step_fused(a, cam, gt, bg, fused_loss=fl_a, exposure=ex_a, view=1, grad_stats=gs_a, **kw)
        with torch.no_grad():
            rr = trainer._RawRaster(b, cam, bg, depth)
            image, zimg, _radii = rr.forward()
            out = _apply(ex_b.params[1], image)
            dL_dout, _t = fl_b.forward_backward(out, gt, w)
            dLd = fl_b.depth_forward_backward(zimg, gtd, LAMBDA_D, dw)[0] if depth else None
            dimg, dE, _p = _backward(ex_b.params[1], image, dL_dout, adam=ex_b._descriptor(ex_b._views[1:2]))
            ex_b.grad.copy_(dE.view(3, 4))
            xg = torch.empty(b.P, 3, device=gpu()) if depth else None
            vis_b = torch.empty(b.P, dtype=torch.uint8, device=gpu())
            extra = dict(grad_stats=gs_b._descriptor()) if gs_b is not None else {}
            rr.backward(dimg, dLd, adam=b.optimizer.fused_descriptor(visible_out=vis_b), xyz_grad=xg, **extra)
            b.optimizer.count_step()
            terms_b = fl_b.terms3 if depth else fl_b.terms3[:2]
        assert torch.equal(bits(terms_a), bits(terms_b)) and torch.equal(vis_a, vis_b.view(torch.bool))
    assert_same_state(model_state(a), model_state(b))
    _same_bits(_exposure_state(ex_a), _exposure_state(ex_b))
    assert ex_a.steps.tolist() == [0, 2]
    if gs_a is not None:
        for (x, _w1), (y, _w2) in zip(gs_a._arrays(), gs_b._arrays()):
            assert torch.equal(x, y) and bool(x.any())


@pytest.mark.parametrize("use_graph", [False, True])
def test_graphed_step_with_an_exposure_equals_the_fused_steps(use_graph):
    from gaussian_lic_amd import trainer
    raw, cams, gts, gtd, bg = _setup()
    a, b = training_model(raw), training_model(raw)
    ex_a = _exposure()
    ex_b = ex_a.clone()
    gs = trainer.GraphedStep(a, cams[0], gts[0], bg, use_graph=use_graph, exposure=ex_a, view=0)
    _same_bits(_exposure_state(ex_a), _exposure_state(ex_b))                 # building the step (warm-up, capture) left the exposure as it was
    for k in (0, 1, 0, 1):
        tg = gs.step(cams[k], gts[k], view=k).clone()
        te = trainer.training_step_fused(b, cams[k], gts[k], bg, exposure=ex_b, view=k)[0]
        assert torch.equal(bits(tg), bits(te))
    assert gs.check() == 0
    assert_same_state(model_state(a), model_state(b))
    _same_bits(_exposure_state(ex_a), _exposure_state(ex_b))
    assert ex_a.steps.tolist() == [2, 2]
    plain = trainer.GraphedStep(b, cams[0], gts[0], bg)
    with pytest.raises(ValueError, match="built without"):
        plain.step(cams[0], gts[0], view=1)


def test_fused_exposure_cpp_host(tmp_path):
    """gslic::Exposure and FusedStep::set_exposure issue the C-ABI calls of training_step_fused(exposure=, view=): parameters, moments, E and its
    state, the step counts and every step's terms are bit-identical to the Python host's over four steps on two views."""
    from gaussian_lic_amd import loss, trainer
    exe = fio.build("fused_exposure")
    iters = 4
    raw, cams, gts, gtd, bg = _setup()
    ex = _exposure(lr=0.02)
    d = str(tmp_path)
    fio.write_inputs(d, raw, cams, gt=gts[0], gt2=gts[1], E=ex.params)
    r = fio.run(exe, d, str(P_), str(W_), str(H_), str(DEG), str(iters), repr(0.02))
    model, fl = training_model(raw), loss.FusedLoss(LAM)
    g, _t = trainer.pose_gradient(model, cams[0], gts[0], bg, fused_loss=fl, exposure=ex, view=0)
    terms = []
    for it in range(iters):
        terms.append(trainer.training_step_fused(model, cams[it % 2], gts[it % 2], bg, fused_loss=fl, exposure=ex, view=it % 2)[0].clone())
    rows = fio.read_rows(d, 15)
    for name, t in [("xyz", model.xyz), ("scaling", model.scaling), ("rotation", model.rotation), ("opacity", model.opacity), ("dc", model.features_dc),
                    ("rest", model.features_rest)]:
        assert torch.equal(rows[name], bits(t.detach().cpu()).reshape(-1)), name
        full = "features_" + name if name in ("dc", "rest") else name
        assert torch.equal(rows["m_" + name], bits(model._m[full][:model.P].cpu()).reshape(-1)), "m_" + name
        assert torch.equal(rows["v_" + name], bits(model._v[full][:model.P].cpu()).reshape(-1)), "v_" + name
    rd = lambda name, dt=np.int32: fio.read(d, name, dt)
    assert torch.equal(rd("E.f32"), bits(ex.params.cpu()).reshape(-1))
    assert torch.equal(rd("E_m.f32"), bits(ex.m.cpu()).reshape(-1)) and torch.equal(rd("E_v.f32"), bits(ex.v.cpu()).reshape(-1))
    assert rd("E_steps.i32").tolist() == ex.steps.tolist() == [2, 2]
    assert torch.equal(rd("E_grad.f32"), bits(ex.grad.cpu()).reshape(-1))
    assert torch.equal(rd("terms.f32"), bits(torch.stack(terms).cpu()).reshape(-1))
    pose = [l for l in r.stdout.splitlines() if l.startswith("pose ")]
    assert len(pose) == 1
    # (the se(3) chain runs on the host in both: the bar of tests/test_shim_gpu.py::test_fused_cpp_host_pose_gradient, 1e-5 of max-abs)
    got, want = np.array([float(x) for x in pose[0].split()[1:]]), np.asarray(g, np.float64)
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()


def test_exposure_learns_a_known_transform():
    """The target is the map's own render under a fixed non-identity [A | b], the map's learning rates are 0: after 30 steps the mean-L1 term is
    below the first step's and E is closer to [A | b] than the identity it started from.  Conditions, not tolerances."""
    from gaussian_lic_amd import trainer
    raw, cams, gts, gtd, bg = _setup()
    model = trainer.GaussianModel({k: (v.clone() if torch.is_tensor(v) else v) for k, v in raw.items()}, gpu())
    model.training_setup({k: 0.0 for k in trainer.DEFAULT_LRS})
    Ab = torch.tensor([[0.8, 0.05, 0.0, 0.06], [0.0, 0.75, 0.05, 0.04], [0.05, 0.0, 0.7, 0.02]], device=gpu())
    with torch.no_grad():
        gt0 = trainer._RawRaster(model, cams[0], bg, False).forward()[0].clone()
    gt = torch.clamp(torch.einsum("ck,khw->chw", Ab[:, :3], gt0) + Ab[:, 3][:, None, None], 0.0, 1.0).contiguous()
    ex = trainer.Exposure(1, gpu(), lr=0.01)
    dist0 = float((ex.matrix(0) - Ab).norm())
    l1 = [float(trainer.training_step_fused(model, cams[0], gt, bg, exposure=ex, view=0)[0][0]) for _ in range(30)]
    print("mean L1 first / last:", l1[0], l1[-1], " |E - [A|b]| first / last:", dist0, float((ex.matrix(0) - Ab).norm()))
    assert l1[-1] < l1[0]
    assert float((ex.matrix(0) - Ab).norm()) < dist0
    assert int(ex.steps[0]) == 30


_DIST_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import torch
torch.distributed.init_process_group("gloo", rank=0, world_size=1)
import gaussian_lic_amd  # noqa: F401
from gaussian_lic_amd import trainer
ex = trainer.Exposure(1, "cpu")
for fn in (trainer.training_step_fused, trainer.training_step, trainer.pose_gradient, trainer.training_step_with_pose):
    try:
        fn(None, None, None, None, exposure=ex, view=0)     # nothing but the refusal can come out of these arguments
    except NotImplementedError as e:
        assert "exposure" in str(e), e
    else:
        raise SystemExit("no NotImplementedError from " + fn.__name__)
torch.distributed.destroy_process_group()
print("REFUSED")
"""


def test_exposure_under_the_gradient_exchange_is_refused_before_any_launch():
    """A process group needs a process of its own: one rank, GSLIC_FORCE_DIST=1 (the exchange path of N > 1)."""
    env = dict(os.environ)
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", GSLIC_FORCE_DIST="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _DIST_CHILD, root], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "REFUSED" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
