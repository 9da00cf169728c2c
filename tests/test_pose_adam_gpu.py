"""-m gpu: the fused-Adam backwards with the camera gradient (gslic_rasterize_backward_camera_adam / _depth_camera_adam) and the two keywords on
top of them — training_step_with_pose(adam_in_backward=True) and GraphedStep(train_pose=True) — against the two-call route they replace.

Every comparison is on bits: the new route runs the same arithmetic in the same order as the old one (same chain, same adam_scalar, same partial
rows and reduction order), so no tolerance appears anywhere.  The scene is that of tests/test_pose_set_gpu.py: 400 rows are six full 64-row
blocks and a partial one of 16 on the M == 15 path (deg 3), one full 256-row block and a partial one of 144 on the generic path (deg 1)."""
import functools

import numpy as np
import pytest
import torch

import fused_check_io as fio
from conftest import make_scene
from gpu_helpers import assert_same_state, bits, gpu, guarded, guards_intact, model_state, training_model
from test_pose_adam_cpu import run_refusal_cases

pytestmark = pytest.mark.gpu

P_, W_, H_ = 400, 64, 48
LAMBDA_D = 0.5
POSE_KEYS = ("view", "proj", "campos", "m", "v", "steps", "grad")


@functools.lru_cache(maxsize=None)
def _setup(deg, seed=5):
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import gt_image
    raw, sc, camd, cam = make_scene("random", P_, W_, H_, deg, seed)
    cam.to_device(gpu())
    cams = [cam, synthetic_camera(W_, H_, 4).to_device(gpu())]
    gts = [gt_image(H_, W_, seed=seed + k).to(gpu()) for k in range(2)]
    gtd = cam.project_depth(raw["xyz"][::5].float() * 1.1).to(gpu())
    return raw, cams, gts, gtd, torch.zeros(3, device=gpu())


def _pose_set(cams, **kw):
    from gaussian_lic_amd import trainer
    ps = trainer.PoseSet(2, cams[0], gpu(), **kw)
    ps.load(1, cams[1])
    return ps


def _pose_state(ps):
    return {k: getattr(ps, k).cpu().clone() for k in POSE_KEYS}


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), k


def _forward_and_loss(model, cam, gt, gtd, depth):
    """(_RawRaster after its forward, radii, dL/dimage, dL/ddepth or None) — each call on a FusedLoss of its own (the gradients live in its scratch)."""
    from gaussian_lic_amd import loss, trainer
    rr = trainer._RawRaster(model, cam, torch.zeros(3, device=gpu()), depth)
    image, d, radii = rr.forward()
    dL_dimage, dL_ddepth, _terms = trainer._fused_losses(loss.FusedLoss(0.2), image, gt, d, gtd if depth else None, LAMBDA_D if depth else 0.0)
    return rr, radii, dL_dimage, dL_ddepth


# ------------------------------------------------------------------------------------------------ 1, 2: the entry points
@pytest.mark.parametrize("deg", [1, 3])
@pytest.mark.parametrize("depth", [False, True])
def test_entry_points_against_the_two_call_route(depth, deg):
    from gaussian_lic_amd import trainer
    raw, cams, gts, gtd, bg = _setup(deg)
    a, b, c = training_model(raw), training_model(raw), training_model(raw)
    before = model_state(b)
    with torch.no_grad():
        # copy A: the camera backward into the slab, then the masked Adam
        rr, radii, dL, dLd = _forward_and_loss(a, cams[1], gts[1], gtd, depth)
        slab = trainer._grad_slab(a)
        out = rr.backward(dL, dLd, out=slab.views, camera_grads=True)
        visible = radii > 0
        a.optimizer.set_visibility_and_N(visible, a.P)
        a.optimizer.step(slab.grads(a))
        # copy B: the new call, its 35 outputs between guard words
        rr, radii_b, dL, dLd = _forward_and_loss(b, cams[1], gts[1], gtd, depth)
        vis = torch.full((P_,), 7, dtype=torch.uint8, device=gpu())
        buf, words = guarded(35, dtype=torch.float32, fill=-7.0)
        cam = rr.backward(dL, dLd, adam=b.optimizer.fused_descriptor(visible_out=vis), xyz_grad=torch.empty(P_, 3, device=gpu()) if depth else None,
                          camera_grads=True, cam_out=words)
        b.optimizer.count_step()
        # copy C, untouched: the camera backward alone (the sums of the parameters as they were)
        rr, _r, dL, dLd = _forward_and_loss(c, cams[1], gts[1], gtd, depth)
        alone = rr.backward(dL, dLd, camera_grads=True)[9:12]
    torch.cuda.synchronize()
    assert torch.equal(radii, radii_b)
    n_vis = int(visible.sum())
    print(f"camera + Adam depth={depth} deg={deg}: {n_vis} of {P_} rows visible")
    assert 0 < n_vis < P_                                                             # both kinds of row are in the test
    assert_same_state(model_state(a), model_state(b))                                 # parameters and both moments
    assert torch.equal(vis.cpu(), visible.to(torch.uint8).cpu())
    for k, n in enumerate((16, 16, 3)):
        assert cam[k].numel() == n
        assert torch.equal(bits(cam[k]), bits(out[9 + k])), k
        assert torch.equal(bits(cam[k]), bits(alone[k])), k
    assert cam[0].data_ptr() == words.data_ptr() and guards_intact(buf, 35)
    assert bool(cam[0].abs().max() > 0) and bool(cam[1].abs().max() > 0) and bool(cam[2].abs().max() > 0)
    if depth:                                                                         # the direct terms are there: view row 2, column 3 = sum of dL/dz
        assert float(cam[0][14]) != 0.0
    after, inv = model_state(b), (~visible).cpu()
    for k in before:                                                                  # rows with radii <= 0: not a bit moved
        assert torch.equal(bits(after[k][inv]), bits(before[k][inv])), k
    assert any(not torch.equal(after[k], before[k]) for k in before)


# ------------------------------------------------------------------------------------------------ 3: training_step_with_pose
STEP_CASES = {
    "row+weight": dict(deg=3, row=True, weight=True),
    "host+exposure": dict(deg=3, row=False, exposure=True),
    "row+depth_weight_huber": dict(deg=1, row=True, depth=True),
    "host+depth+weight": dict(deg=3, row=False, depth=True, weight=True),
    "row+exposure+grad_stats": dict(deg=3, row=True, exposure=True, stats=True),
    "host+depth+grad_stats": dict(deg=1, row=False, depth=True, stats=True),
}


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_training_step_with_pose_adam_in_backward_against_the_default(case):
    from gaussian_lic_amd import loss, trainer
    from gaussian_lic_amd.camera import synthetic_camera
    cfg = STEP_CASES[case]
    raw, cams, gts, gtd, bg = _setup(cfg["deg"])
    rng = torch.Generator().manual_seed(3)
    weight = torch.rand(H_, W_, generator=rng).to(gpu()) if cfg.get("weight") else None
    kw = dict(weight=weight)
    if cfg.get("depth"):
        kw.update(gt_depth=gtd, lambda_depth=LAMBDA_D, depth_weight=(torch.rand(H_, W_, generator=rng) * 2).to(gpu()), depth_huber=0.05)
    results = []
    for fused in (False, True):
        model = training_model(raw)
        ex = trainer.Exposure(2, gpu(), lr=0.01) if cfg.get("exposure") else None
        stats = trainer.GradientStats(model) if cfg.get("stats") else None
        ps = _pose_set(cams, lr_trans=2e-3, lr_rot=1e-3) if cfg["row"] else None
        host = None if cfg["row"] else synthetic_camera(W_, H_, 4).to_device(gpu())
        for it in range(2):                                                           # two steps: the second starts from moved moments and pose
            if cfg["row"]:
                terms, visible, g = trainer.training_step_with_pose(model, cams[0], gts[1], bg, fused_loss=loss.FusedLoss(0.2), poses=ps, view=1,
                                                                    exposure=ex, grad_stats=stats, adam_in_backward=fused, **kw)
                assert g is ps.grad
            else:
                terms, visible, g = trainer.training_step_with_pose(model, host, gts[1], bg, pose_lr=1e-3, fused_loss=loss.FusedLoss(0.2), view=1,
                                                                    exposure=ex, grad_stats=stats, adam_in_backward=fused, **kw)
        torch.cuda.synchronize()
        results.append(dict(
            model=model_state(model), terms=terms.cpu().clone(), visible=visible.cpu().clone(),
            g=g.cpu().clone() if torch.is_tensor(g) else torch.from_numpy(np.asarray(g, np.float64)),
            pose=_pose_state(ps) if ps is not None else dict(view=torch.from_numpy(host.world_view_transform.copy()),
                                                            proj=torch.from_numpy(host.full_proj_transform.copy()),
                                                            campos=torch.from_numpy(host.camera_center.copy())),
            ex={} if ex is None else {k: getattr(ex, k).cpu().clone() for k in ("params", "m", "v", "steps", "grad")},
            stats={} if stats is None else dict(grad_sum=stats.grad_sum().cpu().clone(), n_seen=stats.n_seen().cpu().clone(),
                                                max_radius=stats.max_radius().cpu().clone())))
    old, new = results
    assert_same_state(old["model"], new["model"])
    assert torch.equal(bits(old["terms"]), bits(new["terms"])) and torch.equal(old["visible"], new["visible"]) and new["visible"].dtype == torch.bool
    assert torch.equal(old["g"], new["g"]) and bool(new["g"].abs().max() > 0)
    _same(old["pose"], new["pose"])
    _same(old["ex"], new["ex"])
    _same(old["stats"], new["stats"])
    if cfg["row"]:
        assert new["pose"]["steps"].tolist() == [0, 2]
    if cfg.get("stats"):
        assert int(new["stats"]["n_seen"].max()) == 2 and float(new["stats"]["grad_sum"].max()) > 0
    if cfg.get("exposure"):
        assert new["ex"]["steps"].tolist() == [0, 2]


# ------------------------------------------------------------------------------------------------ 4, 7: GraphedStep(train_pose=True)
def _graphed_sequence(use_graph, depth, deg=3):
    """Six steps alternating view 0, 1 on a GraphedStep(train_pose=True): (map state, pose-set state, the six steps' terms)."""
    from gaussian_lic_amd import trainer
    raw, cams, gts, gtd, bg = _setup(deg)
    model = training_model(raw)
    ps = _pose_set(cams, lr_trans=2e-3, lr_rot=1e-3)
    start = _pose_state(ps)
    kw = dict(gt_depth=gtd, lambda_depth=LAMBDA_D) if depth else {}
    gs = trainer.GraphedStep(model, cams[0], gts[0], bg, use_graph=use_graph, poses=ps, view=0, train_pose=True, **kw)
    _same(_pose_state(ps), start)                                                     # warm-up and capture passes left the set as it was
    terms = [gs.step(gt_image=gts[k % 2], view=k % 2).clone() for k in range(6)]
    assert gs.check() == 0
    return model_state(model), _pose_state(ps), torch.stack(terms).cpu()


def _eager_sequence(depth, deg=3):
    from gaussian_lic_amd import loss, trainer
    raw, cams, gts, gtd, bg = _setup(deg)
    model = training_model(raw)
    ps = _pose_set(cams, lr_trans=2e-3, lr_rot=1e-3)
    kw = dict(gt_depth=gtd, lambda_depth=LAMBDA_D) if depth else {}
    fl = loss.FusedLoss(0.2)
    terms = [trainer.training_step_with_pose(model, cams[0], gts[k % 2], bg, fused_loss=fl, poses=ps, view=k % 2, adam_in_backward=True, **kw)[0].clone()
             for k in range(6)]
    torch.cuda.synchronize()
    return model_state(model), _pose_state(ps), torch.stack(terms).cpu()


@pytest.mark.parametrize("depth", [False, True])
@pytest.mark.parametrize("use_graph", [False, True])
def test_graphed_step_trains_the_pose(use_graph, depth):
    got = _graphed_sequence(use_graph, depth)
    want = _eager_sequence(depth)
    assert_same_state(got[0], want[0])
    _same(got[1], want[1])
    assert torch.equal(bits(got[2]), bits(want[2]))
    assert got[1]["steps"].tolist() == [3, 3]
    again = _graphed_sequence(use_graph, depth)                                       # run to run: the same bits
    assert_same_state(got[0], again[0])
    _same(got[1], again[1])
    assert torch.equal(bits(got[2]), bits(again[2]))


def test_graphed_step_without_train_pose_leaves_the_set_untouched():
    from gaussian_lic_amd import trainer
    raw, cams, gts, gtd, bg = _setup(3)
    model = training_model(raw)
    ps = _pose_set(cams, lr_trans=2e-3, lr_rot=1e-3)
    start = _pose_state(ps)
    gs = trainer.GraphedStep(model, cams[0], gts[0], bg, poses=ps, view=0, train_pose=False)
    assert gs._cam_grads is None
    gs.step(view=1)
    assert gs.check() == 0
    _same(_pose_state(ps), start)


# ------------------------------------------------------------------------------------------------ 5: overflow
@pytest.mark.parametrize("depth", [False, True])
def test_a_step_that_did_not_fit_moves_neither_map_nor_pose(depth):
    from gaussian_lic_amd import loss, trainer
    raw, cams, gts, gtd, bg = _setup(3)
    kw = dict(gt_depth=gtd, lambda_depth=LAMBDA_D) if depth else {}
    a, b = training_model(raw), training_model(raw)
    ps_a, ps_b = (_pose_set(cams, lr_trans=2e-3, lr_rot=1e-3) for _ in range(2))
    with torch.no_grad():
        sizing = trainer._RawRaster(a, cams[0], bg, False, pose=ps_a.pose(1))
        sizing.forward()
        R = int(sizing.state[0])
    assert R > 8
    map0, pose0 = model_state(a), _pose_state(ps_a)
    gs = trainer.GraphedStep(a, cams[0], gts[1], bg, poses=ps_a, view=1, train_pose=True, cap_R=R // 2, check_every=0, **kw)
    gs._cam_grads.fill_(-7.0)
    gs.step()
    torch.cuda.synchronize()
    assert_same_state(map0, model_state(a))                                           # the library's own no-op path
    after = _pose_state(ps_a)
    for k in ("view", "proj", "campos", "m", "v", "steps"):
        assert torch.equal(bits(after[k]), bits(pose0[k])), k
    assert bool((gs._cam_grads == 0).all()) and bool((ps_a.grad == 0).all())
    assert gs.check() == 1 and gs.cap_R >= R
    trainer.training_step_with_pose(b, cams[0], gts[1], bg, fused_loss=loss.FusedLoss(0.2), poses=ps_b, view=1, adam_in_backward=True, **kw)
    torch.cuda.synchronize()
    assert_same_state(model_state(a), model_state(b))
    _same(_pose_state(ps_a), _pose_state(ps_b))
    assert ps_a.steps.tolist() == [0, 1]


# ------------------------------------------------------------------------------------------------ 6: refusals
def test_refusals():
    from gaussian_lic_amd import trainer
    assert run_refusal_cases() > 0                                                    # every GSLIC_ERR_INVALID_ARG case, through _lib
    raw, cams, gts, gtd, bg = _setup(3)
    model = training_model(raw)
    ps = _pose_set(cams)
    with pytest.raises(ValueError, match="train_pose=True needs poses"):
        trainer.GraphedStep(model, cams[0], gts[0], bg, train_pose=True)
    with pytest.raises(NotImplementedError, match="grad_stats"):
        trainer.GraphedStep(model, cams[0], gts[0], bg, poses=ps, view=0, train_pose=True, grad_stats=trainer.GradientStats(model))
    gs = trainer.GraphedStep(model, cams[0], gts[0], bg, poses=ps, view=0, train_pose=True)
    with pytest.raises(ValueError, match="built on a pose set"):
        gs.step(camera=cams[1])
    with pytest.raises(IndexError):
        gs.step(view=2)


# ------------------------------------------------------------------------------------------------ 8: the C++ host
@pytest.mark.parametrize("depth", [False, True])
def test_fused_pose_adam_cpp_host(tmp_path, depth):
    """gslic::FusedStep::step_with_pose issues the C-ABI calls of trainer.training_step_with_pose(poses=, adam_in_backward=True): map, moments, the
    set and every step's terms and gradient are bit-identical to the Python host's over three steps on two views."""
    from gaussian_lic_amd import loss, trainer
    exe = fio.build("fused_pose_adam")
    iters, lr_t, lr_r = 3, 2e-3, 1e-3
    raw, cams, gts, gtd, bg = _setup(3)
    ps = _pose_set(cams, lr_trans=lr_t, lr_rot=lr_r)
    d = str(tmp_path)
    fio.write_inputs(d, raw, cams, gt=gts[0], gt2=gts[1], gt_depth=gtd, projection=ps.projection)
    fio.run(exe, d, str(P_), str(W_), str(H_), "3", str(iters), repr(lr_t), repr(lr_r), repr(LAMBDA_D if depth else 0.0))
    model, fl = training_model(raw), loss.FusedLoss(0.2)
    kw = dict(gt_depth=gtd, lambda_depth=LAMBDA_D) if depth else {}
    terms, grads = [], []
    for it in range(iters):
        t, _vis, g = trainer.training_step_with_pose(model, cams[0], gts[it % 2], bg, fused_loss=fl, poses=ps, view=it % 2, adam_in_backward=True, **kw)
        terms.append(t.clone()); grads.append(g.clone())
    torch.cuda.synchronize()
    rd = lambda name: fio.read(d, name, np.int32)
    for name in ("view", "proj", "campos", "m", "v"):
        assert torch.equal(rd(f"pose_{name}.f32"), bits(getattr(ps, name).cpu()).reshape(-1)), name
    assert rd("pose_steps.i32").tolist() == ps.steps.tolist() == [2, 1]
    assert torch.equal(rd("pose_grads.f32"), bits(torch.stack(grads).cpu()).reshape(-1))
    assert torch.equal(rd("terms.f32"), bits(torch.stack(terms).cpu()).reshape(-1))
    rows, state = fio.read_rows(d, 15), model_state(model)
    for name, key in (("xyz", "xyz"), ("scaling", "scaling"), ("rotation", "rotation"), ("opacity", "opacity"), ("features_dc", "dc"), ("features_rest", "rest")):
        assert torch.equal(rows[key], bits(state[name]).reshape(-1)), name
        assert torch.equal(rows["m_" + key], bits(state[name + ".m"]).reshape(-1)) and torch.equal(rows["v_" + key], bits(state[name + ".v"]).reshape(-1)), name
