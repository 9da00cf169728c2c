"""-m gpu: the trainable pose set — gslic_pose_step / gslic_pose_load on made-up camera gradients against the float64 restatement of their rule
(tests/pose_ref.py), with guard words around every array, and trainer.PoseSet through pose_gradient, training_step_with_pose, GraphedStep (eager
and captured) and the C++ host.

The margins are not chosen: each is 4x the largest gap to the float64 restatement measured on one MI355X over the cases of the test that sets it
(the rule of contribution_ref.MARGIN), relative to the array's largest magnitude.  Every test prints its figures before it asserts."""
import functools

import numpy as np
import pytest
import torch

import fused_check_io as fio
import pose_ref as ref
from conftest import make_scene
from gpu_helpers import assert_same_state, bits, gpu, guarded, guards_intact, model_state, training_model

pytestmark = pytest.mark.gpu

V = 3
# measured on one MI355X (test_one_step_and_eight_steps_against_the_float64_rule, 24 runs: four cases x three gradient scales x one and eight
# steps): largest gap of view / proj / campos / m / v 3.818e-07 (closed branch, eight steps), of grad_out against Camera.pose_gradient 3.393e-07,
# each relative to the array's largest magnitude
STATE_MARGIN = 4 * 3.818e-07
GRAD_MARGIN = 4 * 3.393e-07
# measured (test_trajectory_of_five_pose_steps_against_the_host_route): largest gap of the row's view / campos to the host route's camera after
# five steps 1.257e-05 (the host route rounds its float64 pose to float32 matrices at every step, the row is float32 throughout)
TRAJECTORY_MARGIN = 4 * 1.257e-05
STATE = ("view", "proj", "campos", "m", "v")


def _cams(W=96, H=64):
    from gaussian_lic_amd.camera import synthetic_camera
    return [synthetic_camera(W, H, v) for v in ("se3_c", "se3_d", 2)]


class Guarded:
    """A PoseSet of V views whose eight device arrays each sit between two runs of guard words."""

    NAMES = ("view", "proj", "campos", "m", "v", "steps", "projection", "grad")

    def __init__(self, cams=None, **kw):
        from gaussian_lic_amd import trainer
        cams = cams or _cams()
        self.ps = ps = trainer.PoseSet(V, cams[0], gpu(), **kw)
        for i in range(1, V):
            ps.load(i, cams[i])
        self.bufs = {}
        for name in self.NAMES:
            t = getattr(ps, name)
            buf, words = guarded(t.numel(), dtype=t.dtype)
            words.copy_(t.reshape(-1))
            setattr(ps, name, words.view(t.shape))
            self.bufs[name] = (buf, t.numel())

    def intact(self):
        return all(guards_intact(buf, n) for buf, n in self.bufs.values())

    def row(self, i):
        """Row i on the host, as pose_ref.step takes it (float32 values held in float64)."""
        ps = self.ps
        return dict(view=ps.view[i].cpu().numpy().astype(np.float64), proj=ps.proj[i].cpu().numpy().astype(np.float64),
                    campos=ps.campos[i].cpu().numpy().astype(np.float64), m=ps.m[i].cpu().numpy().astype(np.float64),
                    v=ps.v[i].cpu().numpy().astype(np.float64), steps=int(ps.steps[i]))

    def snapshot(self):
        return {k: getattr(self.ps, k).clone() for k in self.NAMES}


def _grads(seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return tuple((rng.normal(size=n) * scale).astype(np.float32) for n in (16, 16, 3))


def _dev(grads):
    return tuple(torch.from_numpy(g).to(gpu()) for g in grads)


def _gap(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


def _same(a, b, names):
    for k in names:
        assert torch.equal(bits(a[k]), bits(b[k])), k


# ------------------------------------------------------------------------------------------------ the kernels alone
def test_load_is_a_bit_copy_and_pose_load_copies_exactly_the_named_row():
    from gaussian_lic_amd import _lib
    cams = _cams()
    g = Guarded(cams)
    ps = g.ps
    for i, cam in enumerate(cams):
        v, p, c = ps.pose(i)
        assert torch.equal(bits(v.cpu()), bits(torch.from_numpy(cam.world_view_transform.reshape(16))))
        assert torch.equal(bits(p.cpu()), bits(torch.from_numpy(cam.full_proj_transform.reshape(16))))
        assert torch.equal(bits(c.cpu()), bits(torch.from_numpy(cam.camera_center.reshape(3))))
        assert v.data_ptr() == ps.view[i].data_ptr()                                # no copy
    outs = [guarded(n, dtype=torch.float32, fill=-7.0) for n in (16, 16, 3)]
    word = torch.zeros(1, dtype=torch.int32, device=gpu())
    for i in (1, 2, 0):
        word.fill_(i)
        ps._load_row(word, *(w for _b, w in outs))
        for (buf, w), src in zip(outs, (ps.view, ps.proj, ps.campos)):
            assert torch.equal(bits(w), bits(src[i])) and guards_intact(buf, w.numel())
    for (_b, w) in outs:
        w.fill_(-7.0)
    for bad in (-1, V, 1 << 30):                                                     # an out-of-range word writes nothing
        word.fill_(bad)
        ps._load_row(word, *(w for _b, w in outs))
        assert all(bool((w == -7.0).all()) and guards_intact(b, w.numel()) for b, w in outs)
    assert g.intact()
    assert _lib.lib().gslic_abi_version() == 8


# lr_trans, lr_rot: the first Adam step moves every coordinate by about its rate, so theta ~ sqrt(3) lr_rot.  What the "series" case shows is that
# the branch is taken and joins the closed one without a step or a NaN: at theta ~ 3.5e-5 the theta^2 terms of the three series are below 1e-9
# of their leading terms, far under float32 and the margin, so a wrong second coefficient could not be seen here (the series' own arithmetic is
# checked where it is visible, at theta = 0.05 .. 0.2, by tests/test_pose_set_cpu.py on pose_ref).
CASES = {
    "series": dict(lr_trans=1e-3, lr_rot=2e-5),          # theta ~ 3.5e-5 < GSLIC_POSE_SERIES_THETA
    "closed": dict(lr_trans=1e-2, lr_rot=0.3),           # theta ~ 0.52 rad
    "translation": dict(lr_trans=5e-3, lr_rot=0.0),
    "rotation": dict(lr_trans=0.0, lr_rot=1e-2),
}


def _run_against_ref(name, kw, scale, n_steps, row=1):
    """n_steps device steps on one row against pose_ref from the same start: (largest state gap, largest gradient gap, the Guarded)."""
    g = Guarded(**kw)
    ps = g.ps
    want = g.row(row)
    proj64 = ps.projection.cpu().numpy().astype(np.float64)
    state_gap = grad_gap = 0.0
    for k in range(n_steps):
        grads = _grads(1000 * len(name) + k, scale)
        cam = ps.camera(row)                                                         # the row's 35 floats as a host Camera, before the step
        ps.adam_step(row, _dev(grads))
        want, _g64 = ref.step(want, proj64, grads, kw["lr_trans"], kw["lr_rot"])
        grad_gap = max(grad_gap, _gap(ps.grad.cpu().numpy(), cam.pose_gradient(*grads)))
        got = g.row(row)
        assert got["steps"] == want["steps"] == k + 1
        state_gap = max(state_gap, max(_gap(got[a], want[a]) for a in STATE))
    assert g.intact()
    return state_gap, grad_gap, g


def test_one_step_and_eight_steps_against_the_float64_rule():
    worst_state = worst_grad = 0.0
    for name, kw in CASES.items():
        for scale in (1e-3, 1.0, 1e2):
            for n_steps in (1, 8):
                s, gr, g = _run_against_ref(name, kw, scale, n_steps)
                print(f"pose step {name:11s} scale {scale:g} steps {n_steps}: state gap {s:.3e} grad gap {gr:.3e}")
                worst_state, worst_grad = max(worst_state, s), max(worst_grad, gr)
                row = g.row(1)
                assert all(np.isfinite(row[a]).all() for a in STATE)
    print(f"pose step: largest state gap {worst_state:.3e} (bar {STATE_MARGIN:.3e}), largest grad gap {worst_grad:.3e} (bar {GRAD_MARGIN:.3e})")
    assert worst_state <= STATE_MARGIN and worst_grad <= GRAD_MARGIN
    # the two branches were reached: theta of the first step on either side of the threshold
    for name, below in (("series", True), ("closed", False)):
        kw = CASES[name]
        d, *_ = ref.adam(ref.chain(Guarded(**kw).row(1)["view"], _cams()[0].projection_matrix.reshape(16), *_grads(1000 * len(name))),
                         np.zeros(6), np.zeros(6), 0, kw["lr_trans"], kw["lr_rot"])
        theta = float(np.linalg.norm(d[3:]))
        assert (theta < ref.SERIES_THETA) == below and (below or 0.4 < theta < 0.6)


def test_only_the_named_row_changes_and_its_count_advances_by_one():
    g = Guarded(lr_trans=1e-3, lr_rot=1e-3)
    ps = g.ps
    ps.m.copy_(torch.arange(V * 6, device=gpu()).view(V, 6) * 0.01)
    ps.v.copy_(torch.arange(V * 6, device=gpu()).view(V, 6) * 0.001 + 0.5)
    ps.steps.copy_(torch.tensor([3, 5, 9], dtype=torch.int32))
    before = g.snapshot()
    ps.adam_step(1, _dev(_grads(7)))
    after = g.snapshot()
    for k in ("view", "proj", "campos", "m", "v"):
        for i in (0, 2):
            assert torch.equal(bits(after[k][i]), bits(before[k][i])), (k, i)
        assert not torch.equal(after[k][1], before[k][1]), k
    assert after["steps"].tolist() == [3, 6, 9]
    assert torch.equal(bits(after["projection"]), bits(before["projection"])) and g.intact()


def test_the_three_no_ops():
    import ctypes
    from gaussian_lic_amd import _lib
    grads = _grads(11)
    dv, dp, dc = _dev(grads)
    # skip word with one of the bits 1 | 2 | 8 | 16 set (alone, or beside the bit 4 that does not count): nothing but grad_out
    for word in (1, 2, 8, 16, 4 | 16, 27):
        g = Guarded(lr_trans=1e-3, lr_rot=1e-3)
        ps, before = g.ps, g.snapshot()
        ps.grad.fill_(-3.0)
        skip_word = torch.tensor([word], dtype=torch.int32, device=gpu())
        d = ps._descriptor(ps._views[1:2], skip_word)
        _lib.check(_lib.lib().gslic_pose_step(ctypes.byref(d), _lib.ptr(dv), _lib.ptr(dp), _lib.ptr(dc), _lib.ptr(ps.grad), _lib.current_stream_ptr()))
        after = g.snapshot()
        _same(after, before, ("view", "proj", "campos", "m", "v", "steps", "projection"))
        assert _gap(ps.grad.cpu().numpy(), ref.chain(g.row(1)["view"], ps.projection.cpu().numpy(), *grads)) <= GRAD_MARGIN and g.intact(), word
    # a word without those bits (0, or bit 4 alone) is no skip: the row steps
    for word in (0, 4):
        g = Guarded(lr_trans=1e-3, lr_rot=1e-3)
        ps, before = g.ps, g.snapshot()
        skip_word = torch.tensor([word], dtype=torch.int32, device=gpu())
        d = ps._descriptor(ps._views[1:2], skip_word)
        _lib.check(_lib.lib().gslic_pose_step(ctypes.byref(d), _lib.ptr(dv), _lib.ptr(dp), _lib.ptr(dc), _lib.ptr(ps.grad), _lib.current_stream_ptr()))
        after = g.snapshot()
        assert after["steps"].tolist() == [0, 1, 0] and not torch.equal(after["view"][1], before["view"][1]) and g.intact(), word
    # a NaN or an inf in the gradient: state and steps untouched
    for bad in (float("nan"), float("inf")):
        g = Guarded(lr_trans=1e-3, lr_rot=1e-3)
        ps, before = g.ps, g.snapshot()
        poisoned = tuple(a.copy() for a in grads)
        poisoned[0][13] = bad
        ps.adam_step(1, _dev(poisoned))
        after = g.snapshot()
        _same(after, before, ("view", "proj", "campos", "m", "v", "steps", "projection"))
        assert not bool(torch.isfinite(ps.grad).all()) and g.intact()
        assert all(bool(torch.isfinite(after[k]).all()) for k in ("view", "proj", "campos", "m", "v"))
    # both rates 0: delta is zero — the pose keeps its bits, the moments and the count move
    g = Guarded(lr_trans=0.0, lr_rot=0.0)
    ps, before = g.ps, g.snapshot()
    ps.adam_step(1, _dev(grads))
    after = g.snapshot()
    _same(after, before, ("view", "proj", "campos", "projection"))
    assert after["steps"].tolist() == [0, 1, 0] and bool((after["m"][1] != 0).all()) and bool((after["v"][1] > 0).all())
    want, _g = ref.step(Guarded(lr_trans=0.0, lr_rot=0.0).row(1), ps.projection.cpu().numpy(), grads, 0.0, 0.0)
    assert max(_gap(g.row(1)[a], want[a]) for a in ("m", "v")) <= STATE_MARGIN
    assert all(bool(torch.isfinite(after[k]).all()) for k in ("view", "proj", "campos", "m", "v", "grad")) and g.intact()


def _ortho_error(view16):
    R = ref.mat(view16)[:3, :3]
    return float(np.abs(R @ R.T - np.eye(3)).max())


def test_256_steps_accumulate_no_drift_in_R():
    g = Guarded(lr_trans=5e-3, lr_rot=1e-2)
    ps = g.ps
    rng = np.random.default_rng(5)
    first = []
    for k in range(256):
        grads = tuple((rng.normal(size=n) * 10.0 ** rng.uniform(-2, 2)).astype(np.float32) for n in (16, 16, 3))
        ps.adam_step(2, _dev(grads))
        if k < 8:
            first.append(_ortho_error(g.row(2)["view"]))
    bar = 4.0 * max(first)                                  # measured here, on the device: 4x the largest value over the first eight steps
    row = g.row(2)
    last = _ortho_error(row["view"])
    print(f"pose drift: max|R R^T - I| over the first 8 steps {max(first):.3e} (one step {first[0]:.3e}), after 256 steps {last:.3e}, bar {bar:.3e}")
    # (measured on one MI355X: 1.709e-07 after one step, 2.912e-07 the largest over the first eight, 1.713e-07 after 256)
    assert 0.0 < bar and last <= bar and row["steps"] == 256
    Vm = ref.mat(row["view"])
    assert _gap(row["campos"], -(Vm[:3, :3].T @ Vm[:3, 3])) <= STATE_MARGIN
    assert _gap(row["proj"], ref.flat(ref.mat(ps.projection.cpu().numpy()) @ Vm)) <= STATE_MARGIN
    moved = float(np.abs(row["view"] - Guarded().row(2)["view"]).max())
    print(f"pose drift: the view matrix moved by {moved:.3e} over the 256 steps")
    assert moved > 1e-3 and g.intact()                     # the 256 steps went somewhere


def test_two_runs_from_the_same_state_give_the_same_bits():
    runs = []
    for _ in range(2):
        g = Guarded(lr_trans=2e-3, lr_rot=4e-3)
        grad_bits = []
        for k in range(8):
            g.ps.adam_step(k % V, _dev(_grads(40 + k, 10.0 ** (k % 3 - 1))))
            grad_bits.append(bits(g.ps.grad).clone())
        runs.append((g.snapshot(), torch.stack(grad_bits)))
        assert g.intact()
    _same(runs[0][0], runs[1][0], Guarded.NAMES)
    assert torch.equal(runs[0][1], runs[1][1])


# ------------------------------------------------------------------------------------------------ the steps
P_, W_, H_ = 400, 64, 48
LAMBDA_D = 0.5


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
    return {k: getattr(ps, k).cpu().clone() for k in ("view", "proj", "campos", "m", "v", "steps")}


@pytest.mark.parametrize("depth", [False, True])
def test_pose_gradient_on_a_row_is_the_host_routes_gradient(depth):
    from gaussian_lic_amd import loss, trainer
    raw, cams, gts, gtd, bg = _setup(1 if depth else 3)
    model = training_model(raw)
    ps = _pose_set(cams, lr_trans=1e-3, lr_rot=1e-3)
    kw = dict(gt_depth=gtd, lambda_depth=LAMBDA_D) if depth else {}
    before, ps_before = model_state(model), _pose_state(ps)
    want, terms_h = trainer.pose_gradient(model, cams[1], gts[1], bg, fused_loss=loss.FusedLoss(0.2), **kw)
    got, terms_d = trainer.pose_gradient(model, cams[0], gts[1], bg, fused_loss=loss.FusedLoss(0.2), poses=ps, view=1, **kw)
    assert got is ps.grad and got.is_cuda and got.dtype == torch.float32
    gap = _gap(got.cpu().numpy(), want)
    print(f"pose_gradient(poses=) depth={depth}: gap to the host route {gap:.3e} (bar {GRAD_MARGIN:.3e}), |g| max {np.abs(want).max():.3e}")
    assert gap <= GRAD_MARGIN and np.abs(want).max() > 0
    assert torch.equal(bits(terms_d), bits(terms_h)) and terms_d.numel() == (3 if depth else 2)
    assert_same_state(before, model_state(model))
    _same(_pose_state(ps), ps_before, ps_before.keys())                             # do_step=False moves nothing
    with pytest.raises(ValueError, match="differ from the pose set"):
        from gaussian_lic_amd.camera import synthetic_camera
        trainer.pose_gradient(model, synthetic_camera(W_ + 16, H_).to_device(gpu()), gts[1], bg, poses=ps, view=1)


@pytest.mark.parametrize("with_exposure", [False, True])
def test_training_step_with_pose_on_a_row(with_exposure):
    from gaussian_lic_amd import loss, trainer
    raw, cams, gts, gtd, bg = _setup(3)
    a, b, c = training_model(raw), training_model(raw), training_model(raw)
    lr_t, lr_r = 2e-3, 1e-3
    ps = _pose_set(cams, lr_trans=lr_t, lr_rot=lr_r)
    ps_before = _pose_state(ps)
    ex_a = trainer.Exposure(2, gpu(), lr=0.01) if with_exposure else None
    ex_b = ex_a.clone() if with_exposure else None
    kw = lambda ex: dict(exposure=ex, view=1) if ex is not None else dict(view=1)
    terms_a, vis_a, g_a = trainer.training_step_with_pose(a, cams[0], gts[1], bg, fused_loss=loss.FusedLoss(0.2), poses=ps, **kw(ex_a))
    terms_b, vis_b, g_b = trainer.training_step_with_pose(b, cams[1], gts[1], bg, pose_lr=0.0, fused_loss=loss.FusedLoss(0.2), **kw(ex_b))
    assert g_a is ps.grad and torch.equal(bits(terms_a), bits(terms_b)) and torch.equal(vis_a, vis_b)
    assert_same_state(model_state(a), model_state(b))                               # the same calls: parameters and both moments on bits
    for n in a.NAMES:
        assert torch.equal(bits(getattr(a, n).detach()), bits(getattr(b, n).detach())), n
    if with_exposure:
        for k in ("params", "m", "v", "steps", "grad"):
            assert torch.equal(bits(getattr(ex_a, k)), bits(getattr(ex_b, k))), k
        assert ex_a.steps.tolist() == [0, 1]
    assert _gap(g_a.cpu().numpy(), g_b) <= GRAD_MARGIN
    after = _pose_state(ps)
    if not with_exposure:
        # the row against pose_ref on the step's own camera gradients (the same forward, loss and camera backward on a third copy of the map)
        with torch.no_grad():
            rr = trainer._RawRaster(c, cams[1], bg, False)
            image, _d, _r = rr.forward()
            dL_dimage, _dd, _t = trainer._fused_losses(loss.FusedLoss(0.2), image, gts[1], None, None, 0.0)
            out = rr.backward(dL_dimage, None, camera_grads=True)
        grads = tuple(t.cpu().numpy() for t in out[9:12])
        row0 = {k: ps_before[k][1].numpy().astype(np.float64) for k in STATE}
        row0["steps"] = 0
        want, _g = ref.step(row0, ps.projection.cpu().numpy().astype(np.float64), grads, lr_t, lr_r)
        gap = max(_gap(after[k][1].numpy(), want[k]) for k in STATE)
        print(f"training_step_with_pose(poses=): row gap to pose_ref {gap:.3e} (bar {STATE_MARGIN:.3e})")
        assert gap <= STATE_MARGIN
    assert after["steps"].tolist() == [0, 1] and not torch.equal(after["view"][1], ps_before["view"][1])
    for k in STATE:
        assert torch.equal(bits(after[k][0]), bits(ps_before[k][0])), k             # the other view's row is untouched
    with pytest.raises(ValueError, match="pose_lr"):
        trainer.training_step_with_pose(a, cams[0], gts[1], bg, pose_lr=1e-3, poses=ps, view=1)


def test_trajectory_of_five_pose_steps_against_the_host_route():
    """A camera perturbed by xi = (3, -2, 4 mm; 2, -3, 1.5 mrad) looks at the map's own render from the unperturbed pose; five pose-only Adam steps
    (the map fixed) on the device against five on the host route (pose_gradient in float64, pose_ref.adam, apply_pose_increment)."""
    from gaussian_lic_amd import loss, trainer
    from gaussian_lic_amd.camera import synthetic_camera
    raw, cams, gts, gtd, bg = _setup(3)
    model = training_model(raw)
    with torch.no_grad():
        gt = trainer._RawRaster(model, cams[0], bg, False).forward()[0].clone()
    xi = np.array([3e-3, -2e-3, 4e-3, 2e-3, -3e-3, 1.5e-3])
    lr_t = lr_r = 5e-4
    fl = loss.FusedLoss(0.2)
    host = synthetic_camera(W_, H_).apply_pose_increment(xi).to_device(gpu())
    ps = trainer.PoseSet(1, cams[0], gpu(), lr_trans=lr_t, lr_rot=lr_r)
    ps.load(0, host)
    loss_of = lambda terms: float(fl.value(terms))
    m, v, n = np.zeros(6), np.zeros(6), 0
    host_losses, dev_losses = [], []
    for _ in range(5):
        g, terms = trainer.pose_gradient(model, host, gt, bg, fused_loss=fl)
        host_losses.append(loss_of(terms))
        delta, m, v, n = ref.adam(g, m, v, n, lr_t, lr_r)
        host.apply_pose_increment(delta).to_device(gpu())
    host_losses.append(loss_of(trainer.pose_gradient(model, host, gt, bg, fused_loss=fl)[1]))
    for _ in range(5):
        _g, terms = trainer.pose_gradient(model, cams[0], gt, bg, fused_loss=fl, poses=ps, view=0, do_step=True)
        dev_losses.append(terms.clone())
    dev_losses.append(trainer.pose_gradient(model, cams[0], gt, bg, fused_loss=fl, poses=ps, view=0)[1].clone())
    dev_losses = [loss_of(t) for t in dev_losses]
    gap = max(_gap(ps.view[0].cpu().numpy(), host.world_view_transform.reshape(16)), _gap(ps.campos[0].cpu().numpy(), host.camera_center))
    print(f"pose trajectory: host losses {host_losses[0]:.6e} -> {host_losses[-1]:.6e}, device {dev_losses[0]:.6e} -> {dev_losses[-1]:.6e}, "
          f"gap of the row to the host camera after five steps {gap:.3e} (bar {TRAJECTORY_MARGIN:.3e})")
    assert host_losses[-1] < host_losses[0], "the scene and xi must let the host route itself reduce the loss"
    assert dev_losses[-1] < dev_losses[0]
    assert gap <= TRAJECTORY_MARGIN and ps.steps.tolist() == [5]


def test_one_set_serves_pyramid_level_1():
    """A set built from the level-0 camera, row 1 moved by a step: pose_gradient on cam.at_level(1) is the host route's gradient on the row's
    level-1 camera, and a GraphedStep on a keyframe store at level 1 reads its pose from the same set."""
    from gaussian_lic_amd import loss, trainer
    from gaussian_lic_amd.synthetic import gt_image
    raw, cams, gts, gtd, bg = _setup(3)
    ps = _stepped_pose_set(cams)
    lvl = ps.camera(1, level=1)
    assert (lvl.image_width, lvl.image_height) == (W_ // 2, H_ // 2)
    gt1 = gt_image(H_ // 2, W_ // 2, seed=9).to(gpu())
    model = training_model(raw)
    want, terms_h = trainer.pose_gradient(model, lvl, gt1, bg, fused_loss=loss.FusedLoss(0.2))
    got, terms_d = trainer.pose_gradient(model, cams[0].at_level(1), gt1, bg, fused_loss=loss.FusedLoss(0.2), poses=ps, view=1)
    gap = _gap(got.cpu().numpy(), want)
    print(f"pose_gradient(poses=) at level 1: gap to the host route {gap:.3e} (bar {GRAD_MARGIN:.3e}), |g| max {np.abs(want).max():.3e}")
    assert gap <= GRAD_MARGIN and np.abs(want).max() > 0 and torch.equal(bits(terms_d), bits(terms_h))
    store = trainer.KeyframeStore(W_, H_, 2, gpu())
    for gt in gts:
        store.add(gt)
    a, b = training_model(raw), training_model(raw)
    gs = trainer.GraphedStep(a, cams[0], None, bg, keyframes=store, frame=0, level=1, poses=ps, view=0)
    plain = trainer.GraphedStep(b, cams[0], None, bg, keyframes=store, frame=0, level=1)
    assert (gs.W, gs.H) == (W_ // 2, H_ // 2)
    ta = gs.step(view=1, frame=1).clone()
    tb = plain.step(camera=lvl, frame=1).clone()
    assert torch.equal(bits(ta), bits(tb)) and gs.check() == 0 and plain.check() == 0
    assert_same_state(model_state(a), model_state(b))


def test_a_set_on_a_device_given_without_an_index_steps():
    from gaussian_lic_amd import trainer
    cams = _cams()
    ps = trainer.PoseSet(2, cams[0], "cuda", lr_trans=1e-3, lr_rot=1e-3)
    g = ps.adam_step(1, tuple(t.to("cuda") for t in _dev(_grads(2))))
    assert g is ps.grad and ps.steps.tolist() == [0, 1] and bool(g.abs().min() > 0)
    assert ps.camera(1).d_world_view_transform.device == ps.view.device


def test_fused_pose_cpp_host(tmp_path):
    """gslic::PoseSet and the pose-set overload of FusedStep::pose_gradient issue the C-ABI calls of trainer.pose_gradient(poses=, view=,
    do_step=True): the rows, the moments, the step counts and every step's gradient are bit-identical to the Python host's over three steps on
    two views.  (The pose files go through fused_check_io's extra float32 arrays and its reader of out_ files.)"""
    from gaussian_lic_amd import loss, trainer
    exe = fio.build("fused_pose")
    iters, lr_t, lr_r = 3, 2e-3, 1e-3
    raw, cams, gts, gtd, bg = _setup(3)
    ps = _pose_set(cams, lr_trans=lr_t, lr_rot=lr_r)
    d = str(tmp_path)
    fio.write_inputs(d, raw, cams, gt=gts[0], gt2=gts[1], projection=ps.projection)
    fio.run(exe, d, str(P_), str(W_), str(H_), "3", str(iters), repr(lr_t), repr(lr_r))
    model, fl = training_model(raw), loss.FusedLoss(0.2)
    grads = [trainer.pose_gradient(model, cams[0], gts[it % 2], bg, fused_loss=fl, poses=ps, view=it % 2, do_step=True)[0].clone() for it in range(iters)]
    rd = lambda name: fio.read(d, name, np.int32)
    for name in ("view", "proj", "campos", "m", "v"):
        assert torch.equal(rd(f"pose_{name}.f32"), bits(getattr(ps, name).cpu()).reshape(-1)), name
    assert rd("pose_steps.i32").tolist() == ps.steps.tolist() == [2, 1]
    assert torch.equal(rd("pose_grads.f32"), bits(torch.stack(grads).cpu()).reshape(-1))
    assert bool(torch.stack(grads).abs().min() > 0)
    # gslic::PoseSet::clone and reset_moments(0) on the clone: the rows and the last gradient by value, row 0's state zeroed in the clone alone
    assert torch.equal(rd("clone_view.f32"), bits(ps.view.cpu()).reshape(-1)) and torch.equal(rd("clone_grad.f32"), bits(ps.grad.cpu()).reshape(-1))
    m_clone = ps.m.cpu().clone()
    m_clone[0] = 0
    assert torch.equal(rd("clone_m.f32"), bits(m_clone).reshape(-1))
    assert rd("clone_steps.i32").tolist() == [0, 1] and rd("pose_steps_after_clone.i32").tolist() == [2, 1]


def _stepped_pose_set(cams):
    """Two rows, row 1 moved by one step on made-up gradients: a pose no host Camera produced."""
    ps = _pose_set(cams, lr_trans=2e-3, lr_rot=2e-3)
    ps.adam_step(1, _dev(_grads(3)))
    return ps


def test_graphed_step_reads_its_pose_from_the_set():
    from gaussian_lic_amd import trainer
    raw, cams, gts, gtd, bg = _setup(3)
    a, b = training_model(raw), training_model(raw)
    ps = _stepped_pose_set(cams)
    ps_before = _pose_state(ps)
    gs = trainer.GraphedStep(a, cams[0], gts[0], bg, poses=ps, view=0)
    plain = trainer.GraphedStep(b, cams[0], gts[0], bg)
    ta = gs.step(view=1).clone()
    tb = plain.step(camera=ps.camera(1)).clone()
    assert torch.equal(bits(ta), bits(tb)) and gs.check() == 0 and plain.check() == 0
    assert_same_state(model_state(a), model_state(b))
    assert torch.equal(bits(gs.view).reshape(16), bits(ps.view[1])) and torch.equal(bits(gs.campos).reshape(3), bits(ps.campos[1]))
    _same(_pose_state(ps), ps_before, ps_before.keys())                             # the graphed step trains no pose
    with pytest.raises(ValueError, match="built on a pose set"):
        gs.step(camera=cams[1])
    with pytest.raises(ValueError, match="built without"):
        plain.step(view=1)
    with pytest.raises(IndexError):
        gs.step(view=2)


def test_captured_step_changes_keyframe_pose_through_the_device_word():
    """The captured-view case of tests/test_exposure_gpu.py with a pose set in the exposure's place: same order of host synchronisation and device
    work around the replays."""
    from gaussian_lic_amd import trainer
    raw, cams, gts, gtd, bg = _setup(3)
    a, b = training_model(raw), training_model(raw)
    ps = _stepped_pose_set(cams)
    row_cams = [ps.camera(0), ps.camera(1)]
    ps_before = _pose_state(ps)
    gs = trainer.GraphedStep(a, cams[0], gts[0], bg, use_graph=True, poses=ps, view=0)
    for k in (0, 1, 0, 1):
        tg = gs.step(gt_image=gts[k], view=k).clone()
        te = trainer.training_step_fused(b, row_cams[k], gts[k], bg)[0]
        assert torch.equal(bits(tg), bits(te))
    assert gs.check() == 0
    assert_same_state(model_state(a), model_state(b))
    _same(_pose_state(ps), ps_before, ps_before.keys())
