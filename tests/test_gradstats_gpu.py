"""-m gpu: the gradient densification statistics (gslic_rasterize_backward_adam_stats / _depth_adam_stats, gslic_gradient_stats_accumulate,
trainer.GradientStats).

The yardstick is never the code under test: the existing ten-gradient backward (gslic_rasterize_backward / _depth) on a bit-identical second
forward of the same parameters gives dL_dmean2D, which tests/gradstats_ref.py pushes through a numpy float32 transcription of the rule.  Every
comparison is on bits.  Row moves are held against plain torch indexing."""
import functools

import numpy as np
import pytest
import torch

import fused_check_io as fio
import gradstats_ref as gr
from gpu_helpers import gpu

pytestmark = pytest.mark.gpu


def _mods():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import rasterizer, trainer
    return trainer, rasterizer


def _cams(views=gr.VIEWS):
    from gaussian_lic_amd.camera import synthetic_camera
    return [synthetic_camera(gr.W, gr.H, v).to_device(gpu()) for v in views]


def _map(P, degree, order="insertion", **kw):
    trainer, _rz = _mods()
    m = trainer.GaussianModel(gr.scene(P, degree), gpu(), order=order, **kw)
    m.training_setup()
    return m


class Guarded:
    """The three accumulators as views into buffers with guard words on both sides, pre-filled with the sentinels."""
    G = 64

    def __init__(self, P):
        self.P = P
        s, n, r = gr.sentinels(P)
        self.bufs, self.views = [], []
        for init, dt in ((s, torch.float32), (n.view(np.int32), torch.int32), (r, torch.int32)):
            b = torch.full((P + 2 * self.G,), gr.GUARD, dtype=torch.int32, device=gpu())
            v = b[self.G:self.G + P].view(dt)
            v.copy_(torch.from_numpy(init.copy()).to(gpu()))
            self.bufs.append(b)
            self.views.append(v)

    def descriptor(self):
        return _mods()[1].grad_stats_descriptor(*self.views, self.P)

    def numpy(self):
        """(grad_sum bits, n_seen, max_radius) on the host, after checking the guard words."""
        torch.cuda.synchronize()
        for b in self.bufs:
            assert bool((b[:self.G] == gr.GUARD).all()) and bool((b[self.G + self.P:] == gr.GUARD).all()), "a guard word was overwritten"
        return [v.cpu().numpy().view(np.uint32).copy() for v in self.views]


def _u32(ref):   # (numpy reference arrays as uint32 words: not gpu_helpers.bits, which views one tensor)
    return [np.ascontiguousarray(a).view(np.uint32) for a in ref]


def _same(got, want):   # (lists of numpy arrays: not gpu_helpers.same_tensors, which compares tensors)
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def _dL(k, depth=False):
    from gaussian_lic_amd.synthetic import pixel_grad
    g = pixel_grad(gr.H, gr.W, seed=31 + k).to(gpu())
    return (g, (0.1 * pixel_grad(gr.H, gr.W, seed=77 + k)[0]).contiguous().to(gpu())) if depth else (g, None)


def _view_reference(m, cam, dL, dLd):
    """dL_dmean2D and radii of the ten-gradient backward on a forward of its own (CPU numpy)."""
    trainer, _rz = _mods()
    fwd = trainer._RawRaster(m, cam, torch.zeros(3, device=gpu()), depth=dLd is not None)
    with torch.no_grad():
        fwd.forward()
        g = fwd.backward(dL, dLd)
    return g[0].cpu().numpy(), fwd.state[2].cpu().numpy()


def _fused_view(m, cam, dL, dLd, stats):
    """The fused Adam backward with statistics on a second forward of the same parameters (updates the map)."""
    trainer, _rz = _mods()
    fwd = trainer._RawRaster(m, cam, torch.zeros(3, device=gpu()), depth=dLd is not None)
    with torch.no_grad():
        fwd.forward()
        fwd.backward(dL, dLd, adam=m.optimizer.fused_descriptor(), grad_stats=stats)
    m.optimizer.count_step()
    return fwd.state[2].cpu().numpy()


def _three_views(P, degree, depth):
    m = _map(P, degree)
    g = Guarded(P)
    ref = gr.sentinels(P)
    vis = []
    before = m.xyz.detach().clone()
    for k, cam in enumerate(_cams()):
        dL, dLd = _dL(k, depth)
        m2d, radii = _view_reference(m, cam, dL, dLd)
        gr.apply_rule(*ref, m2d, radii)
        radii2 = _fused_view(m, cam, dL, dLd, g.descriptor())
        assert np.array_equal(radii, radii2)                     # the second forward is the first
        vis.append(radii > 0)
        got = g.numpy()                                          # (guard words after every call)
    vis = np.stack(vis)
    print(f"[gradstats] P {P} degree {degree} depth {depth}: visible per view {vis.sum(1).tolist()} never visible {int((~vis.any(0)).sum())}")
    assert vis.any() and (~vis).any()                            # at least one visible and one invisible row, or the case proves nothing
    if P > 1:
        assert (~vis.any(0)).any() and vis.sum(1).max() > 1      # a row no view sees keeps its sentinels
    assert not torch.equal(before, m.xyz.detach())               # Adam did move the map between the views
    want = _u32(ref)
    assert _same(got, want), [int((a != b).sum()) for a, b in zip(got, want)]
    never = ~vis.any(0)
    assert (got[0][never] == np.float32(gr.SENT_SUM).view(np.uint32)).all() and (got[1][never] == gr.SENT_SEEN).all() and (got[2][never] == 7).all()


@pytest.mark.parametrize("degree", [3, 1])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 257, 4097])
def test_rule_over_three_views(P, degree):
    _three_views(P, degree, depth=False)


@pytest.mark.parametrize("degree", [3, 1])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 257, 4097])
def test_rule_on_the_depth_variant(P, degree):
    _three_views(P, degree, depth=True)


def test_stand_alone_kernel_equals_the_fused_route_and_keeps_to_its_rows():
    _trainer, rz = _mods()
    P = 257
    m = _map(P, 3)
    cam = _cams()[0]
    dL, _ = _dL(0)
    m2d, radii = _view_reference(m, cam, dL, None)
    fused, alone, part = Guarded(P), Guarded(P), Guarded(P)
    t_m2d, t_r = torch.from_numpy(m2d).to(gpu()), torch.from_numpy(radii).to(gpu())
    rz.gradient_stats_accumulate(t_m2d, t_r, *alone.views)
    rz.gradient_stats_accumulate(t_m2d, t_r, *part.views, rows=(64, P))
    _fused_view(m, cam, dL, None, fused.descriptor())
    ref, ref_part = gr.sentinels(P), gr.sentinels(P)
    gr.apply_rule(*ref, m2d, radii)
    gr.apply_rule(*ref_part, m2d, radii, rows=(64, P))
    a, f, p = alone.numpy(), fused.numpy(), part.numpy()
    assert (radii[:64] > 0).any() and (radii[64:] > 0).any()
    assert _same(a, f) and _same(a, _u32(ref)) and _same(p, _u32(ref_part))
    assert _same([x[:64] for x in p], _u32([x[:64] for x in gr.sentinels(P)])) and not _same(p, a)


@pytest.mark.parametrize("depth", [False, True])
def test_capacity_overflow_touches_nothing(depth):
    trainer, rz = _mods()
    P = 257
    m = _map(P, 3)
    cam = _cams()[0]
    dL, dLd = _dL(0, depth)
    sizing = trainer._RawRaster(m, cam, torch.zeros(3, device=gpu()), depth=depth)
    with torch.no_grad():
        sizing.forward()
    R, B = sizing.state[:2]
    g = Guarded(P)
    start = g.numpy()
    params = [p.detach().clone() for p in m.parameters()]
    for cap_R, fits in ((R // 3, False), (R + 4096, True)):
        bufs = rz.CapacityBuffers(P, gr.W, gr.H, cap_R, B + 64, gpu(), depth=depth)
        fwd = trainer._RawRaster(m, cam, torch.zeros(3, device=gpu()), depth=depth)
        with torch.no_grad():
            fwd.forward(bufs)
            fwd.backward(dL, dLd, adam=m.optimizer.fused_descriptor(), grad_stats=g.descriptor())
        now = g.numpy()
        _r, _b, bits, good = bufs.read_status()
        assert (bits != 0) == (not fits) and good == int(fits)
        assert _same(now, start) == (not fits)
        assert all(torch.equal(a, b.detach()) for a, b in zip(params, m.parameters())) == (not fits)


def _state(m):   # (the 18 row arrays on the device, as a list: not gpu_helpers.model_state, which reads the optimizer's state)
    torch.cuda.synchronize()
    return [t[:m.P].clone() for d in (m._buf, m._m, m._v) for t in (d[n] for n in m.NAMES)]


@pytest.mark.parametrize("order", ["insertion", "morton"])
def test_training_is_unchanged_by_the_statistics(order):
    trainer, _rz = _mods()
    from gaussian_lic_amd.synthetic import gt_image
    P = 4097
    cams = _cams()
    gts = [gt_image(gr.H, gr.W, seed=5 + k).to(gpu()) for k in range(3)]
    bg = torch.zeros(3, device=gpu())
    plain, with_st, plain_u, unfused = (_map(P, 3, order) for _ in range(4))
    st, st_u = trainer.GradientStats(with_st), trainer.GradientStats(unfused)
    for k in range(4):
        trainer.training_step_fused(plain, cams[k % 3], gts[k % 3], bg)
        trainer.training_step_fused(with_st, cams[k % 3], gts[k % 3], bg, grad_stats=st)
        trainer.training_step_fused(plain_u, cams[k % 3], gts[k % 3], bg, adam_in_backward=False)
        trainer.training_step_fused(unfused, cams[k % 3], gts[k % 3], bg, adam_in_backward=False, grad_stats=st_u)
    a, b, c, d = _state(plain), _state(with_st), _state(plain_u), _state(unfused)
    differ = lambda x, y: [i for i, (u, v) in enumerate(zip(x, y)) if not torch.equal(u, v)]
    print(f"[gradstats] {order}: arrays that differ fused {differ(a, b)} unfused {differ(c, d)} fused vs unfused {differ(a, c)}")
    assert differ(a, b) == [] and differ(c, d) == []
    assert 2 <= int(st.n_seen().max()) <= 4 and int(st.max_radius().max()) > 0 and bool((st.grad_sum() > 0).any())   # (view 0 is stepped twice)
    # the stand-alone route of the unfused step adds up to the same bits as the kernel's own accumulation
    for x, y in zip(st._arrays(), st_u._arrays()):
        assert torch.equal(x[0], y[0])


@pytest.mark.parametrize("order", ["insertion", "morton"])
@pytest.mark.parametrize("use_graph", [False, True])
def test_graphed_step_with_statistics(use_graph, order):
    trainer, _rz = _mods()
    from gaussian_lic_amd.synthetic import gt_image
    P = 4097
    cams = _cams()[:2]
    gts = [gt_image(gr.H, gr.W, seed=5 + k).to(gpu()) for k in range(2)]
    bg = torch.zeros(3, device=gpu())
    eager, plain, graphed = _map(P, 3, order), _map(P, 3, order), _map(P, 3, order)
    st_e, st_g = trainer.GradientStats(eager), trainer.GradientStats(graphed)
    st_g._maxr[:P] = 3                                       # what is there when the step is built stays (warm-up and capture are undone)
    st_e._maxr[:P] = 3
    gs_plain = trainer.GraphedStep(plain, cams[0], gts[0], bg, use_graph=use_graph)
    for k in range(4):
        gs_plain.step(cams[k % 2], gts[k % 2])
    assert gs_plain.check() == 0
    gs = trainer.GraphedStep(graphed, cams[0], gts[0], bg, use_graph=use_graph, grad_stats=st_g)
    for k in range(4):
        gs.step(cams[k % 2], gts[k % 2])
    assert gs.check() == 0
    for k in range(4):
        trainer.training_step_fused(eager, cams[k % 2], gts[k % 2], bg, grad_stats=st_e)
    a, b, c = _state(eager), _state(graphed), _state(plain)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and all(torch.equal(x, y) for x, y in zip(a, c))
    for x, y in zip(st_e._arrays(), st_g._arrays()):
        assert torch.equal(x[0], y[0])
    assert int(st_g.n_seen().max()) == 4                     # (six, had the two passes of the build not been undone)
    # a statistics object whose arrays were replaced since the step was built is refused like a stale layout
    st_g._alloc(graphed.capacity)
    with pytest.raises(RuntimeError, match="reallocated"):
        gs.step(cams[0], gts[0])


def _snap(st):
    torch.cuda.synchronize()
    P = st.model.P
    return [a[:P].cpu().clone() for a, _w in st._arrays()]


def test_other_paths_feed_the_same_statistics():
    """training_step (autograd, raw and operator renderer) and training_step_with_pose: one view each, equal to the rule on that view's gradient."""
    trainer, _rz = _mods()
    from gaussian_lic_amd.synthetic import gt_image
    P = 257
    cam = _cams()[1]
    gt = gt_image(gr.H, gr.W, seed=5).to(gpu())
    bg = torch.zeros(3, device=gpu())
    got = []
    for kind in ("fused", "autograd", "pose"):
        m = _map(P, 3)
        st = trainer.GradientStats(m)
        if kind == "fused":
            trainer.training_step_fused(m, cam, gt, bg, grad_stats=st)
        elif kind == "autograd":
            trainer.training_step(m, cam, gt, bg, one_node_loss=True, grad_stats=st)
        else:
            trainer.training_step_with_pose(m, cam, gt, bg, grad_stats=st)
        got.append(_snap(st))
    assert bool(got[0][1].any())
    assert all(torch.equal(x, y) for x, y in zip(got[0], got[2]))          # the same loss kernels, the same backward sums
    assert torch.equal(got[0][1], got[1][1]) and torch.equal(got[0][2], got[1][2])   # (autograd's loss differs in rounding: counts and radii only)
    # the operator renderer leaves the gradient in screenspace_points.grad
    m = _map(P, 3)
    st = trainer.GradientStats(m)
    trainer.training_step(m, cam, gt, bg, raw_render=False, grad_stats=st)
    s = _snap(st)
    assert torch.equal(s[1], got[0][1]) and torch.equal(s[2], got[0][2]) and bool((s[0] > 0).any())


def test_statistics_follow_the_rows():
    trainer, _rz = _mods()
    from gaussian_lic_amd.synthetic import gt_image, lidar_scene
    dev = gpu()
    P = 600
    cams = _cams()[:2]
    gts = [gt_image(gr.H, gr.W, seed=5 + k).to(dev) for k in range(2)]
    bg = torch.zeros(3, device=dev)
    a, d = _map(P, 3), _map(P, 3, "morton", resort_fraction=None)
    assert not torch.equal(d.tie_rank.long().cpu(), torch.arange(P))
    sa, sd = trainer.GradientStats(a), trainer.GradientStats(d)
    for k in range(2):
        trainer.training_step_fused(a, cams[k], gts[k], bg, grad_stats=sa)
        trainer.training_step_fused(d, cams[k], gts[k], bg, grad_stats=sd)
    order = d.original_order().cpu()
    assert all(torch.equal(x, y[order]) for x, y in zip(_snap(sa), _snap(sd))) and bool(_snap(sa)[1].any())   # the twins agree row for row
    # masks: torch reproduces them from the arrays
    thr = float(sd.mean_gradient()[sd.n_seen() > 0].median())
    grow = sd.grow_mask(thr)
    assert torch.equal(grow.bool(), (sd.n_seen() >= 1) & (sd.grad_sum() >= torch.tensor(np.float32(thr), device=dev) * sd.n_seen().float()))
    assert 0 < int(grow.sum()) < d.P
    rlim = int(sd.max_radius().float().median())
    big = sd.big_mask(rlim)
    assert torch.equal(big.bool(), sd.max_radius() > rlim) and 0 < int(big.sum()) < d.P
    # prune: old[kept]
    stale = trainer.GradientStats(d)
    stale.detach()
    old = _snap(sd)
    n, kept = d.prune(drop=big)
    assert n == int(big.sum()) and all(torch.equal(x, y[kept.cpu()]) for x, y in zip(_snap(sd), old))
    assert all(not bool(arr[d.P:].any()) for arr, _w in sd._arrays())
    with pytest.raises(RuntimeError, match="rows changed"):
        stale.grad_sum()
    # densify: new rows and split parents zero, everything else as it was
    old = _snap(sd)
    P0 = d.P
    grow = sd.grow_mask(thr)
    split_scale = float(torch.exp(d.scaling.detach()).max(1).values.median())
    over = (d.scaling.detach() > trainer.densify_threshold(split_scale)).any(1).cpu()      # the split rule, on the scaling as it is before the call
    k, n_split, parents = d.densify(grow, split_scale=split_scale)
    assert k > 0 and 0 < n_split < k and d.P == P0 + k
    now = _snap(sd)
    split = torch.zeros(P0, dtype=torch.bool)
    split[parents.cpu()] = True
    split &= over
    assert int(split.sum()) == n_split
    assert all(not bool(x[P0:].any()) for x in now)
    assert all(torch.equal(x[:P0][~split], y[~split]) and not bool(x[:P0][split].any()) for x, y in zip(now, old))
    assert int(split.sum()) > 0
    # extend: appended rows zero
    old = _snap(sd)
    P0 = d.P
    cam = cams[0]
    frame = lidar_scene(300, gr.W, gr.H, sh_degree=0, seed=77)
    col = (frame["features_dc"].reshape(-1, 3) * 0.28209479177387814 + 0.5).to(dev)
    Rcw = torch.from_numpy(cam.world_view_transform[:3, :3].T.copy())
    tcw = torch.from_numpy(cam.world_view_transform[3, :3].copy())
    k = d.extend(cam, frame["xyz"].to(dev), col, frame["xyz"][:, 2].contiguous().to(dev), Rcw, tcw, (float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy)))
    now = _snap(sd)
    assert k > 0 and all(torch.equal(x[:P0], y) and not bool(x[P0:].any()) for x, y in zip(now, old))
    # resort: the permutation
    trainer.training_step_fused(d, cams[1], gts[1], bg, grad_stats=sd)
    old = _snap(sd)
    perm = d.resort().cpu()
    assert not torch.equal(perm, torch.arange(d.P))
    assert all(torch.equal(x, y[perm]) for x, y in zip(_snap(sd), old))


def test_non_finite_gradient_rows():
    trainer, _rz = _mods()
    P = 257
    m = _map(P, 3)
    cam = _cams()[0]
    dL, _ = _dL(0)
    dL = dL.clone()
    dL[1, gr.H // 2, gr.W // 2] = float("nan")
    m2d, radii = _view_reference(m, cam, dL, None)
    ref = gr.sentinels(P)
    n = gr.apply_rule(*ref, m2d, radii)
    bad = (radii > 0) & ~np.isfinite(n)
    fine = (radii > 0) & np.isfinite(n)
    assert bad.any() and fine.any()
    g = Guarded(P)
    _fused_view(m, cam, dL, None, g.descriptor())
    got = g.numpy()
    assert _same(got, _u32(ref))
    assert (got[0][bad] == np.float32(gr.SENT_SUM).view(np.uint32)).all() and (got[1][bad] == gr.SENT_SEEN).all()
    assert (got[2][bad].view(np.int32) == np.maximum(radii[bad], 7)).all() and (got[1][fine] == gr.SENT_SEEN + 1).all()


@pytest.mark.parametrize("order", ["insertion", "morton"])
def test_fused_gradient_stats_cpp_host(tmp_path, order):
    """gslic::GradientStats behind gslic::FusedStep::set_gradient_stats issues the calls of the Python host: through steps, a densify() driven by
    grow_mask, a prune() driven by big_mask and a resort(), with steps in between, the three statistics arrays and all 19 row arrays (6 parameters,
    12 moments, the tie rank) are bit-identical to the Python model's, on both row orders."""
    trainer, _rz = _mods()
    from gaussian_lic_amd.synthetic import gt_image
    exe = fio.build("fused_gradient_stats")
    P, iters, seed = 600, 2, 11
    m = _map(P, 3, order, resort_fraction=None)
    cam = _cams()[1]
    gt = gt_image(gr.H, gr.W, seed=5).to(gpu())
    bg = torch.zeros(3, device=gpu())
    d = str(tmp_path)
    fio.write_inputs(d, m, cam, gt=gt, tie_rank=m.tie_rank)
    st = trainer.GradientStats(m)

    def steps():
        for _ in range(iters):
            trainer.training_step_fused(m, cam, gt, bg, grad_stats=st)
    steps()
    grad_above = float(np.float32(st.mean_gradient()[st.n_seen() > 0].median().item()))
    split_scale = float(torch.exp(m.scaling.detach().double()).max(1).values.median())
    k, n_split, _parents = m.densify(st.grow_mask(grad_above), split_scale, seed=seed)
    assert 0 < n_split < k < P
    steps()
    rlim = int(st.max_radius()[st.n_seen() > 0].float().median())
    n, _kept = m.prune(drop=st.big_mask(rlim))
    assert 0 < n < m.P
    steps()
    perm = m.to_morton_order(resort_fraction=None) if order == "insertion" else m.resort()
    assert not torch.equal(perm.cpu(), torch.arange(m.P))
    steps()
    r = fio.run(exe, d, str(P), str(gr.W), str(gr.H), "3", str(iters), repr(grad_above), str(rlim), repr(split_scale), str(seed))
    assert f"densify added {k} splits {n_split} pruned {n} size {m.P}" in r.stdout, r.stdout
    torch.cuda.synchronize()
    rd = functools.partial(fio.read, d)
    bits = lambda t: t.detach().contiguous().view(torch.int32).cpu().reshape(-1)
    Pn = m.P
    for name, f in (("xyz", "xyz"), ("features_dc", "dc"), ("features_rest", "rest"), ("opacity", "opacity"), ("scaling", "scaling"), ("rotation", "rotation")):
        for pre, src in (("", m._buf), ("m_", m._m), ("v_", m._v)):
            assert torch.equal(rd(pre + f + ".f32", np.int32), bits(src[name][:Pn])), pre + f
    assert torch.equal(rd("tie.i32", np.int32), m.tie_rank.cpu())
    assert torch.equal(rd("grad_sum.f32", np.int32), bits(st.grad_sum())) and bool((st.grad_sum() > 0).any())
    assert torch.equal(rd("n_seen.i32", np.int32), st._seen_n[:Pn].cpu()) and int(st.n_seen().max()) == 4 * iters
    assert torch.equal(rd("max_radius.i32", np.int32), st.max_radius().cpu())
