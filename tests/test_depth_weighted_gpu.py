"""-m gpu: the weighted / Huber depth loss (gslic_depth_loss_weighted_forward_backward) — the kernels against the float32 restatement of the
header's rule (tests/depth_weight_ref.py: the gradient bit for bit, the sums within the bound of their summands), against today's unweighted entry
point and under a graph; then depth_weight= / depth_huber= through training_step_fused, pose_gradient, training_step_with_pose, GraphedStep and
the C++ host's gslic::FusedStep."""
import functools

import numpy as np
import pytest
import torch

import depth_weight_ref as ref
import fused_check_io as fio
from conftest import make_scene
from gpu_helpers import assert_same_state, bits, gpu, guarded, guards_intact, model_state, training_model

pytestmark = pytest.mark.gpu

F = np.float32
GUARD_BITS = 0x7FC0FFEE   # a NaN pattern no kernel produces (the outputs are floats)
# 2048-pixel workgroups, eight pixels per thread, 256 partials per pass of the second kernel's loop: one pixel; one partial workgroup (1961);
# exactly one; the last workgroup one pixel short (4095); three and a tail; 264 workgroups (more than one partial per thread)
SHAPES = [(1, 1), (37, 53), (64, 32), (45, 91), (70, 90), (600, 900)]
DELTAS = [0.0, 0.25, 3.0]
LAM = 0.5
LAMBDA_D = 0.5


def _nan_guarded(n):
    buf, words = guarded(n, sentinel=GUARD_BITS)
    return buf, words.view(torch.float32)


def _weighted(depth, gt, weight, delta, lam=LAM):
    """The entry point on guarded buffers of its own: (dL_ddepth [H,W], terms [2], partials) as host numpy — asserts that the guard words survive."""
    from gaussian_lic_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    H, W = depth.shape
    n_part = int(L.gslic_depth_loss_weighted_partials_count(H, W))
    gb_dL, dL = _nan_guarded(H * W)
    gb_p, partials = _nan_guarded(n_part)
    gb_t, terms = _nan_guarded(2)
    _lib.check(L.gslic_depth_loss_weighted_forward_backward(H, W, float(lam), float(delta), p(depth), p(gt), p(weight), p(partials), p(terms), p(dL),
                                                            _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    for buf, n, name in ((gb_dL, H * W, "dL_ddepth"), (gb_p, n_part, "partials"), (gb_t, 2, "terms")):
        assert guards_intact(buf, n, sentinel=GUARD_BITS), name + " guard"
    return dL.view(H, W).cpu().numpy().copy(), terms.cpu().numpy().copy(), partials.cpu().numpy().copy()


def _unweighted(depth, gt, lam=LAM):
    """Today's entry point, gslic_depth_l1_loss_forward_backward: (dL_ddepth, term)."""
    from gaussian_lic_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    H, W = depth.shape
    dL, term = torch.empty_like(depth), torch.empty(1, device=gpu())
    partials = torch.empty(int(L.gslic_depth_l1_loss_partials_count(H, W)), device=gpu())
    _lib.check(L.gslic_depth_l1_loss_forward_backward(H, W, float(lam), p(depth), p(gt), p(partials), p(term), p(dL), _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    return dL.cpu().numpy(), term.cpu().numpy()


def _tree(x):
    """The kernel's order over per-workgroup partials, in float32: thread t of 256 adds b = t, t + 256, ...; a xor-shuffle tree (32 ... 1) per 64
    lanes; (r0 + r1) + (r2 + r3)."""
    x = np.asarray(x, F)
    v = np.zeros(256, F)
    for t in range(256):
        for b in range(t, len(x), 256):
            v[t] = F(v[t] + x[b])
    lane = np.arange(256)
    for d in (32, 16, 8, 4, 2, 1):
        v = (v + v[(lane & ~63) | ((lane & 63) ^ d)]).astype(F)
    return F(F(v[0] + v[64]) + F(v[128] + v[192]))


def _exact_residuals(delta):
    """(gt, depth) pairs whose float32 difference depth - gt is exactly +-x for x in {0, delta, the float below delta, the float above delta} (delta
    = 0: 0 and the smallest normal steps around 0.25): depth = gt +- x for the first gt of a short list for which the subtraction gives x back."""
    d = F(delta if delta > 0 else 0.25)
    pairs, found = [], set()
    for x in (F(0), d, np.nextafter(d, F(0)), np.nextafter(d, F(np.inf))):
        for s in (F(1), F(-1)):
            for g in (F(1.0), F(0.5), F(0.125), F(2.0 ** -10), F(4.0)):
                dep = F(g + s * x)
                if F(dep - g) == F(s * x):
                    pairs.append((g, dep))
                    found.add((float(x), float(s)))
                    break
    assert {(float(x), 1.0) for x in (F(0), d)} <= found and {(float(x), -1.0) for x in (F(0), d)} <= found
    assert all(any((float(x), s) in found for s in (1.0, -1.0)) for x in (np.nextafter(d, F(0)), np.nextafter(d, F(np.inf))))
    return pairs


@functools.lru_cache(maxsize=None)
def _inputs(H, W, delta):
    """Host float32 (depth, gt, weight) of a shape: gt with zeros, a NaN and a negative value; weights with 0, NaN, a negative value, +inf, values
    above 1 and denormals; residuals exactly 0, +-delta and one float inside and outside of it (as many of the special pixels as the image holds)."""
    rng = np.random.default_rng(1000 * H + W + int(100 * delta))
    N = H * W
    gt = (rng.random(N) * 10.0 + 0.01).astype(F)
    gt[rng.random(N) < 0.45] = 0.0
    depth = (gt + (rng.random(N).astype(F) - F(0.5)) * F(8.0 if delta > 1 else 2.0)).astype(F)
    weight = (rng.random(N) * 3.0).astype(F)
    slots = iter(rng.permutation(N))
    if N == 1:
        gt[0], depth[0], weight[0] = 2.0, 2.5, 1.75
    else:
        for g, dep in _exact_residuals(delta):
            i = next(slots, None)
            if i is None:
                break
            gt[i], depth[i], weight[i] = g, dep, F(0.75 + 2.0 * rng.random())
        for g in (np.nan, -3.0, 0.0):
            i = next(slots, None)
            if i is not None:
                gt[i] = g
        for w in (0.0, np.nan, -2.0, np.inf, 1e-40, 3e-39, 7.5):
            i = next(slots, None)
            if i is not None:
                weight[i] = w
                gt[i] = gt[i] if gt[i] > 0 else F(3.0)     # a measured pixel, so that the weight decides
    return depth.reshape(H, W), gt.reshape(H, W), weight.reshape(H, W)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu())


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, F).view(np.int32), np.asarray(b, F).view(np.int32))


# ---------------------------------------------------------------------------------------------------- 1, 2. gradient on bits, sums within their bound
@pytest.mark.parametrize("delta", DELTAS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_kernel_is_the_rule(H, W, delta):
    depth, gt, weight = _inputs(H, W, delta)
    for w in (weight, None):
        dL, terms, partials = _weighted(_dev(depth), _dev(gt), None if w is None else _dev(w), delta)
        S = terms[1]
        # 1. the gradient from the kernel's own S, bit for bit
        want = ref.gradient(depth, gt, w, delta, LAM, S)
        assert _same_bits(dL, want), (int((dL.view(np.int32) != want.view(np.int32)).sum()), "pixels differ")
        assert not np.isnan(dL).any()
        # 2. non-negative summands: any order is within n 2^-24 of the float64 sum
        S64, T64, n = ref.sums64(depth, gt, w, delta)
        nblk = -(-H * W // 2048)
        T = _tree(partials[0:2 * nblk:2])
        assert _tree(partials[1:2 * nblk:2]).view(np.int32) == S.view(np.int32)
        print(f"{H}x{W} delta {delta} weight {w is not None}: n {n} S {S!r} S64 {S64!r} T {T!r} T64 {T64!r}")
        assert abs(float(S) - S64) <= n * 2.0 ** -24 * S64
        assert abs(float(T) - T64) <= n * 2.0 ** -24 * T64
        assert terms[0].view(np.int32) == (F(T) / F(S) if S > 0 else F(0)).view(np.int32)
        if H * W > 1:
            assert n > 0 and S > 0 and terms[0] > 0


# ---------------------------------------------------------------------------------------------------- 3. against today's entry point
@pytest.mark.parametrize("H,W", SHAPES)
def test_unit_weight_and_no_threshold_is_todays_entry_point_bit_for_bit(H, W):
    depth, gt, _w = _inputs(H, W, 0.0)
    d, g = _dev(depth), _dev(gt)
    dL0, term0 = _unweighted(d, g)
    for w in (None, torch.ones(H, W, device=gpu())):
        dL, terms, _p = _weighted(d, g, w, 0.0)
        assert _same_bits(dL, dL0) and _same_bits(terms[0], term0[0])
        assert float(terms[1]) == float(((gt > 0)).sum())


# ---------------------------------------------------------------------------------------------------- 4. a zero weight is no measurement
@pytest.mark.parametrize("delta", DELTAS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_zero_weight_is_an_unmeasured_pixel(H, W, delta):
    depth, gt, weight = _inputs(H, W, delta)
    with np.errstate(invalid="ignore"):
        keep = (weight > 1.0).astype(F)                       # a 0/1 weight (NaN: 0)
        masked_gt = (gt * keep).astype(F)
    d = _dev(depth)
    dL_a, terms_a, _p = _weighted(d, _dev(gt), _dev(keep), delta)
    dL_b, terms_b, _p = _weighted(d, _dev(masked_gt), None, delta)
    assert _same_bits(dL_a, dL_b) and _same_bits(terms_a, terms_b)
    # S = 0: all weights zero (or read as zero), or no measurement — terms 0, the gradient all (positive) zeros, also where depth is not finite
    d_bad = depth.copy(); d_bad.flat[0] = np.nan; d_bad.flat[-1] = np.inf
    for g, w in ((gt, np.zeros_like(gt)), (gt, np.full_like(gt, np.nan)), (np.zeros_like(gt), weight), (np.zeros_like(gt), None)):
        dL, terms, _p = _weighted(_dev(d_bad), _dev(g), None if w is None else _dev(w), delta)
        assert not dL.view(np.int32).any() and not terms.view(np.int32).any()


# ---------------------------------------------------------------------------------------------------- 5. repeatable, and the same under a graph
def test_two_calls_and_a_graph_replay_give_the_same_bits():
    from gaussian_lic_amd import _lib
    H, W, delta = 70, 90, 0.25
    depth, gt, weight = _inputs(H, W, delta)
    d, g, w = _dev(depth), _dev(gt), _dev(weight)
    dL1, terms1, _p = _weighted(d, g, w, delta)
    dL2, terms2, _p = _weighted(d, g, w, delta)
    assert _same_bits(dL1, dL2) and _same_bits(terms1, terms2)
    L, p = _lib.lib(), _lib.ptr
    dL = torch.full((H, W), float("nan"), device=gpu())
    terms = torch.full((2,), float("nan"), device=gpu())
    partials = torch.empty(int(L.gslic_depth_loss_weighted_partials_count(H, W)), device=gpu())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # (no allocation, no synchronisation, nothing read back: the call only enqueues its two launches)
        _lib.check(L.gslic_depth_loss_weighted_forward_backward(H, W, LAM, delta, p(d), p(g), p(w), p(partials), p(terms), p(dL), _lib.current_stream_ptr()))
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(dL.cpu().numpy(), dL1) and _same_bits(terms.cpu().numpy(), terms1)


# ---------------------------------------------------------------------------------------------------- FusedLoss
def test_fused_loss_keeps_terms3_and_exposes_the_weight_sum():
    from gaussian_lic_amd import loss
    H, W, delta = 70, 90, 0.25
    depth, gt, weight = _inputs(H, W, delta)
    d, g, w = _dev(depth), _dev(gt), _dev(weight)
    fl = loss.FusedLoss(0.2)
    assert fl.depth_weight_sum is None
    dL, term = fl.depth_forward_backward(d, g, LAM, weight=w, huber=delta)
    dL_k, terms_k, _p = _weighted(d, g, w, delta)
    assert _same_bits(dL.cpu().numpy(), dL_k)
    assert fl.terms3.numel() == 3 and _same_bits(fl.terms3[2:3].cpu().numpy(), terms_k[0:1]) and term.data_ptr() == fl.terms3[2:3].data_ptr()
    assert _same_bits(fl.depth_weight_sum.cpu().numpy(), terms_k[1:2])
    # the autograd statement of the same rule, within the bound of its sums (two sums of n non-negative float32 terms and a quotient each)
    n = ref.sums64(depth, gt, weight, delta)[2]
    assert abs(float(loss.depth_l1(d, g, w, delta)) - float(term)) <= (4 * n + 4) * 2.0 ** -24 * float(term)
    with pytest.raises(ValueError, match="float32"):
        fl.depth_forward_backward(d, g, LAM, weight=w.double())
    with pytest.raises(ValueError, match="float32"):
        fl.depth_forward_backward(d, g, LAM, weight=w[:-1])


# ---------------------------------------------------------------------------------------------------- the steps
def _setup(P=5000, W=160, H=120, deg=3, seed=5):
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd.synthetic import gt_image
    raw, sc, camd, cam = make_scene("random", P, W, H, deg, seed)
    cam.to_device(gpu())
    gtd = cam.project_depth(raw["xyz"][::5].float() * 1.1).to(gpu())
    assert int((gtd > 0).sum()) > 100
    return raw, cam, gt_image(H, W, seed=seed).to(gpu()), gtd, torch.zeros(3, device=gpu())


# 6. fused against autograd: the comparison and the bars of tests/test_depth_fused_gpu.py::test_fused_depth_step_matches_autograd_depth_step
@pytest.mark.parametrize("huber", [0.0, 0.3])
def test_fused_weighted_depth_step_matches_the_autograd_step(huber):
    from gaussian_lic_amd import trainer
    raw, cam, gt, gtd, bg = _setup(P=30000, W=320, H=240, seed=61)
    w = trainer.range_weight(gtd, 0.05, 0.02)
    assert w.device == gtd.device and float(w.max()) <= 1.0 and int((w > 0).sum()) == int((gtd > 0).sum())
    a, b = training_model(raw), training_model(raw)
    kw = dict(gt_depth=gtd, lambda_depth=LAMBDA_D, depth_weight=w, depth_huber=huber)
    loss, vis = trainer.training_step(a, cam, gt, bg, do_step=False, raw_render=False, **kw)
    g_ref = [p.grad.clone() for p in a.parameters()]
    captured = {}
    b.optimizer.step = lambda grads=None: captured.setdefault("g", [g.clone() for g in grads])
    terms, vis2 = trainer.training_step_fused(b, cam, gt, bg, adam_in_backward=False, **kw)
    assert torch.equal(vis, vis2)
    fl = trainer._default_fused_loss()
    assert terms.numel() == 3 and float(terms[2]) > 0
    print(f"huber {huber}: loss fused {float(fl.value(terms, LAMBDA_D))!r} autograd {float(loss)!r}")
    assert abs(float(fl.value(terms, LAMBDA_D)) - float(loss)) < 2e-6
    for name, gr, g in zip(a.NAMES, g_ref, captured["g"]):
        scale = float(gr.abs().max())
        if name == "rotation":
            scale = max(scale, 1e-6)
        err = float((g.reshape(gr.shape) - gr).abs().max()) / max(scale, 1e-30)
        print(f"  {name}: {err:.3e}")
        assert err < 5e-5, (name, err)
    # the weight and the threshold change the step
    c = training_model(raw)
    c.optimizer.step = lambda grads=None: captured.setdefault("plain", [g.clone() for g in grads])
    trainer.training_step_fused(c, cam, gt, bg, adam_in_backward=False, gt_depth=gtd, lambda_depth=LAMBDA_D)
    assert not torch.equal(captured["plain"][0], captured["g"][0])


# 7. a 0/1 depth_weight is gt_depth * mask, on every path, without a tolerance
@pytest.mark.parametrize("huber", [0.0, 0.3])
def test_mask_as_depth_weight_is_the_masked_target_bit_for_bit(huber):
    from gaussian_lic_amd import trainer
    raw, cam, gt, gtd, bg = _setup()
    H, W = gtd.shape
    yy, xx = torch.meshgrid(torch.arange(H, device=gpu()), torch.arange(W, device=gpu()), indexing="ij")
    mask = (((yy // 8) + (xx // 8)) % 3 != 0).float()
    assert 0 < int(((gtd > 0) & (mask > 0)).sum()) < int((gtd > 0).sum())
    kw_w = dict(gt_depth=gtd, lambda_depth=LAMBDA_D, depth_weight=mask, depth_huber=huber)
    kw_m = dict(gt_depth=gtd * mask, lambda_depth=LAMBDA_D, depth_huber=huber)
    for adam_in_backward in (True, False):
        a, b = training_model(raw), training_model(raw)
        ta, va = trainer.training_step_fused(a, cam, gt, bg, adam_in_backward=adam_in_backward, **kw_w)
        tb, vb = trainer.training_step_fused(b, cam, gt, bg, adam_in_backward=adam_in_backward, **kw_m)
        assert torch.equal(bits(ta), bits(tb)) and torch.equal(va, vb) and ta.numel() == 3
        assert_same_state(model_state(a), model_state(b))
    m = training_model(raw)
    ga, t1 = trainer.pose_gradient(m, cam, gt, bg, **kw_w)
    t1 = t1.clone()
    gb, t2 = trainer.pose_gradient(m, cam, gt, bg, **kw_m)
    assert np.array_equal(np.asarray(ga), np.asarray(gb)) and np.abs(np.asarray(ga)).max() > 0 and torch.equal(bits(t1), bits(t2))
    g_plain, _t = trainer.pose_gradient(m, cam, gt, bg, gt_depth=gtd, lambda_depth=LAMBDA_D)
    assert not np.array_equal(np.asarray(ga), np.asarray(g_plain))
    a, b = training_model(raw), training_model(raw)
    ta, va, ga = trainer.training_step_with_pose(a, cam, gt, bg, pose_lr=0.0, **kw_w)
    tb, vb, gb = trainer.training_step_with_pose(b, cam, gt, bg, pose_lr=0.0, **kw_m)
    assert torch.equal(bits(ta), bits(tb)) and torch.equal(va, vb) and np.array_equal(np.asarray(ga), np.asarray(gb))
    assert_same_state(model_state(a), model_state(b))


# 8. GraphedStep
@pytest.mark.parametrize("use_graph", [False, True])
def test_graphed_step_with_a_depth_weight_equals_eager_steps(use_graph):
    from gaussian_lic_amd import trainer
    raw, cam, gt, gtd, bg = _setup(P=20000, W=320, H=240, seed=91)
    ws = [trainer.range_weight(gtd, 0.05, 0.02), trainer.range_weight(gtd, 0.5, 0.3) * 4.0, None]   # replaced at the second step, kept at the third
    huber = 0.3
    a, b = training_model(raw), training_model(raw)
    gs = trainer.GraphedStep(a, cam, gt, bg, use_graph=use_graph, gt_depth=gtd, lambda_depth=LAMBDA_D, depth_weight=ws[0], depth_huber=huber)
    loaded = None
    for k in range(3):
        loaded = ws[k] if ws[k] is not None else loaded
        t_g = gs.step(cam, gt, gtd, depth_weight=ws[k]).clone()
        t_e = trainer.training_step_fused(b, cam, gt, bg, gt_depth=gtd, lambda_depth=LAMBDA_D, depth_weight=loaded, depth_huber=huber)[0].clone()
        assert t_g.numel() == 3 and torch.equal(bits(t_g), bits(t_e)), k
    assert gs.check() == 0
    assert_same_state(model_state(a), model_state(b))


def test_graphed_step_depth_weight_mismatches_raise():
    from gaussian_lic_amd import trainer
    raw, cam, gt, gtd, bg = _setup()
    w = trainer.range_weight(gtd, 0.05, 0.02)
    m = training_model(raw)
    before = model_state(m)
    plain = trainer.GraphedStep(m, cam, gt, bg, gt_depth=gtd, lambda_depth=LAMBDA_D)
    with pytest.raises(ValueError, match="built without"):
        plain.step(cam, gt, gtd, depth_weight=w)
    weighted = trainer.GraphedStep(m, cam, gt, bg, gt_depth=gtd, lambda_depth=LAMBDA_D, depth_weight=w)
    with pytest.raises(ValueError, match="shape"):
        weighted.step(cam, gt, gtd, depth_weight=w[:-1])
    with pytest.raises(ValueError, match="without gt_depth"):
        trainer.GraphedStep(m, cam, gt, bg, depth_weight=w)
    assert_same_state(before, model_state(m))


# 9. the defaults are today's step, launch for launch
def _launches(fn):
    from gaussian_lic_amd import _lib
    _lib.profile_enable(True)
    try:
        _lib.profile_reset()
        out = fn()
        counts = {k: n for k, (_ms, n) in _lib.profile_collect().items()}
    finally:
        _lib.profile_enable(False)
    return counts, out


def test_defaults_issue_todays_launches():
    from gaussian_lic_amd import trainer
    raw, cam, gt, gtd, bg = _setup()
    base = dict(gt_depth=gtd, lambda_depth=LAMBDA_D)
    off = dict(base, depth_weight=None, depth_huber=0)
    for adam_in_backward in (True, False):
        a, b = training_model(raw), training_model(raw)
        trainer.training_step_fused(a, cam, gt, bg, **base); trainer.training_step_fused(b, cam, gt, bg, **base)   # (first-step allocations out of the way)
        a, b = training_model(raw), training_model(raw)
        n_a, _o = _launches(lambda: trainer.training_step_fused(a, cam, gt, bg, adam_in_backward=adam_in_backward, **base))
        n_b, _o = _launches(lambda: trainer.training_step_fused(b, cam, gt, bg, adam_in_backward=adam_in_backward, **off))
        assert n_a == n_b and n_a["depth_loss"] == 2, (n_a, n_b)
        assert_same_state(model_state(a), model_state(b))
    m = training_model(raw)
    n_a, (g_a, _t) = _launches(lambda: trainer.pose_gradient(m, cam, gt, bg, **base))
    n_b, (g_b, _t) = _launches(lambda: trainer.pose_gradient(m, cam, gt, bg, **off))
    assert n_a == n_b and np.array_equal(np.asarray(g_a), np.asarray(g_b))
    a, b = training_model(raw), training_model(raw)
    n_a, _o = _launches(lambda: trainer.training_step_with_pose(a, cam, gt, bg, **base))
    n_b, _o = _launches(lambda: trainer.training_step_with_pose(b, cam, gt, bg, **off))
    assert n_a == n_b
    assert_same_state(model_state(a), model_state(b))
    a, b = training_model(raw), training_model(raw)
    ga, gb = trainer.GraphedStep(a, cam, gt, bg, **base), trainer.GraphedStep(b, cam, gt, bg, **off)
    n_a, _o = _launches(lambda: ga.step())
    n_b, _o = _launches(lambda: gb.step())
    assert n_a == n_b and ga.check() == 0 and gb.check() == 0
    assert_same_state(model_state(a), model_state(b))
    # the weighted step: the same number of launches under the same profiler id, the new kernels
    c = training_model(raw)
    n_c, _o = _launches(lambda: trainer.training_step_fused(c, cam, gt, bg, depth_huber=0.3, **base))
    assert n_c["depth_loss"] == 2 and not torch.equal(model_state(c)["xyz"], model_state(a)["xyz"])


# 10. the C++ host
@pytest.mark.parametrize("huber,use_weight", [(0.3, True), (0.0, True), (0.3, False)])
def test_fused_depth_weighted_cpp_host(tmp_path, huber, use_weight):
    """gslic::FusedStep::step / pose_gradient with depth_weight / depth_huber issue the C-ABI calls of training_step_fused / pose_gradient: terms, the
    weight sum, parameters and moments after three steps are bit-identical to the Python host's.  The driver is built when missing."""
    from gaussian_lic_amd import loss, trainer
    exe = fio.build("fused_depth_weighted")
    P, W, H, deg, iters = 5000, 160, 120, 3, 3
    raw, cam, gt, gtd, bg = _setup(P, W, H, deg, 44)
    w = trainer.range_weight(gtd, 0.05, 0.02) * 2.5 if use_weight else None
    d = str(tmp_path)
    extra = dict(depth_weight=w) if use_weight else {}
    fio.write_inputs(d, raw, cam, gt=gt, gt_depth=gtd, **extra)
    r = fio.run(exe, d, str(P), str(W), str(H), str(deg), str(iters), repr(LAMBDA_D), repr(huber), str(int(use_weight)))
    model = training_model(raw)
    fl = loss.FusedLoss(0.2)
    kw = dict(gt_depth=gtd, lambda_depth=LAMBDA_D, depth_weight=w, depth_huber=huber)
    g, _t = trainer.pose_gradient(model, cam, gt, bg, fused_loss=fl, **kw)
    for _ in range(iters):
        terms, _vis = trainer.training_step_fused(model, cam, gt, bg, fused_loss=fl, **kw)
    rd = lambda name, n: fio.read(d, name + ".f32", np.int32)
    assert torch.equal(rd("terms", 3), bits(terms.cpu()))
    assert torch.equal(rd("depth_weight_sum", 1), bits(fl.depth_weight_sum.cpu()))
    rows = fio.read_rows(d, 15)
    state = model_state(model)
    for name, key in (("xyz", "xyz"), ("scaling", "scaling"), ("rotation", "rotation"), ("opacity", "opacity"), ("features_dc", "dc"), ("features_rest", "rest")):
        assert torch.equal(rows[key], bits(state[name]).reshape(-1)), name
        assert torch.equal(rows["m_" + key], bits(state[name + ".m"]).reshape(-1)) and torch.equal(rows["v_" + key], bits(state[name + ".v"]).reshape(-1)), name
    pose = [l for l in r.stdout.splitlines() if l.startswith("pose ")]
    assert len(pose) == 1
    # (the se(3) chain runs on the host in both: the bar of tests/test_shim_gpu.py::test_fused_cpp_host_pose_gradient, 1e-5 of max-abs)
    got, want = np.array([float(x) for x in pose[0].split()[1:]]), np.asarray(g, np.float64)
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()


# 11. refusals
def test_depth_weight_needs_a_depth_target_and_one_gpu(monkeypatch):
    from gaussian_lic_amd import trainer
    raw, cam, gt, gtd, bg = _setup()
    w = trainer.range_weight(gtd, 0.05, 0.02)
    m = training_model(raw)
    before = model_state(m)
    for fn in (trainer.training_step, trainer.training_step_fused, trainer.pose_gradient, trainer.training_step_with_pose):
        with pytest.raises(ValueError, match="without gt_depth"):
            fn(m, cam, gt, bg, depth_weight=w)
    # the N > 1 path, as a process group of one rank takes it under GSLIC_FORCE_DIST=1: the error gt_depth raises there
    monkeypatch.setenv("GSLIC_FORCE_DIST", "1")
    torch.distributed.init_process_group("gloo", store=torch.distributed.HashStore(), rank=0, world_size=1)
    try:
        assert trainer._dist_on()
        with pytest.raises(NotImplementedError, match="N > 1"):
            trainer.training_step_fused(m, cam, gt, bg, gt_depth=gtd, lambda_depth=LAMBDA_D)
        with pytest.raises(NotImplementedError, match="N > 1"):
            trainer.training_step_fused(m, cam, gt, bg, gt_depth=gtd, lambda_depth=LAMBDA_D, depth_weight=w)
        with pytest.raises(NotImplementedError, match="N > 1"):
            trainer.training_step_fused(m, cam, gt, bg, depth_weight=w)
    finally:
        torch.distributed.destroy_process_group()
    assert not trainer._dist_on()
    assert_same_state(before, model_state(m))


# evaluation
def test_evaluate_visual_quality_adds_depth_metrics_when_asked():
    from gaussian_lic_amd import loss, trainer
    from gaussian_lic_amd.rasterizer import render
    raw, cam, gt, gtd, bg = _setup()
    m = training_model(raw)
    w = trainer.range_weight(gtd, 0.05, 0.02)
    plain = loss.evaluate_visual_quality(m, [cam, cam], [gt, gt], bg)
    assert len(plain) == 2
    out = loss.evaluate_visual_quality(m, [cam, cam], [gt, gt], bg, gt_depths=[gtd, None], depth_weights=[w, None])
    assert len(out) == 3 and torch.equal(out[0], plain[0]) and torch.equal(out[1], plain[1])
    with torch.no_grad():
        depth = render(cam, m, bg, return_depth=True)[5]
    want = loss.depth_metrics(depth, gtd, w)
    assert set(out[2]) == {"mae", "rmse", "abs_rel", "delta1", "n"}
    for k, v in want.items():
        assert float(out[2][k]) == float(v) and np.isfinite(float(v)), k
    assert float(want["n"]) > 0 and 0.0 <= float(want["delta1"]) <= 1.0
