"""CPU-only: the weighted / Huber depth loss without a device — the two exports and their refusals (reported before any device work), the torch
helpers trainer.range_weight and loss.depth_metrics on hand-computed values, and loss.depth_l1(weight, huber) on CPU tensors against the float64
restatement (tests/depth_weight_ref.py) and torch's smooth_l1_loss."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import depth_weight_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG = -1


def _lib():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------------- the two symbols
def test_symbols_are_exported_and_declared():
    _l = _lib()
    L = _l.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gslic_hip.h")).read(), flags=re.S)
    for sym in ("gslic_depth_loss_weighted_forward_backward", "gslic_depth_loss_weighted_partials_count"):
        assert hasattr(ctypes.CDLL(_l.LIB_PATH), sym), sym
        assert sym in _l.EXPORTS and re.search(r"\b" + sym + r"\s*\(", header), sym
    assert L.gslic_abi_version() == 8
    # the scratch covers one {T, S} pair per workgroup of 2048 pixels
    count = L.gslic_depth_loss_weighted_partials_count
    assert count(1, 1) >= 2 and count(64, 32) >= 2 and count(45, 91) >= 4 and count(600, 900) >= 2 * 264 and count(1080, 1920) >= 2 * 1013
    assert count(0, 5) > 0 and count(5, -1) > 0


# ---------------------------------------------------------------------------------------------------- refusals, before any device work
def _call(L, H=4, W=6, lam=0.5, delta=0.0, depth=0x10000, gt=0x20000, weight=0x30000, partials=0x40000, terms=0x50000, dL=0x60000):
    """The entry point on made-up addresses: every case here is refused before anything is dereferenced or launched."""
    vp = lambda a: None if a is None else ctypes.c_void_p(a)
    rc = L.gslic_depth_loss_weighted_forward_backward(H, W, lam, delta, vp(depth), vp(gt), vp(weight), vp(partials), vp(terms), vp(dL), None)
    return rc, L.gslic_last_error().decode()


@pytest.mark.parametrize("kw,name", [
    (dict(H=0), "H"), (dict(H=-3), "H"), (dict(W=0), "W"), (dict(W=-1), "W"),
    (dict(depth=None), "depth"), (dict(gt=None), "gt_depth"), (dict(partials=None), "partials"), (dict(terms=None), "terms"), (dict(dL=None), "dL_ddepth"),
    (dict(delta=-0.25), "delta"), (dict(delta=float("nan")), "delta"), (dict(delta=float("inf")), "delta"),
    (dict(lam=float("nan")), "lambda_depth"),
    (dict(dL=0x10000), "dL_ddepth"), (dict(dL=0x20000 + 4 * 23), "dL_ddepth"), (dict(dL=0x30000 - 4), "dL_ddepth"),
    (dict(terms=0x10000 + 8), "terms"), (dict(terms=0x20000 - 4), "terms"), (dict(terms=0x30000 + 4 * 23), "terms"),
])
def test_refusals_name_the_argument(kw, name):
    rc, msg = _call(_lib().lib(), **kw)
    assert rc == ERR_INVALID_ARG, (kw, rc)
    assert re.search(r"\b" + name + r"\b", msg), (kw, msg)


def test_overlap_refusals_name_both_sides():
    L = _lib().lib()
    assert "dL_ddepth overlaps depth" in _call(L, dL=0x10000)[1]
    assert "dL_ddepth overlaps gt_depth" in _call(L, dL=0x20000 - 4 * 23)[1]
    assert "dL_ddepth overlaps weight" in _call(L, dL=0x30000 + 4)[1]
    assert "terms overlaps weight" in _call(L, terms=0x30000)[1]


# ---------------------------------------------------------------------------------------------------- range_weight, depth_metrics: 3 x 4 by hand
def test_range_weight_by_hand():
    from gaussian_lic_amd import trainer
    d = torch.tensor([[0.0, 1.0, 2.0, 4.0], [-1.0, float("nan"), 10.0, 0.5], [20.0, 0.0, 3.0, 8.0]])
    w = trainer.range_weight(d, 0.5, 0.25)
    # sigma_abs / (sigma_abs + sigma_rel d): 0.5 / (0.5 + 0.25 d); every value below is exact in binary or the float32 quotient
    want = torch.tensor([[0.0, 0.5 / 0.75, 0.5, 0.5 / 1.5], [0.0, 0.0, 0.5 / 3.0, 0.8], [0.5 / 5.5, 0.0, 0.4, 0.2]], dtype=torch.float64).float()
    assert w.dtype == torch.float32 and tuple(w.shape) == (3, 4)
    assert torch.equal(w, want)
    assert torch.equal(trainer.range_weight(d, 0.5, 0.0), (d > 0).float())          # no relative term: 1 wherever there is a measurement
    assert float(trainer.range_weight(torch.tensor([1e-30]), 0.5, 0.25)) == 1.0    # 1 at the sensor
    for bad in ((0.0, 0.1), (-1.0, 0.1), (0.5, -0.1), (float("nan"), 0.1), (0.5, float("nan")), (float("inf"), 0.1)):
        with pytest.raises(ValueError, match="range_weight"):
            trainer.range_weight(d, *bad)


def test_depth_metrics_by_hand():
    from gaussian_lic_amd import loss
    gt = torch.tensor([[0.0, 2.0, 4.0, 10.0], [1.0, 0.0, 8.0, -1.0], [float("nan"), 5.0, 2.0, 0.0]])
    D = torch.tensor([[7.0, 2.5, 3.0, 13.0], [1.0, 9.0, 8.0, 3.0], [1.0, 4.0, 3.0, 2.0]])
    # measured pixels (gt > 0), D - d: 0.5, -1, 3, 0, 0, -1, 1  — seven of them
    m = loss.depth_metrics(D, gt)
    assert all(v.dtype == torch.float64 for v in m.values())
    assert float(m["n"]) == 7.0
    assert float(m["mae"]) == pytest.approx(6.5 / 7, rel=1e-15)
    assert float(m["rmse"]) == pytest.approx((12.25 / 7) ** 0.5, rel=1e-15)
    assert float(m["abs_rel"]) == pytest.approx((0.25 + 0.25 + 0.3 + 0 + 0 + 0.2 + 0.5) / 7, rel=1e-15)
    # max(D/d, d/D): 1.25 (not below), 1.333, 1.3, 1, 1, 1.25 (not below), 1.5 -> two of seven
    assert float(m["delta1"]) == pytest.approx(2 / 7, rel=1e-15)
    # weights: the pixel (0,1) counted twice, (0,2) left out, a NaN and a negative weight read as 0, +inf as 0
    w = torch.ones(3, 4)
    w[0, 1], w[0, 2], w[0, 3], w[1, 0], w[2, 1] = 2.0, 0.0, float("nan"), -3.0, float("inf")
    # left: (0,1) x2 [0.5], (1,2) [0], (2,2) [1]  -> S = 4
    mw = loss.depth_metrics(D, gt, w)
    assert float(mw["n"]) == 4.0
    assert float(mw["mae"]) == pytest.approx((2 * 0.5 + 0 + 1) / 4, rel=1e-15)
    assert float(mw["rmse"]) == pytest.approx(((2 * 0.25 + 0 + 1) / 4) ** 0.5, rel=1e-15)
    assert float(mw["abs_rel"]) == pytest.approx((2 * 0.25 + 0 + 0.5) / 4, rel=1e-15)
    assert float(mw["delta1"]) == pytest.approx(1 / 4, rel=1e-15)
    # nothing measured: zeros, no NaN
    z = loss.depth_metrics(D, torch.zeros(3, 4))
    assert all(float(v) == 0.0 for v in z.values())
    # a non-positive or NaN rendered depth fails the ratio test and does not poison the rest
    D2 = D.clone(); D2[1, 0] = 0.0                       # one of the two pixels that passed
    assert float(loss.depth_metrics(D2, gt)["delta1"]) == pytest.approx(1 / 7, rel=1e-15)
    D2[1, 2] = -8.0                                       # the other: a negative depth whose ratios are both below 1.25
    assert float(loss.depth_metrics(D2, gt)["delta1"]) == 0.0
    D2[0, 1] = float("nan")
    assert float(loss.depth_metrics(D2, gt)["delta1"]) == 0.0


# ---------------------------------------------------------------------------------------------------- depth_l1(weight, huber) on CPU tensors
def _case(seed, H=23, W=37):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(H, W, generator=g) * 10.0
    gt[torch.rand(H, W, generator=g) < 0.5] = 0.0
    gt[0, 0], gt[0, 1] = float("nan"), -2.0
    depth = gt + (torch.rand(H, W, generator=g) - 0.5) * 2.0
    depth = torch.where(torch.rand(H, W, generator=g) < 0.1, gt, depth)   # residual exactly 0
    w = torch.rand(H, W, generator=g) * 3.0                               # above 1 too
    w[1, :6] = torch.tensor([0.0, float("nan"), -1.0, float("inf"), 1e-40, 2.5])
    return depth, gt, w


@pytest.mark.parametrize("delta", [0.0, 0.25, 3.0])
@pytest.mark.parametrize("weighted", [False, True])
def test_depth_l1_matches_the_float64_restatement(delta, weighted):
    from gaussian_lic_amd import loss
    depth, gt, w = _case(5)
    w = w if weighted else None
    got = float(loss.depth_l1(depth, gt, w, delta))
    want = ref.loss64(depth.numpy(), gt.numpy(), None if w is None else w.numpy(), delta)
    n = ref.sums64(depth.numpy(), gt.numpy(), None if w is None else w.numpy(), delta)[2]
    assert n > 100
    # non-negative float32 summands: either sum is within n 2^-24 of the float64 one, whatever the order; the quotient adds one rounding
    assert abs(got - want) <= want * (2 * n + 2) * 2.0 ** -24
    # the gradient: lambda k w rho' with S in float64 here (autograd's S is a float32 sum of its own: one more n 2^-24)
    d = depth.clone().requires_grad_(True)
    loss.depth_l1(d, gt, w, delta).backward()
    S64 = ref.sums64(depth.numpy(), gt.numpy(), None if w is None else w.numpy(), delta)[0]
    m, wr, r, rho, drho = ref.pieces(depth.numpy(), gt.numpy(), None if w is None else w.numpy(), delta)
    want_g = np.where(m, wr.astype(np.float64) * drho.astype(np.float64) / S64, 0.0)
    assert not torch.isnan(d.grad).any()
    np.testing.assert_allclose(d.grad.numpy(), want_g, rtol=(n + 8) * 2.0 ** -24, atol=1e-12)
    assert float(d.grad[0, 0]) == 0.0 and float(d.grad[0, 1]) == 0.0 and (not weighted or not d.grad[1, :4].any())


@pytest.mark.parametrize("delta", [0.25, 3.0])
def test_depth_l1_huber_is_torch_smooth_l1(delta):
    from gaussian_lic_amd import loss
    depth, gt, _w = _case(6)
    m = gt > 0
    want = torch.nn.functional.smooth_l1_loss(depth[m].double(), gt[m].double(), beta=delta)
    got = loss.depth_l1(depth, gt, None, delta)
    assert abs(float(got) - float(want)) <= float(want) * (2 * int(m.sum()) + 2) * 2.0 ** -24


def test_depth_l1_defaults_are_the_old_graph_and_edge_cases():
    from gaussian_lic_amd import loss
    depth, gt, w = _case(7)
    d = depth.clone().requires_grad_(True)
    out = loss.depth_l1(d, gt)
    mask = gt > 0
    old = torch.where(mask, (depth - gt).abs(), torch.zeros_like(depth)).sum() / mask.sum().clamp_min(1).to(depth.dtype)
    assert torch.equal(out.detach(), old) and out.grad_fn.name() == "DivBackward0"
    assert torch.equal(loss.depth_l1(depth, gt, None, 0.0), old)
    # a 0/1 weight is the mask folded into the target; ones change nothing but the path
    keep = (w > 1.0).float()
    for delta in (0.0, 0.25):
        assert torch.equal(loss.depth_l1(depth, gt, keep, delta), loss.depth_l1(depth, torch.where(keep > 0, gt, torch.zeros_like(gt)), torch.ones_like(gt), delta))
    # all weights zero / nothing measured: 0 with a zero gradient, no NaN — also where the unmeasured depth is NaN
    dn = depth.clone(); dn[gt.isnan() | ~(gt > 0)] = float("nan")
    for wz, g in ((torch.zeros_like(gt), gt), (w, torch.zeros_like(gt)), (w, gt)):
        x = dn.clone().requires_grad_(True)
        y = loss.depth_l1(x, g, wz, 0.25)
        y.backward()
        assert torch.isfinite(y) and not torch.isnan(x.grad).any()
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="huber"):
            loss.depth_l1(depth, gt, None, bad)


def test_steps_refuse_a_depth_weight_without_a_depth_target():
    """The check runs before anything touches the device (the arguments here are never used)."""
    from gaussian_lic_amd import trainer
    w = torch.ones(4, 6)
    for fn in (trainer.training_step, trainer.training_step_fused, trainer.pose_gradient, trainer.training_step_with_pose):
        with pytest.raises(ValueError, match="without gt_depth"):
            fn(None, None, None, None, depth_weight=w)
        with pytest.raises(ValueError, match="without gt_depth"):
            fn(None, None, None, None, depth_huber=0.25)
        with pytest.raises(ValueError, match="depth_huber"):
            fn(None, None, None, None, gt_depth=w, lambda_depth=0.5, depth_huber=-1.0)
