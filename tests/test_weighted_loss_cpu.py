"""CPU-only: the weighted L1 + SSIM loss — the argument checks of the new entry point that return before any device work, its scratch size,
and the float64 reference the GPU tests compare against (tests/weighted_loss_ref.py): it reduces to the unweighted formula at w == 1, its
autograd gradient agrees with central differences, and it clamps the weights as the kernels do."""
import inspect

import numpy as np
import pytest
import torch

import weighted_loss_ref as wr


def _lib():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    return _lib, _lib.lib()


def test_weighted_loss_partials_count():
    _l, L = _lib()
    for H, W in ((1, 1), (31, 33), (240, 320), (1080, 1920)):
        tiles = ((H + 31) // 32) * ((W + 31) // 32)
        # two sums per tile and plane, the weight sum per tile, the two coefficients of the backward; never less than the unweighted scratch
        assert L.gslic_l1_ssim_loss_weighted_partials_count(3, H, W) >= 7 * tiles + 2
        assert L.gslic_l1_ssim_loss_weighted_partials_count(3, H, W) >= L.gslic_loss_partials_count(1, 3, H, W)
    slack = L.gslic_loss_partials_count(0, 3, 10, 10)          # the slack-only value of the neighbouring count
    for bad in ((0, 10, 10), (3, 0, 10), (3, 10, -4)):
        assert L.gslic_l1_ssim_loss_weighted_partials_count(*bad) == slack == 8


def test_weighted_loss_entry_point_validates_without_gpu():
    _l, L = _lib()
    none = [None] * 9
    for bad in ((0, 4, 4), (3, 0, 4), (3, 4, -1)):
        assert L.gslic_l1_ssim_loss_weighted_forward_backward(*bad, 1e-4, 9e-4, 0.2, *none, None) == -1
        assert b"empty" in L.gslic_last_error()
    assert L.gslic_l1_ssim_loss_weighted_forward_backward(3, 4, 4, 1e-4, 9e-4, 0.2, *none, None) == -1 and b"NULL" in L.gslic_last_error()
    # every pointer is checked: one NULL among otherwise plausible (never dereferenced) addresses
    import ctypes
    buf = (ctypes.c_float * 8)()
    ok = [ctypes.cast(buf, ctypes.c_void_p)] * 9
    for i in range(9):
        args = list(ok)
        args[i] = None
        assert L.gslic_l1_ssim_loss_weighted_forward_backward(3, 4, 4, 1e-4, 9e-4, 0.2, *args, None) == -1, i
        assert b"NULL" in L.gslic_last_error()
    assert _l.lib().gslic_abi_version() == 8


def test_python_surface_takes_the_weight():
    from gaussian_lic_amd import loss, trainer
    for fn in (loss.FusedLoss.forward_backward, loss.l1_ssim_loss, loss.psnr, trainer.training_step, trainer.training_step_fused, trainer.pose_gradient,
               trainer.training_step_with_pose, trainer.GraphedStep.__init__, trainer.GraphedStep.step, trainer._fused_losses):
        p = inspect.signature(fn).parameters
        assert "weight" in p and p["weight"].default is None, fn
    assert inspect.signature(loss.evaluate_visual_quality).parameters["weights"].default is None
    assert loss.FusedLoss(0.2).weight_sum is None


@pytest.mark.parametrize("H,W", [(12, 12), (33, 20)])
def test_reference_with_unit_weight_is_the_unweighted_formula(H, W):
    img, gt = wr.images(H, W, 3)
    a = float(wr.weighted_loss(img, gt, torch.ones(H, W)))
    b = float(wr.unweighted_loss(img, gt))
    assert abs(a - b) <= 1e-14
    t, _g = wr.weighted_reference(img, gt, torch.ones(H, W))
    assert t[2] == H * W and abs(t[0] - float((img.double() - gt.double()).abs().mean())) <= 1e-15


def test_reference_gradient_against_central_differences():
    H = W = 12
    g = torch.Generator().manual_seed(5)
    img = torch.rand(3, H, W, generator=g, dtype=torch.float64)
    sign = torch.where(torch.rand(3, H, W, generator=g) < 0.5, -1.0, 1.0).double()
    gt = img + sign * (0.02 + 0.3 * torch.rand(3, H, W, generator=g, dtype=torch.float64))    # |img - gt| >= 0.02: the L1 term is smooth across the step
    w = torch.rand(H, W, generator=g)
    w[2:5, 3:9] = 0.0
    _t, grad = wr.weighted_reference(img, gt, w)
    h = 1e-6
    num = torch.zeros_like(img)
    for i in range(img.numel()):
        d = torch.zeros(img.numel(), dtype=torch.float64)
        d[i] = h
        d = d.reshape(img.shape)
        num.view(-1)[i] = (float(wr.weighted_loss(img + d, gt, w)) - float(wr.weighted_loss(img - d, gt, w))) / (2 * h)
    assert float((img - gt).abs().min()) > 10 * h
    assert float((grad - num).abs().max()) <= 1e-8 * float(grad.abs().max()) + 1e-12
    assert float(grad.abs().max()) > 0


def test_reference_clamps_like_the_kernels_and_handles_no_weight():
    H, W = 20, 17
    img, gt = wr.images(H, W, 7)
    dirty = wr.weight_pattern("dirty", H, W)
    assert bool(torch.isnan(dirty).any()) and bool((dirty < 0).any()) and bool((dirty == 2).any()) and bool(torch.isinf(dirty).any())
    clean = wr.clamp_weight(dirty)
    assert bool(torch.isfinite(clean).all()) and float(clean.min()) == 0.0 and float(clean.max()) == 1.0
    assert bool((clean[torch.isnan(dirty) | (dirty < 0)] == 0).all()) and bool((clean[dirty > 1] == 1).all())
    keep = (dirty >= 0) & (dirty <= 1)
    assert torch.equal(clean[keep], dirty[keep])
    ta, ga = wr.weighted_reference(img, gt, dirty)
    tb, gb = wr.weighted_reference(img, gt, clean)
    assert np.array_equal(ta, tb) and torch.equal(ga, gb)
    from gaussian_lic_amd.loss import clamp_weight
    assert torch.equal(clamp_weight(dirty), clean)
    tz, gz = wr.weighted_reference(img, gt, torch.zeros(H, W))
    assert not tz.any() and not bool(gz.any())
    # a mask only moves the loss through the pixels it keeps
    m = wr.weight_pattern("frame", H, W)
    _t, gm = wr.weighted_reference(img, gt, m)
    assert bool(gm.abs().sum() > 0)


def test_weighted_psnr_and_fused_loss_value_are_plain_arithmetic():
    from gaussian_lic_amd import loss
    fl = loss.FusedLoss(0.2)
    t = torch.tensor([0.25, 0.5, 2.0])
    assert abs(float(fl.value(t)) - (0.8 * 0.25 + 0.2 * 0.5)) < 1e-7              # FusedLoss.value is unchanged
    assert abs(float(fl.value(t, 0.5)) - (0.8 * 0.25 + 0.2 * 0.5 + 1.0)) < 1e-6
    a, b = wr.images(9, 14, 1)
    assert torch.equal(loss.psnr(a, b), loss.psnr(a, b, None))
    assert abs(float(loss.psnr(a, b, torch.ones(9, 14))) - float(loss.psnr(a, b))) < 1e-4
    w = torch.zeros(9, 14)
    w[2:5, 3:7] = 1.0
    assert abs(float(loss.psnr(a, b, w)) - float(loss.psnr(a[:, 2:5, 3:7], b[:, 2:5, 3:7]))) < 1e-4
