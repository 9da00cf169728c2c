"""CPU-only: the host side of depth supervision on the fused path — the depth-aware scratch sizes (gslic_*_bytes_depth) and the argument checks
of the new entry points that return before any device work."""
import ctypes

import pytest


def _lib():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    return _lib, _lib.lib()


@pytest.mark.parametrize("W,H", [(64, 48), (320, 240), (1920, 1080), (70, 50)])
def test_depth_image_bytes_cover_the_colour_layout_plus_one_float_per_pixel(W, H):
    _l, L = _lib()
    T = ((W + 15) // 16) * ((H + 15) // 16)
    assert L.gslic_img_bytes_depth(W, H) >= L.gslic_img_bytes(W, H) + 4 * 256 * T
    assert L.gslic_img_bytes_depth(W + 16, H) > L.gslic_img_bytes_depth(W, H)


def test_depth_binning_and_sample_bytes_are_monotonic_and_cover_the_colour_sizes():
    _l, L = _lib()
    prev_b = prev_s = 0
    for n in (0, 1, 7, 64, 1000, 4096, 65537, 10 ** 6, 2 * 10 ** 7):
        b, s = L.gslic_binning_bytes_depth(n), L.gslic_sample_bytes_depth(n)
        assert b >= L.gslic_binning_bytes(n, 0) + 4 * n      # dL/dz per instance, behind the colour arrays
        assert s >= L.gslic_sample_bytes(n) + 4 * 256 * n    # the depth at every bucket start, per pixel
        assert b >= prev_b and s >= prev_s
        prev_b, prev_s = b, s
    assert L.gslic_binning_bytes_depth(-5) == L.gslic_binning_bytes_depth(0)


def test_depth_loss_partials_count():
    _l, L = _lib()
    for H, W in ((1, 1), (240, 320), (1080, 1920)):
        assert L.gslic_depth_l1_loss_partials_count(H, W) >= 2 * ((H * W + 2047) // 2048)
    assert L.gslic_depth_l1_loss_partials_count(0, 10) > 0


def test_depth_entry_points_validate_without_gpu():
    _l, L = _lib()
    # depth loss: empty image / NULL pointers
    assert L.gslic_depth_l1_loss_forward_backward(0, 10, 1.0, None, None, None, None, None, None) == -1
    assert L.gslic_depth_l1_loss_forward_backward(4, 4, 1.0, None, None, None, None, None, None) == -1 and b"NULL" in L.gslic_last_error()
    # capacity depth forward: out_depth NULL
    prm = _l.RasterParams(10, 3, 15, 64, 48, 1.0, 1.0, -1, 1, -1, 1, 1.0, 0, 0, 0, 1)
    R, B = ctypes.c_int32(0), ctypes.c_int32(0)
    rc = L.gslic_rasterize_forward_depth_capacity(ctypes.byref(prm), None, 0, None, 0, None, 0, None, 0, *([None] * 12), None, None, None, None,
                                                  ctypes.byref(R), ctypes.byref(B), None, None)
    assert rc == -1 and b"out_depth" in L.gslic_last_error()
    prm.no_color = 1
    rc = L.gslic_rasterize_forward_depth_capacity(ctypes.byref(prm), None, 0, None, 0, None, 0, None, 0, *([None] * 12), None, None, None, None,
                                                  ctypes.byref(R), ctypes.byref(B), None, None)
    assert rc == -1 and b"no_color" in L.gslic_last_error()
    prm.no_color = 0
    # fused-Adam depth backward: adam, dL_ddepth and dL_dmean3D are required
    ad = _l.AdamFused()
    args = lambda dLd, xyz_grad, adam: (ctypes.byref(prm), 0, 0, *([None] * 12), *([None] * 4), None, dLd, None, xyz_grad, None, None, None, None,
                                         0.0, adam, None)
    dummy = ctypes.c_void_p(16)   # (never dereferenced: the calls fail on their checks first)
    assert L.gslic_rasterize_backward_depth_adam(*args(dummy, dummy, None)) == -1 and b"adam" in L.gslic_last_error()
    assert L.gslic_rasterize_backward_depth_adam(*args(None, dummy, ctypes.byref(ad))) == -1 and b"dL_ddepth" in L.gslic_last_error()
    assert L.gslic_rasterize_backward_depth_adam(*args(dummy, None, ctypes.byref(ad))) == -1 and b"dL_dmean3D" in L.gslic_last_error()
    # P == 0: nothing to do
    prm.P = 0
    assert L.gslic_rasterize_backward_depth_adam(*args(None, None, None)) == 0


def test_fused_loss_value_with_and_without_depth():
    import torch
    from gaussian_lic_amd.loss import FusedLoss
    fl = FusedLoss(0.2)
    t = torch.tensor([0.5, 0.25, 2.0])
    assert float(fl.value(t[:2])) == pytest.approx(0.8 * 0.5 + 0.2 * 0.75)
    assert float(fl.value(t, 0.0)) == float(fl.value(t[:2]))
    assert float(fl.value(t, 0.1)) == pytest.approx(0.8 * 0.5 + 0.2 * 0.75 + 0.1 * 2.0)


def test_capacity_buffers_refuse_depth_without_colour():
    import torch
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import rasterizer as rz
    with pytest.raises(ValueError):
        rz.CapacityBuffers(10, 64, 48, 100, 10, torch.device("cpu"), no_color=True, depth=True)
    bufs = rz.CapacityBuffers(10, 64, 48, 100, 10, torch.device("cpu"), depth=True)
    _l, L = _lib()
    assert bufs.depth.shape == (48, 64) and bufs.img.numel() == L.gslic_img_bytes_depth(64, 48)
    assert bufs.binning.numel() == L.gslic_binning_bytes_depth(100) and bufs.sample.numel() == L.gslic_sample_bytes_depth(10)
