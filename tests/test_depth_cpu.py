"""CPU-only: depth rendering's host side — argument validation of gslic_rasterize_forward_depth / gslic_rasterize_backward_depth before any
device work, Camera.project_depth against a plain loop, and the masked depth L1."""
import ctypes

import numpy as np
import torch


def _prm(_lib, P=10, D=3, no_color=0):
    return _lib.RasterParams(P, D, 15, 64, 48, 1.0, 1.0, -1, 1, -1, 1, 1.0, 0, 0, no_color, 0)


def test_depth_entry_points_validate_without_gpu():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    L = _lib.lib()
    calls = []

    def alloc(_c, n):
        calls.append(n)
        return 0

    cb = _lib.ALLOC_FN(alloc)
    R, B = ctypes.c_int32(7), ctypes.c_int32(7)
    dummy = ctypes.c_void_p(16)   # never dereferenced: every call below fails (or returns) before any device work

    def fwd(prm, out_depth):
        return L.gslic_rasterize_forward_depth(ctypes.byref(prm), *([cb, None] * 4), *([None] * 12), None, dummy, out_depth, dummy,
                                               ctypes.byref(R), ctypes.byref(B), None)

    def bwd(prm, dL_ddepth):
        return L.gslic_rasterize_backward_depth(ctypes.byref(prm), 5, 5, *([None] * 12), *([dummy] * 4), dummy, dL_ddepth,
                                                *([None] * 10), 0.0, None)

    # forward: NULL out_depth, no_color = 1, SH degree > 3
    assert fwd(_prm(_lib), None) == -1 and b"out_depth" in L.gslic_last_error()
    assert fwd(_prm(_lib, no_color=1), dummy) == -1 and b"no_color" in L.gslic_last_error()
    assert fwd(_prm(_lib, D=5), dummy) == -1 and b"degree" in L.gslic_last_error()
    # backward: the same three
    assert bwd(_prm(_lib), None) == -1 and b"dL_ddepth" in L.gslic_last_error()
    assert bwd(_prm(_lib, no_color=1), dummy) == -1 and b"no_color" in L.gslic_last_error()
    assert bwd(_prm(_lib, D=5), dummy) == -1 and b"degree" in L.gslic_last_error()
    assert not calls
    # P = 0: nothing to do, no allocator call, R = B = 0
    R.value, B.value = 7, 7
    assert fwd(_prm(_lib, P=0), None) == 0 and R.value == 0 and B.value == 0
    assert bwd(_prm(_lib, P=0), None) == 0
    assert not calls


def _project_loop(cam, pts):
    """gaussian.cpp:548-565 as a plain loop in float32: nearest point per pixel, 0 elsewhere."""
    W, H = cam.image_width, cam.image_height
    R_cw = cam.R_wc.T.astype(np.float32)
    t_cw = (-cam.R_wc.T @ cam.t_wc).astype(np.float32)
    f32 = np.float32
    out = np.zeros((H, W), np.float32)
    best = {}
    for p in pts.astype(np.float32):
        pc = [f32(f32(f32(f32(p[0] * R_cw[i, 0]) + f32(p[1] * R_cw[i, 1])) + f32(p[2] * R_cw[i, 2])) + t_cw[i]) for i in range(3)]
        z = pc[2]
        if not z > 0:
            continue
        x = int(np.floor(f32(f32(f32(pc[0] * cam.fx) / z) + cam.cx)))
        y = int(np.floor(f32(f32(f32(pc[1] * cam.fy) / z) + cam.cy)))
        if not (0 <= x < W and 0 <= y < H):
            continue
        if (x, y) not in best or z < best[(x, y)]:
            best[(x, y)] = z
    for (x, y), z in best.items():
        out[y, x] = z
    return out


def test_project_depth_matches_a_plain_loop():
    from gaussian_lic_amd.camera import Camera, rotation_ypr
    W, H = 40, 30
    cam = Camera(W, H, 30.0, 32.0, 19.5, 15.2, R_wc=rotation_ypr(10.0, -5.0, 3.0), t_wc=np.array([0.2, -0.1, 0.3]))
    rng = np.random.default_rng(3)
    n = 4000
    # points in front of the camera (a cloud that hits the image and spills past its border), some behind it, and exact duplicates in depth
    pc = np.stack([rng.uniform(-1.2, 1.2, n), rng.uniform(-1.0, 1.0, n), rng.uniform(-0.5, 4.0, n)], 1)
    pc[:200, 2] = -pc[:200, 2] - 0.1                                    # behind the camera
    pw = pc @ cam.R_wc.T + cam.t_wc                                      # camera frame -> world
    pts = torch.from_numpy(pw.astype(np.float32))
    got = cam.project_depth(pts).numpy()
    ref = _project_loop(cam, pts.numpy())
    assert got.shape == (H, W)
    np.testing.assert_array_equal(got, ref)
    assert (ref > 0).sum() > 300 and (ref == 0).sum() > 0                # many pixels hit, some empty
    # the nearest point wins: put a far point and a near one on the same pixel
    near = cam.R_wc @ np.array([0.0, 0.0, 1.0]) + cam.t_wc
    far = cam.R_wc @ np.array([0.0, 0.0, 3.0]) + cam.t_wc
    d = cam.project_depth(torch.tensor(np.stack([far, near]), dtype=torch.float32)).numpy()
    assert (d > 0).sum() == 1 and abs(float(d.max()) - 1.0) < 1e-5
    # everything behind the camera or outside the image: all zeros
    assert cam.project_depth(torch.tensor([[0.0, 0.0, -1.0], [100.0, 0.0, 1.0]]) @ torch.from_numpy(cam.R_wc.T.astype(np.float32))
                             + torch.from_numpy(cam.t_wc.astype(np.float32))).abs().sum() == 0


def test_depth_l1_is_masked():
    from gaussian_lic_amd.loss import depth_l1
    depth = torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], requires_grad=True)
    gt = torch.tensor([[0.0, 2.5, 0.0], [3.0, 0.0, -1.0]])              # measured at (0, 1) and (1, 0) only (gt > 0)
    loss = depth_l1(depth, gt)
    assert abs(float(loss.detach()) - (0.5 + 1.0) / 2) < 1e-7
    loss.backward()
    np.testing.assert_array_equal(depth.grad.numpy(), np.array([[0.0, -0.5, 0.0], [0.5, 0.0, 0.0]], np.float32))
    d2 = torch.ones(2, 3, requires_grad=True)
    z = depth_l1(d2, torch.zeros(2, 3))                                 # no measurement at all: 0, and backward works
    assert float(z.detach()) == 0.0
    z.backward()
    assert float(d2.grad.abs().sum()) == 0.0
