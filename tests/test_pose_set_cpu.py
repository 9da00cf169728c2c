"""CPU-only: the float64 restatement of the pose set's rule (tests/pose_ref.py) against the library's own host code (camera.se3_exp,
Camera.pose_gradient) and torch.optim.Adam, the level invariance of projection_matrix on bits, the argument checks of gslic_pose_step /
gslic_pose_load (made before any device work, so they run without a GPU), and trainer.PoseSet's host-side interface on a CPU device."""
import ctypes

import numpy as np
import pytest
import torch

import pose_ref as ref


def _camera(W=96, H=64, view="se3_c"):
    from gaussian_lic_amd.camera import synthetic_camera
    return synthetic_camera(W, H, view)


def test_exp_equals_camera_se3_exp():
    from gaussian_lic_amd.camera import se3_exp
    rng = np.random.default_rng(0)
    cases = [np.zeros(6), np.r_[rng.normal(size=3), 0, 0, 0], np.r_[0, 0, 0, 0.3, -0.4, 0.1]]
    for theta in (1e-9, 1e-6, 0.99e-4, 1.01e-4, 1e-2, 0.5, 3.0):      # both branches of either implementation, and around either threshold
        phi = rng.normal(size=3)
        cases.append(np.r_[rng.normal(size=3), phi / np.linalg.norm(phi) * theta])
    # camera.se3_exp takes its closed branch from theta = 1e-8 on, where (1 - cos theta) / theta^2 cancels in float64: b carries a relative error of
    # about eps / theta^2, which reaches the translation as eps |rho| / theta (pose_ref switches to the series below 1e-4 and has no such term).
    # The bar is 1e-12 plus four times that term; it is 1e-12 itself wherever camera.se3_exp is accurate.
    eps = np.finfo(np.float64).eps
    for xi in cases:
        theta = float(np.linalg.norm(xi[3:]))
        tol = 1e-12 + (4.0 * eps * float(np.linalg.norm(xi[:3])) / theta if theta >= 1e-8 else 0.0)
        assert np.abs(ref.se3_exp(xi) - se3_exp(xi)).max() <= tol, xi


def test_series_coefficients_are_the_closed_forms_to_fourth_order():
    """Below theta = 1e-4 the second term of each series is under 1e-9 of the first, so no comparison of poses there can tell a wrong one.  The
    series itself is checked where its terms are visible: at theta = 0.05 .. 0.2 it must meet the closed forms up to the first neglected terms,
    theta^4 / 120, theta^4 / 720 and theta^4 / 5040 (a wrong theta^2 coefficient would miss by about theta^2 / 10)."""
    for theta in (0.05, 0.1, 0.2):
        for got, want, next_term in zip(ref.series_coefficients(theta), ref.closed_coefficients(theta), (120.0, 720.0, 5040.0)):
            gap = abs(got - want)
            assert 0.5 * theta ** 4 / next_term <= gap <= 1.01 * theta ** 4 / next_term, (theta, got, want)
    assert ref.exp_coefficients(0.99e-4) == ref.series_coefficients(0.99e-4) and ref.exp_coefficients(1.01e-4) == ref.closed_coefficients(1.01e-4)


def test_chain_equals_camera_pose_gradient():
    rng = np.random.default_rng(1)
    for view in ("se3_a", "se3_b", "se3_c", "se3_d", None):
        cam = _camera(view=view)
        dv, dp, dc = rng.normal(size=16), rng.normal(size=16), rng.normal(size=3)
        want = cam.pose_gradient(dv, dp, dc)
        got = ref.chain(cam.world_view_transform.reshape(16), cam.projection_matrix.reshape(16), dv, dp, dc)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_adam_equals_torch_adam_with_two_parameter_groups():
    rng = np.random.default_rng(2)
    lr_t, lr_r, betas, eps = 2e-3, 5e-4, (0.9, 0.999), 1e-8
    f = lambda x: float(np.float32(x))                                  # (pose_ref takes the scalars as the float32 the kernel is handed)
    rho, phi = torch.zeros(3, dtype=torch.float64, requires_grad=True), torch.zeros(3, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([dict(params=[rho], lr=f(lr_t)), dict(params=[phi], lr=f(lr_r))], betas=(f(betas[0]), f(betas[1])), eps=f(eps))
    m, v, n, total = np.zeros(6), np.zeros(6), 0, np.zeros(6)
    for _ in range(20):
        g = rng.normal(size=6) * 10.0 ** rng.uniform(-3, 1)
        rho.grad, phi.grad = torch.from_numpy(g[:3].copy()), torch.from_numpy(g[3:].copy())
        opt.step()
        delta, m, v, n = ref.adam(g, m, v, n, lr_t, lr_r, betas, eps)
        total += delta
        want = np.r_[rho.detach().numpy(), phi.detach().numpy()]
        assert np.abs(total - want).max() <= 1e-12 * np.abs(want).max()
    assert n == 20


def test_projection_matrix_is_the_same_bits_at_pyramid_levels_0_to_2():
    """projection_matrix, tanfov and the four limits depend on fx / W, cx / W, fy / H, cy / H and the depth range alone: a size divisible by 2^l
    keeps their bits at level l, so one PoseSet serves those levels (its check passes and camera(view, level) is the row at that size); a width
    that is not divisible drops a column and changes cx / W."""
    from gaussian_lic_amd import trainer
    cam = _camera(1920, 1080)
    ps = trainer.PoseSet(1, cam, "cpu")
    f32 = lambda x: np.float32(x).view(np.int32)
    for level in (0, 1, 2):
        at = cam.at_level(level)
        assert np.array_equal(at.projection_matrix.view(np.int32), cam.projection_matrix.view(np.int32)), level
        for k in trainer.PoseSet._BAKED:
            assert f32(getattr(at, k)) == f32(getattr(cam, k)), (level, k)
        assert ps.matches(at)
        assert trainer._check_poses("t", ps, 0, at) is ps                        # what every step checks
        back = ps.camera(0, level=level)
        assert (back.image_width, back.image_height) == (1920 >> level, 1080 >> level) and ps.matches(back)
        assert np.array_equal(back.full_proj_transform.view(np.int32), cam.full_proj_transform.view(np.int32))
    odd = _camera(1918, 1080)
    assert not np.array_equal(odd.at_level(2).projection_matrix, odd.projection_matrix)
    assert not trainer.PoseSet(1, odd, "cpu").matches(odd.at_level(2))
    with pytest.raises(ValueError, match="differ from the pose set"):
        trainer._check_poses("t", ps, 0, odd)


def test_poses_under_a_process_group_are_refused(monkeypatch):
    from gaussian_lic_amd import trainer
    cam = _camera()
    ps = trainer.PoseSet(1, cam, "cpu")
    monkeypatch.setattr(trainer, "_dist_on", lambda: True)
    assert trainer._check_poses("t", None, 0) is None
    for call in (lambda: trainer._check_poses("t", ps, 0, cam),
                 lambda: trainer.pose_gradient(None, cam, None, None, fused_loss=object(), poses=ps, view=0),
                 lambda: trainer.training_step_with_pose(None, cam, None, None, fused_loss=object(), poses=ps, view=0)):
        with pytest.raises(NotImplementedError, match="single-GPU only"):
            call()


def _fake(n_views=3):
    """A descriptor and gradient pointers over made-up, disjoint, non-NULL addresses: every call below must be refused before it touches them."""
    from gaussian_lic_amd import _lib
    base = 0x10000000
    a = [base + 0x1000 * k for k in range(13)]
    d = _lib.PoseAdam(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], n_views, 1e-3, 1e-3, 0.9, 0.999, 1e-8, None)
    return d, a[8:12], a


MEMBERS = ("view_all", "proj_all", "campos_all", "m", "v", "step_count", "projection", "view")
GRADS = ("dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos", "grad_out")


def _step(d, grads):
    from gaussian_lic_amd import _lib
    L = _lib.lib()
    rc = L.gslic_pose_step(None if d is None else ctypes.byref(d), *grads, None)
    return rc, L.gslic_last_error().decode()


def test_pose_step_argument_errors_without_gpu():
    d, grads, a = _fake()
    rc, msg = _step(None, grads)
    assert rc == -1 and "descriptor" in msg
    for name in MEMBERS:
        d, grads, a = _fake()
        setattr(d, name, None)
        rc, msg = _step(d, grads)
        assert rc == -1 and f"{name} is NULL" in msg, msg
    for k, name in enumerate(GRADS):
        d, grads, a = _fake()
        grads[k] = None
        rc, msg = _step(d, grads)
        assert rc == -1 and f"{name} is NULL" in msg, msg
    d, grads, a = _fake(n_views=0)
    rc, msg = _step(d, grads)
    assert rc == -1 and "n_views" in msg
    # a gradient inside a state array (the last float of the third row of view_all), grad_out on a moment row, grad_out on a gradient
    d, grads, a = _fake()
    grads[0] = a[0] + 4 * (16 * 3 - 1)
    rc, msg = _step(d, grads)
    assert rc == -1 and "dL_dviewmatrix overlaps view_all" in msg, msg
    d, grads, a = _fake()
    grads[3] = a[3] + 4 * 6
    rc, msg = _step(d, grads)
    assert rc == -1 and "grad_out overlaps m" in msg, msg
    d, grads, a = _fake()
    grads[3] = grads[2] + 8
    rc, msg = _step(d, grads)
    assert rc == -1 and "grad_out overlaps dL_dcampos" in msg, msg
    for name in ("lr_trans", "lr_rot", "beta1", "beta2", "eps"):
        for bad in (float("nan"), -1e-3):
            d, grads, a = _fake()
            setattr(d, name, bad)
            rc, msg = _step(d, grads)
            assert rc == -1 and name in msg and "NaN or negative" in msg, msg
    for name in ("beta1", "beta2"):
        for bad in (1.0, 1.5):
            d, grads, a = _fake()
            setattr(d, name, bad)
            rc, msg = _step(d, grads)
            assert rc == -1 and name in msg and "below 1" in msg, msg


def test_pose_load_argument_errors_without_gpu():
    from gaussian_lic_amd import _lib
    L = _lib.lib()
    a = [0x20000000 + 0x1000 * k for k in range(7)]
    names = ("view_all", "proj_all", "campos_all", "view_word", "view_out", "proj_out", "campos_out")

    def call(ptrs, n_views=3):
        rc = L.gslic_pose_load(*ptrs[:4], n_views, *ptrs[4:], None)
        return rc, L.gslic_last_error().decode()

    for k, name in enumerate(names):
        ptrs = list(a)
        ptrs[k] = None
        rc, msg = call(ptrs)
        assert rc == -1 and f"{name} is NULL" in msg, msg
    for n in (0, -2):
        rc, msg = call(list(a), n)
        assert rc == -1 and "n_views" in msg
    ptrs = list(a)
    ptrs[4] = a[0] + 4 * 16 * 2           # view_out on row 2 of view_all
    rc, msg = call(ptrs)
    assert rc == -1 and "view_out overlaps view_all" in msg, msg
    ptrs = list(a)
    ptrs[6] = a[5] + 4 * 15               # campos_out on the last float of proj_out
    rc, msg = call(ptrs)
    assert rc == -1 and "campos_out overlaps proj_out" in msg, msg


def test_pose_set_host_interface_on_a_cpu_device():
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    cams = [_camera(view=v) for v in ("se3_c", "se3_d")]
    ps = trainer.PoseSet(3, cams[0], "cpu", lr_rot=2e-3, lr_trans=5e-3)
    ps.load(1, cams[1])
    for i, cam in ((0, cams[0]), (1, cams[1]), (2, cams[0])):               # bit copies of the camera's arrays; unloaded rows hold the set's camera
        v, p, c = ps.pose(i)
        assert np.array_equal(v.numpy().view(np.int32), cam.world_view_transform.reshape(16).view(np.int32))
        assert np.array_equal(p.numpy().view(np.int32), cam.full_proj_transform.reshape(16).view(np.int32))
        assert np.array_equal(c.numpy().view(np.int32), cam.camera_center.view(np.int32))
    assert ps.pose(1)[0].data_ptr() == ps.view[1].data_ptr()               # views, not copies
    back = ps.camera(1)
    assert np.abs(back.R_wc - cams[1].R_wc).max() < 1e-6 and np.abs(back.t_wc - cams[1].t_wc).max() < 1e-6
    assert np.array_equal(back.full_proj_transform.view(np.int32), cams[1].full_proj_transform.view(np.int32))
    assert ps.matches(back)
    with pytest.raises(ValueError, match="differ from the pose set"):
        ps.load(0, synthetic_camera(96, 64 + 16, "se3_c"))                  # another image size: other baked scalars and projection
    with pytest.raises(IndexError):
        ps.pose(3)
    with pytest.raises(ValueError):
        trainer.PoseSet(2, cams[0], "cpu", betas=(0.9, 1.0))
    ps.m[1] = 1.0; ps.v[1] = 2.0; ps.steps[1] = 7
    other = ps.clone()
    for k in ("view", "proj", "campos", "m", "v", "steps"):
        assert torch.equal(getattr(other, k), getattr(ps, k)), k
    assert (other.lr_rot, other.lr_trans) == (2e-3, 5e-3)
    ps.reset_moments(1)
    assert ps.steps.tolist() == [0, 0, 0] and not bool(ps.m.any()) and not bool(ps.v.any())
    assert other.steps.tolist() == [0, 7, 0]
    assert trainer._check_poses("t", None, 0) is None
    with pytest.raises(ValueError, match="trainer.PoseSet"):
        trainer._check_poses("t", object(), 0)
    with pytest.raises(IndexError):
        trainer._check_poses("t", ps, 5)
    with pytest.raises(ValueError, match="do_step=True needs poses"):
        trainer.pose_gradient(None, cams[0], None, None, fused_loss=object(), do_step=True)
