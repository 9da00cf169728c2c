"""CPU-only: the float64 restatement of the shared calibration's rule (tests/pose_shared_ref.py) — its two gradients against central finite
differences, X against the moves it accumulates, its no-ops one by one — the argument checks of gslic_pose_step_shared /
gslic_pose_calibrate_rows (made before any device work, so they run without a GPU; argument_cases() is shared with
tests/test_pose_shared_gpu.py) and the host-side interface and refusals of trainer.PoseSet(shared=True) and the steps that take it.

Finite differences: the step sizes (1e-7, checked against 2.5e-8) and the tolerance (5e-4 of the gradient's largest magnitude + 1e-7) are those of
the per-view chain's own finite-difference test, tests/test_camera_grad.py::test_pose_gradient_chain_matches_finite_differences."""
import ctypes
import types

import numpy as np
import pytest
import torch

import pose_ref as ref
import pose_shared_ref as sref

V = 4


def _camera(W=96, H=64, view="se3_c"):
    from gaussian_lic_amd.camera import synthetic_camera
    return synthetic_camera(W, H, view)


def _set(twist_scale=1.0, seed=0):
    """A reference set of V rows (the synthetic cameras' poses) with seeded twists, and the projection."""
    cams = [_camera(view=v) for v in ("se3_a", "se3_b", "se3_c", "se3_d")]
    rng = np.random.default_rng(seed)
    projection = np.asarray(cams[0].projection_matrix, np.float64).reshape(16)
    rows = []
    for c in cams:   # the cameras' float32 matrices are orthonormal to 6e-8 only: the rows start orthonormal in float64, as every moved row is
        Vm = ref.mat(c.world_view_transform.reshape(16))
        Vm[:3, :3] = ref.orthonormalise(Vm[:3, :3])
        rows.append(ref.recompose(Vm, projection))
    s = sref.new_set([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], rng.normal(size=(V, 6)) * twist_scale)
    return s, projection


def _grads(seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return tuple(rng.normal(size=n) * scale for n in (16, 16, 3))


# ------------------------------------------------------------------------------------------------ gradients against finite differences
def _toy_loss(view16, projection, weights):
    """A differentiable loss of T_cw through the three arrays the rasteriser reads: linear in view and proj, linear in campos = -R^T t."""
    Wv, Wp, wc = weights
    Vm = ref.mat(view16)
    _v, p, c = ref.recompose(Vm, projection)
    return float(Wv @ ref.flat(Vm) + Wp @ p + wc @ c)


def _moved(view16, d):
    """exp(d^) T, no re-orthonormalisation (the increment is what is differentiated)."""
    return ref.flat(ref.se3_exp(d) @ ref.mat(view16))


@pytest.mark.parametrize("i", [0, 2, 3])
def test_gradients_against_central_finite_differences(i):
    s, projection = _set()
    weights = _grads(10 + i)                       # the loss's weights ARE its three camera gradients (it is linear in the three arrays)
    g7 = sref.gradient(s, projection, weights, i)
    scale = max(float(np.abs(g7).max()), 1e-12)
    tol = 5e-4 * scale + 1e-7

    # L as a function of the whole set, rendered from row i: a common left increment moves every row, a time offset moves row j by dt xi_j
    def loss_common(xi):
        rows = [_moved(s["view"][j], xi) for j in range(V)]
        return _toy_loss(rows[i], projection, weights)

    def loss_tau(dt):
        rows = [_moved(s["view"][j], dt * s["twist"][j]) for j in range(V)]
        return _toy_loss(rows[i], projection, weights)

    def fd(f, h):
        return (f(+h) - f(-h)) / (2 * h)
    for k in range(6):
        e = np.zeros(6); e[k] = 1.0
        f1, f2 = fd(lambda h: loss_common(h * e), 1e-7), fd(lambda h: loss_common(h * e), 2.5e-8)
        assert abs(f1 - f2) <= 1e-3 * scale and abs(f1 - g7[k]) <= tol, (k, f1, f2, g7[k])
    f1, f2 = fd(loss_tau, 1e-7), fd(loss_tau, 2.5e-8)
    assert abs(f1 - f2) <= 1e-3 * scale and abs(f1 - g7[6]) <= tol, (f1, f2, g7[6])
    assert abs(g7[6] - float(s["twist"][i] @ g7[:6])) <= 1e-12 * scale and abs(g7[6]) > 0


# ------------------------------------------------------------------------------------------------ X tracks the moves
X_TOL = 1e-12   # float64: each of the K = 24 steps re-orthonormalises R (a few eps = 2.2e-16 of |T| <= ~10 each), on both sides of the comparison


def test_X_times_the_first_pose_is_the_last_pose_when_lr_time_is_0():
    s0, projection = _set()
    s = sref.copy_set(s0)
    K = 24
    for k in range(K):
        s, g7 = sref.step(s, projection, _grads(100 + k, 10.0 ** (k % 3 - 1)), k % V, 5e-3, 1e-2, 0.0)
        assert g7 is not None
    assert s["ssteps"] == K and s["tau"] == 0.0
    X4 = np.eye(4); X4[:3] = s["X"]
    worst = 0.0
    for j in range(V):
        worst = max(worst, float(np.abs(X4 @ ref.mat(s0["view"][j]) - ref.mat(s["view"][j])).max()))
    print(f"X tracks the moves: max |X T_j(0) - T_j(K)| over {V} rows and K = {K} steps {worst:.3e} (bar {X_TOL:.1e})")
    assert worst <= X_TOL
    assert float(np.abs(s["X"] - np.eye(3, 4)).max()) > 1e-2          # the steps went somewhere
    R = s["X"][:, :3]
    assert float(np.abs(R @ R.T - np.eye(3)).max()) <= 1e-14


# ------------------------------------------------------------------------------------------------ the no-ops of the reference
STATE = ("view", "proj", "campos", "twist", "sm", "sv", "X")


def _same(a, b, keys=STATE + ("ssteps", "tau")):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_no_ops_of_the_reference_one_by_one():
    s, projection = _set()
    grads = _grads(3)
    rates = (1e-3, 2e-3, 5e-4)
    # the step itself: every row, X, tau and the moments move
    new, g7 = sref.step(s, projection, grads, 1, *rates)
    assert new["ssteps"] == 1 and new["tau"] != 0 and all(not np.array_equal(new["view"][j], s["view"][j]) for j in range(V))
    assert not np.array_equal(new["X"], s["X"]) and (new["sm"] != 0).all()
    # skip: only grad_out
    kept, g_skip = sref.step(s, projection, grads, 1, *rates, skip=True)
    _same(kept, s)
    assert np.array_equal(g_skip, g7)
    # a gradient that is not finite: only grad_out, ssteps stays
    for bad in (np.nan, np.inf):
        poisoned = tuple(a.copy() for a in grads)
        poisoned[0][13] = bad
        kept, g_bad = sref.step(s, projection, poisoned, 1, *rates)
        _same(kept, s)
        assert not np.isfinite(g_bad).all()
    # g finite, g_tau not (an infinite twist coordinate on the stepped row)
    t = sref.copy_set(s)
    t["twist"][1, 0] = np.inf
    kept, g_bad = sref.step(t, projection, grads, 1, *rates)
    _same(kept, t)
    assert np.isfinite(g_bad[:6]).all() and not np.isfinite(g_bad[6])
    # all three rates zero: moments and ssteps move, nothing else
    new, _g = sref.step(s, projection, grads, 1, 0.0, 0.0, 0.0)
    _same(new, s, ("view", "proj", "campos", "X", "tau"))
    assert new["ssteps"] == 1 and (new["sm"] != 0).all() and (new["sv"] > 0).all()
    # d_x = 0, d_tau != 0: a row of zero twist keeps its bits while its neighbours move; X keeps its bits, tau moves
    t = sref.copy_set(s)
    t["twist"][2] = 0.0
    new, _g = sref.step(t, projection, grads, 1, 0.0, 0.0, 5e-4)
    assert np.array_equal(new["view"][2], t["view"][2]) and np.array_equal(new["campos"][2], t["campos"][2])
    assert all(not np.array_equal(new["view"][j], t["view"][j]) for j in (0, 1, 3))
    assert np.array_equal(new["X"], t["X"]) and new["tau"] != 0.0
    # a row whose d_j is not finite keeps its bits (an infinite twist on ANOTHER row: g_tau is finite, d_tau inf = inf there)
    t = sref.copy_set(s)
    t["twist"][3, 4] = np.inf
    new, _g = sref.step(t, projection, grads, 1, *rates)
    assert np.array_equal(new["view"][3], t["view"][3]) and all(not np.array_equal(new["view"][j], t["view"][j]) for j in (0, 1, 2))
    # d_tau not finite (eps = 0 on a zero second moment: the stepped row's twist is zero, so g_tau = 0): rows and tau keep their bits, X moves by d_x
    t = sref.copy_set(s)
    t["twist"][1] = 0.0
    new, g0 = sref.step(t, projection, grads, 1, *rates, eps=0.0)
    assert g0[6] == 0.0 and np.array_equal(new["view"], t["view"]) and new["tau"] == 0.0 and not np.array_equal(new["X"], t["X"])
    # a view word outside [0, V): nothing at all
    for bad in (-1, V, 1 << 30):
        kept, none = sref.step(s, projection, grads, bad, *rates)
        _same(kept, s)
        assert none is None


def test_calibrate_rows_of_the_reference():
    s0, projection = _set()
    # identity X and tau = 0: the matrix within the Gram-Schmidt rounding of float64
    new = sref.calibrate_rows(s0, projection, 1, 2)
    assert float(np.abs(new["view"] - s0["view"]).max()) <= 1e-15 * 10 and np.array_equal(new["view"][[0, 3]], s0["view"][[0, 3]])
    # after K extrinsic-only steps a fresh copy of an old row's start, calibrated, is the old row
    s = sref.copy_set(s0)
    for k in range(12):
        s, _g = sref.step(s, projection, _grads(200 + k), k % V, 5e-3, 1e-2, 0.0)
    fresh = sref.copy_set(s)
    fresh["view"][2], fresh["proj"][2], fresh["campos"][2] = s0["view"][2], s0["proj"][2], s0["campos"][2]
    got = sref.calibrate_rows(fresh, projection, 2, 1)
    assert float(np.abs(got["view"][2] - s["view"][2]).max()) <= X_TOL and float(np.abs(got["campos"][2] - s["campos"][2]).max()) <= X_TOL
    for j in (0, 1, 3):
        assert np.array_equal(got["view"][j], s["view"][j])


# ------------------------------------------------------------------------------------------------ the C-ABI argument checks
MEMBERS = ("view_all", "proj_all", "campos_all", "projection", "view", "twist", "sm", "sv", "ssteps", "X", "tau")
GRADS = ("dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos", "grad_out")
CALIBRATE_MEMBERS = ("view_all", "proj_all", "campos_all", "projection", "twist", "X", "tau")


def _fake(n_views=3):
    """A descriptor and gradient pointers over made-up, disjoint, non-NULL addresses: every call below must be refused before it touches them."""
    from gaussian_lic_amd import _lib
    a = {name: 0x10000000 + 0x1000 * k for k, name in enumerate(MEMBERS + GRADS)}
    d = _lib.PoseShared(**{n: a[n] for n in MEMBERS}, n_views=n_views, lr_trans=1e-3, lr_rot=1e-3, lr_time=1e-4, beta1=0.9, beta2=0.999, eps=1e-8,
                        skip=None)
    return d, [a[n] for n in GRADS], a


def argument_cases():
    """[(label, "step" | "calibrate", descriptor or None, arguments behind it, the words the message must hold)]."""
    cases = [("NULL descriptor", "step", None, _fake()[1], ("descriptor",)), ("NULL descriptor", "calibrate", None, [0, 1], ("descriptor",))]
    for name in MEMBERS:
        d, grads, a = _fake()
        setattr(d, name, None)
        cases.append((f"NULL {name}", "step", d, grads, (f"{name} is NULL",)))
    for name in CALIBRATE_MEMBERS:
        d, grads, a = _fake()
        setattr(d, name, None)
        cases.append((f"NULL {name}", "calibrate", d, [0, 1], (f"{name} is NULL",)))
    for k, name in enumerate(GRADS):
        d, grads, a = _fake()
        grads[k] = None
        cases.append((f"NULL {name}", "step", d, grads, (f"{name} is NULL",)))
    for kind, args in (("step", _fake()[1]), ("calibrate", [0, 0])):
        d, _g, a = _fake(n_views=0)
        cases.append(("n_views 0", kind, d, args, ("n_views",)))
    # overlaps: a gradient on the last float of row 2 of view_all, grad_out on the last float of sm, of X, on tau, on twist; grad_out on a gradient
    for g_k, target, offset in ((0, "view_all", 4 * (16 * 3 - 1)), (3, "sm", 4 * 6), (3, "X", 4 * 11), (3, "tau", 0), (3, "twist", 4 * (6 * 3 - 1)),
                                (1, "sv", 0), (2, "ssteps", 0)):
        d, grads, a = _fake()
        grads[g_k] = a[target] + offset
        cases.append((f"{GRADS[g_k]} on {target}", "step", d, grads, (f"{GRADS[g_k]} overlaps {target}",)))
    d, grads, a = _fake()
    grads[3] = grads[2] + 8
    cases.append(("grad_out on dL_dcampos", "step", d, grads, ("grad_out overlaps dL_dcampos",)))
    d, grads, a = _fake()
    grads[3] = grads[0] - 4 * 6                                                     # the seventh float of grad_out is the first of dL_dviewmatrix
    cases.append(("grad_out[6] on dL_dviewmatrix", "step", d, grads, ("grad_out overlaps dL_dviewmatrix",)))
    for name in ("lr_trans", "lr_rot", "lr_time", "beta1", "beta2", "eps"):
        for bad in (float("nan"), -1e-3):
            d, grads, a = _fake()
            setattr(d, name, bad)
            cases.append((f"{name} = {bad}", "step", d, grads, (name, "NaN or negative")))
    for name in ("beta1", "beta2"):
        d, grads, a = _fake()
        setattr(d, name, 1.0)
        cases.append((f"{name} = 1", "step", d, grads, (name, "below 1")))
    for first, count in ((-1, 1), (0, -1), (2, 2), (3, 1), (0, 4)):
        cases.append((f"rows [{first}, {first + count})", "calibrate", _fake()[0], [first, count], ("first", "n_views")))
    return cases


def run_argument_cases():
    from gaussian_lic_amd import _lib
    L = _lib.lib()
    cases = argument_cases()
    for label, kind, d, args, words in cases:
        ref_d = None if d is None else ctypes.byref(d)
        rc = L.gslic_pose_step_shared(ref_d, *args, None) if kind == "step" else L.gslic_pose_calibrate_rows(ref_d, *args, None)
        msg = L.gslic_last_error().decode()
        assert rc == -1 and all(w in msg for w in words), (label, kind, rc, msg)
    # count = 0 inside the range is a no-op that touches nothing
    assert L.gslic_pose_calibrate_rows(ctypes.byref(_fake()[0]), 3, 0, None) == 0
    return len(cases)


def test_argument_errors_without_gpu():
    assert run_argument_cases() == 2 + 11 + 7 + 4 + 2 + 7 + 2 + 12 + 2 + 5


# ------------------------------------------------------------------------------------------------ the host-side interface
def test_pose_set_shared_interface_on_a_cpu_device():
    from gaussian_lic_amd import trainer
    cams = [_camera(view=v) for v in ("se3_c", "se3_d")]
    plain = trainer.PoseSet(2, cams[0], "cpu")
    assert not plain.shared and not hasattr(plain, "X") and "X" not in plain.state_dict()          # shared=False: the set as it is
    ps = trainer.PoseSet(3, cams[0], "cpu", lr_rot=2e-3, lr_trans=5e-3, shared=True, lr_time=1e-4)
    assert ps.shared and ps.lr_time == 1e-4
    assert ps.twist.shape == (3, 6) and not bool(ps.twist.any()) and ps.sm.shape == ps.sv.shape == ps.shared_grad.shape == (7,)
    assert ps.ssteps.tolist() == [0] and ps.ssteps.dtype == torch.int32 and ps.tau.tolist() == [0.0]
    assert np.array_equal(ps.extrinsic(), np.eye(4)) and ps.time_offset() == 0.0
    ps.set_twist(1, [1, 2, 3, 4, 5, 6])
    ps.load(2, cams[1], twist=np.arange(6) * 0.5)
    assert ps.twist[1].tolist() == [1, 2, 3, 4, 5, 6] and ps.twist[2].tolist() == [0, 0.5, 1, 1.5, 2, 2.5] and not bool(ps.twist[0].any())
    assert np.array_equal(ps.view[2].numpy().view(np.int32), cams[1].world_view_transform.reshape(16).view(np.int32))     # calibrated=False: the bit copy
    with pytest.raises(ValueError, match="six values"):
        ps.set_twist(0, [1, 2, 3])
    with pytest.raises(IndexError):
        ps.set_twist(3, np.zeros(6))
    with pytest.raises(IndexError):
        ps.calibrate_rows(2, 2)
    ps.sm[:] = 1.0; ps.sv[:] = 2.0; ps.ssteps[0] = 7; ps.tau[0] = 0.25; ps.X[3] = 0.5; ps.shared_grad[:] = 3.0; ps.m[1] = 4.0
    other = ps.clone()
    for k in ("view", "proj", "campos", "m", "v", "steps", "twist", "sm", "sv", "ssteps", "X", "tau", "shared_grad"):
        assert torch.equal(getattr(other, k), getattr(ps, k)) and getattr(other, k).data_ptr() != getattr(ps, k).data_ptr(), k
    assert other.shared and other.lr_time == 1e-4 and other.time_offset() == 0.25 and other.extrinsic()[0, 3] == 0.5
    ps.reset_moments(shared=True)
    assert not bool(ps.sm.any()) and not bool(ps.sv.any()) and ps.ssteps.tolist() == [0] and not bool(ps.shared_grad.any())
    assert ps.time_offset() == 0.25 and ps.extrinsic()[0, 3] == 0.5 and bool(ps.m[1].all())       # the calibration and the per-view moments stay
    assert other.ssteps.tolist() == [7]
    fresh = trainer.PoseSet(3, cams[0], "cpu", shared=True)
    fresh.load_state_dict(other.state_dict())
    assert fresh.lr_time == 1e-4 and torch.equal(fresh.X, other.X) and torch.equal(fresh.twist, other.twist) and fresh.ssteps.tolist() == [7]
    with pytest.raises(ValueError, match="shared=True"):
        trainer.PoseSet(3, cams[0], "cpu").load_state_dict(other.state_dict())
    with pytest.raises(ValueError, match="shared=True"):
        fresh.load_state_dict(trainer.PoseSet(3, cams[0], "cpu").state_dict())


def test_refusals_that_need_no_device(monkeypatch):
    from gaussian_lic_amd import trainer
    cam = _camera()
    plain = trainer.PoseSet(2, cam, "cpu")
    shared = trainer.PoseSet(2, cam, "cpu", shared=True)
    for bad in (-1e-3, float("nan")):
        with pytest.raises(ValueError, match="lr_time"):
            trainer.PoseSet(2, cam, "cpu", shared=True, lr_time=bad)
    with pytest.raises(ValueError, match="without shared=True"):
        trainer.PoseSet(2, cam, "cpu", lr_time=1e-3)
    for call in (lambda: plain.set_twist(0, np.zeros(6)), lambda: plain.load(0, cam, twist=np.zeros(6)), lambda: plain.load(0, cam, calibrated=True),
                 lambda: plain.calibrate_rows(0, 1), plain.extrinsic, plain.time_offset, lambda: plain.reset_moments(shared=True),
                 lambda: plain.shared_adam_step(0, (torch.zeros(16), torch.zeros(16), torch.zeros(3)))):
        with pytest.raises(ValueError, match="without shared=True"):
            call()
    for step in (trainer.pose_gradient, trainer.training_step_with_pose):
        with pytest.raises(ValueError, match="shared=True needs poses"):
            step(None, cam, None, None, fused_loss=object(), shared=True)
        with pytest.raises(ValueError, match="built without shared=True"):
            step(None, cam, None, None, fused_loss=object(), poses=plain, view=0, shared=True)
        with pytest.raises(IndexError):
            step(None, cam, None, None, fused_loss=object(), poses=shared, view=2, shared=True)
    # GraphedStep: refused before any device work (a stand-in model: only its device is read before the check)
    model = types.SimpleNamespace(device=torch.device("cpu"))
    cam.to_device("cpu")
    with pytest.raises(ValueError, match="built without shared=True"):
        trainer.GraphedStep(model, cam, torch.zeros(3, 64, 96), None, poses=plain, view=0, train_pose="shared")
    with pytest.raises(ValueError, match="must be False, True or"):
        trainer.GraphedStep(model, cam, torch.zeros(3, 64, 96), None, poses=shared, view=0, train_pose="both")
    with pytest.raises(ValueError, match="needs poses"):
        trainer.GraphedStep(model, cam, torch.zeros(3, 64, 96), None, train_pose="shared")
    # N > 1: the shared calibration is single-GPU only, like the set itself
    monkeypatch.setattr(trainer, "_dist_on", lambda: True)
    for step in (trainer.pose_gradient, trainer.training_step_with_pose):
        with pytest.raises(NotImplementedError, match="single-GPU only"):
            step(None, cam, None, None, fused_loss=object(), poses=shared, view=0, shared=True)
