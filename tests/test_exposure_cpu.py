"""CPU-only: the exposure model without a device — the restatement (tests/exposure_ref.py) against torch's float64 autograd and torch.optim.Adam,
the float32 wording of the Adam rule and the float64 sums inside the bounds the GPU tests assert, the three exports and every refusal (reported
before any device work), and trainer.Exposure's state."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import exposure_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG = -1


def _lib():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------------- the restatement
def test_float64_backward_is_autograd_of_einsum():
    E, x, g = ref.case(33, 17, 1)
    Et = torch.tensor(E, dtype=torch.float64, requires_grad=True)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    out = torch.einsum("ck,khw->chw", Et[:, :3], xt) + Et[:, 3][:, None, None]
    np.testing.assert_allclose(out.detach().numpy(), ref.apply64(E, x), rtol=1e-14, atol=1e-15)
    out.backward(torch.tensor(g, dtype=torch.float64))
    dimg, dE, mag = ref.backward64(E, x, g)
    np.testing.assert_allclose(xt.grad.numpy(), dimg, rtol=1e-13, atol=1e-18)
    np.testing.assert_allclose(Et.grad.numpy(), dE, rtol=0, atol=1e-13 * mag.max())
    # the float32 rule is the float64 one up to its own roundings (3 products and 3 sums of magnitudes below 1.5 * 1 + 1.5)
    assert np.abs(ref.apply32(E, x).astype(np.float64) - ref.apply64(E, x)).max() <= 8 * 6.0 * 2.0 ** -24
    assert np.abs(ref.dimage32(E, g).astype(np.float64) - dimg).max() <= 8 * np.abs(g).max() * 4.5 * 2.0 ** -24
    assert np.array_equal(ref.apply32(ref.IDENTITY, x).view(np.int32), x.view(np.int32))   # [I | 0] returns the image's own bits


def test_float64_sum_is_far_inside_the_bound_of_the_gpu_test():
    """The GPU test holds each entry of dL_dE to n 2^-24 sum_p |g x| of the float64 sum: the worst case of ANY float32 summation order.  The float64
    reference's own error (n 2^-53 of the same sum) has to be negligible against it — and a float32 sum in another order has to pass."""
    for H, W in ((1, 1), (1, 63), (33, 17), (70, 50), (160, 120)):
        E, x, g = ref.case(H, W, 7)
        n = H * W
        _dimg, dE, mag = ref.backward64(E, x, g)
        bound = n * 2.0 ** -24 * mag
        assert (n * 2.0 ** -53 * mag <= bound * 1e-8).all()
        x1 = np.concatenate([x, np.ones_like(x[:1])])
        dE32 = np.array([[np.sum((g[c] * x1[k]).astype(np.float32).ravel(), dtype=np.float32) for k in range(4)] for c in range(3)])
        assert (np.abs(dE32.astype(np.float64) - dE) <= bound).all()


def test_reference_adam_is_torch_adam_over_five_steps():
    rng = np.random.default_rng(3)
    lr, b1, b2, eps = 0.01, 0.9, 0.999, 1e-8
    p0 = rng.uniform(-1.5, 1.5, (3, 4))
    pt = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([pt], lr=lr, betas=(b1, b2), eps=eps)
    p, m, v, t = p0.copy(), np.zeros((3, 4)), np.zeros((3, 4)), 0
    for _step in range(5):
        g = rng.standard_normal((3, 4)) * 10.0 ** rng.uniform(-6, 0, (3, 4))
        pt.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        p, m, v, t = ref.adam64(p, m, v, t, g, lr, b1, b2, eps)
        np.testing.assert_allclose(pt.detach().numpy(), p, rtol=1e-13, atol=1e-15)
    assert t == 5


def test_float32_wording_of_adam_is_inside_the_bound_of_the_gpu_test():
    """|dp - dp_ref| <= 16 2^-24 |dp_ref| + 2^-24 |p| per element and step, against a float64 trajectory that runs FREE from the same start on the
    same float32 gradients (the GPU test's comparison), with the scalars the float32 values the descriptor holds."""
    rng = np.random.default_rng(4)
    lr, b1, b2, eps = (float(np.float32(a)) for a in (0.01, 0.9, 0.999, 1e-8))
    p32 = rng.uniform(-1.5, 1.5, (2, 12)).astype(np.float32)
    m32, v32, t32 = np.zeros_like(p32), np.zeros_like(p32), [0, 0]
    p64, m64, v64, t64 = p32.astype(np.float64), np.zeros((2, 12)), np.zeros((2, 12)), [0, 0]
    for step in range(5):
        i = step % 2
        g = (rng.standard_normal(12) * 10.0 ** rng.uniform(-5, 0, 12)).astype(np.float32)
        before32, before64 = p32[i].copy(), p64[i].copy()
        p32[i], m32[i], v32[i], t32[i] = ref.adam32(p32[i], m32[i], v32[i], t32[i], g, lr, b1, b2, eps)
        p64[i], m64[i], v64[i], t64[i] = ref.adam64(p64[i], m64[i], v64[i], t64[i], g, lr, b1, b2, eps)
        dp, dp_ref = p32[i].astype(np.float64) - before32.astype(np.float64), p64[i] - before64
        assert (np.abs(dp - dp_ref) <= 16 * 2.0 ** -24 * np.abs(dp_ref) + 2.0 ** -24 * np.abs(before32)).all(), step
    assert t32 == [3, 2]


# ---------------------------------------------------------------------------------------------------- the exports and their refusals
def test_symbols_are_exported_and_declared():
    _l = _lib()
    L = _l.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gslic_hip.h")).read(), flags=re.S)
    for sym in ("gslic_exposure_apply", "gslic_exposure_backward", "gslic_exposure_partials_count"):
        assert hasattr(ctypes.CDLL(_l.LIB_PATH), sym), sym
        assert sym in _l.EXPORTS and re.search(r"\b" + sym + r"\s*\(", header), sym
    assert L.gslic_abi_version() == 8
    count = L.gslic_exposure_partials_count
    assert count(1, 1) == 12 and count(1080, 1920) % 12 == 0 and count(1080, 1920) >= 12 * 1013 and count(0, 5) > 0 and count(5, -1) > 0


IMG = 3 * 4 * 6 * 4   # bytes of a [3,4,6] float image


def _apply(L, H=4, W=6, E=0x10000, image=0x20000, out=0x30000):
    vp = lambda a: None if a is None else ctypes.c_void_p(a)
    rc = L.gslic_exposure_apply(H, W, vp(E), vp(image), vp(out), None)
    return rc, L.gslic_last_error().decode()


def _adam(_l, **kw):
    d = dict(param=0x100000, m=0x110000, v=0x120000, step_count=0x130000, view=0x140000, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, skip=None)
    d.update(kw)
    return _l.ExposureAdam(*(d[k] for k in ("param", "m", "v", "step_count", "view", "lr", "beta1", "beta2", "eps", "skip")))


def _backward(_l, H=4, W=6, E=0x10000, image=0x20000, g=0x30000, dimage=0x40000, partials=0x50000, dE=0x60000, adam=None):
    L = _l.lib()
    vp = lambda a: None if a is None else ctypes.c_void_p(a)
    rc = L.gslic_exposure_backward(H, W, vp(E), vp(image), vp(g), vp(dimage), vp(partials), vp(dE), None if adam is None else ctypes.byref(adam), None)
    return rc, L.gslic_last_error().decode()


@pytest.mark.parametrize("kw,name", [
    (dict(H=0), "H"), (dict(H=-2), "H"), (dict(W=0), "W"), (dict(W=-1), "W"),
    (dict(E=None), "E"), (dict(image=None), "image"), (dict(out=None), "out"),
    (dict(out=0x20000), "image"), (dict(out=0x20000 + IMG - 4), "image"), (dict(out=0x20000 - 4), "image"),
    (dict(out=0x10000 + 44), "E"), (dict(out=0x10000 - IMG + 4), "E"),
])
def test_apply_refusals_name_the_argument(kw, name):
    rc, msg = _apply(_lib().lib(), **kw)
    assert rc == ERR_INVALID_ARG, (kw, rc)
    assert re.search(r"\b" + name + r"\b", msg), (kw, msg)


@pytest.mark.parametrize("kw,name", [
    (dict(H=0), "H"), (dict(W=-5), "W"),
    (dict(E=None), "E"), (dict(image=None), "image"), (dict(g=None), "dL_dout"), (dict(dimage=None), "dL_dimage"), (dict(partials=None), "partials"),
    (dict(dE=None), "dL_dE"),
    (dict(dimage=0x10000), "dL_dimage overlaps E"), (dict(dimage=0x20000 + 4), "dL_dimage overlaps image"), (dict(dimage=0x30000 - 4), "dL_dimage overlaps dL_dout"),
    (dict(dE=0x10000 + 44), "dL_dE overlaps E"), (dict(dE=0x20000 + IMG - 4), "dL_dE overlaps image"), (dict(dE=0x30000 - 44), "dL_dE overlaps dL_dout"),
    (dict(dE=0x40000 + 8), "dL_dE overlaps dL_dimage"),
])
def test_backward_refusals_name_the_argument(kw, name):
    rc, msg = _backward(_lib(), **kw)
    assert rc == ERR_INVALID_ARG, (kw, rc)
    assert name in msg, (kw, msg)


@pytest.mark.parametrize("kw,name", [
    (dict(param=None), "param"), (dict(m=None), "m"), (dict(v=None), "v"), (dict(step_count=None), "step_count"), (dict(view=None), "view"),
    (dict(lr=-0.01), "lr"), (dict(lr=float("nan")), "lr"), (dict(eps=-1e-8), "eps"), (dict(eps=float("nan")), "eps"),
    (dict(beta1=-0.1), "beta1"), (dict(beta1=float("nan")), "beta1"), (dict(beta1=1.0), "beta1"), (dict(beta1=1.5), "beta1"),
    (dict(beta2=-0.1), "beta2"), (dict(beta2=float("nan")), "beta2"), (dict(beta2=1.0), "beta2"),
])
def test_adam_descriptor_refusals_name_the_member(kw, name):
    _l = _lib()
    rc, msg = _backward(_l, adam=_adam(_l, **kw))
    assert rc == ERR_INVALID_ARG, (kw, rc)
    assert re.search(r"adam->" + name + r"\b", msg), (kw, msg)


# ---------------------------------------------------------------------------------------------------- trainer.Exposure
def test_exposure_state_round_trips():
    from gaussian_lic_amd import trainer
    ex = trainer.Exposure(3, "cpu", lr=0.02, betas=(0.8, 0.99), eps=1e-6)
    assert tuple(ex.params.shape) == (3, 3, 4) and ex.steps.dtype == torch.int32 and tuple(ex.grad.shape) == (3, 4)
    for i in range(3):
        assert torch.equal(ex.matrix(i), torch.eye(3, 4))
    g = torch.Generator().manual_seed(0)
    ex.params.copy_(torch.randn(3, 3, 4, generator=g)); ex.m.copy_(torch.randn(3, 3, 4, generator=g)); ex.v.copy_(torch.rand(3, 3, 4, generator=g))
    ex.steps.copy_(torch.tensor([4, 0, 9], dtype=torch.int32))
    state = ex.state_dict()
    ex.params.zero_()   # (the state holds copies)
    other = trainer.Exposure(3, "cpu")
    other.load_state_dict(state)
    for a, b in ((other.params, state["params"]), (other.m, state["m"]), (other.v, state["v"]), (other.steps, state["steps"])):
        assert torch.equal(a, b)
    assert (other.lr, other.betas, other.eps) == (0.02, (0.8, 0.99), 1e-6)
    assert torch.equal(other.matrix(2), state["params"][2]) and other.matrix(2).data_ptr() == other.params[2].data_ptr()
    other.reset(2)
    assert torch.equal(other.matrix(2), torch.eye(3, 4)) and int(other.steps[2]) == 0 and not other.m[2].any() and not other.v[2].any()
    assert torch.equal(other.params[0], state["params"][0]) and int(other.steps[0]) == 4
    other.reset()
    assert torch.equal(other.params, torch.eye(3, 4).expand(3, 3, 4)) and not other.steps.any()
    with pytest.raises(ValueError):
        trainer.Exposure(2, "cpu").load_state_dict(state)
    with pytest.raises(IndexError):
        other.matrix(3)
    with pytest.raises(ValueError):
        trainer.Exposure(0, "cpu")
    with pytest.raises(ValueError):
        trainer.Exposure(1, "cpu", betas=(1.0, 0.999))


def test_exposure_adam_step_in_torch_ops_is_the_reference_rule():
    """Exposure.adam_step (the autograd training_step's update) on CPU tensors against the float64 rule."""
    from gaussian_lic_amd import trainer
    ex = trainer.Exposure(2, "cpu")
    rng = np.random.default_rng(9)
    p, m, v, t = ex.params[1].numpy().astype(np.float64), np.zeros((3, 4)), np.zeros((3, 4)), 0
    for _ in range(3):
        g = (rng.standard_normal((3, 4)) * 1e-2).astype(np.float32)
        ex.adam_step(1, torch.from_numpy(g))
        p, m, v, t = ref.adam64(p, m, v, t, g, ex.lr, *ex.betas, ex.eps)
        np.testing.assert_allclose(ex.params[1].numpy(), p, rtol=2e-6, atol=1e-7)
    assert ex.steps.tolist() == [0, 3] and torch.equal(ex.params[0], torch.eye(3, 4))


def test_steps_refuse_a_foreign_exposure_before_any_launch():
    from gaussian_lic_amd import trainer
    for fn in (trainer.training_step, trainer.training_step_fused, trainer.pose_gradient, trainer.training_step_with_pose):
        with pytest.raises(ValueError, match="trainer.Exposure"):
            fn(None, None, None, None, exposure=torch.eye(3, 4))
        with pytest.raises(IndexError):
            fn(None, None, None, None, exposure=trainer.Exposure(2, "cpu"), view=2)
