"""-m gpu: the calibration a pose set's views share — gslic_pose_step_shared / gslic_pose_calibrate_rows on designed sets and made-up camera
gradients against the float64 restatement of their rule (tests/pose_shared_ref.py) and, where the rule is gslic_pose_step's, against that kernel
on bits, with guard words around every array; and trainer.PoseSet(shared=True) through pose_gradient, training_step_with_pose, GraphedStep (eager
and captured) and the C++ host.

The margins are those tests/test_pose_set_gpu.py holds gslic_pose_step to against pose_ref (STATE_MARGIN for the state, GRAD_MARGIN for the
gradient, each relative to the array's largest magnitude); they are imported from there, not restated.  Every test prints its figures before it
asserts."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pose_ref as ref
import pose_shared_ref as sref
from gpu_helpers import assert_same_state, bits, gpu, guarded, guards_intact, model_state, scene_model
from test_pose_set_gpu import GRAD_MARGIN, STATE_MARGIN
from test_pose_shared_cpu import run_argument_cases

pytestmark = pytest.mark.gpu

W_, H_ = 96, 64
ROW = ("view", "proj", "campos")
SHARED = ("sm", "sv", "ssteps", "X", "tau")
NAMES = ROW + ("m", "v", "steps", "projection", "grad", "twist") + SHARED + ("shared_grad",)
SIZES = (1, 3, 64, 65, 257, 1000)       # the edges of a lane, a wave and the workgroup's stride of 256 rows
# series and closed branch in one call: theta_x ~ sqrt(3) lr_rot = 3.5e-5 is under GSLIC_POSE_SERIES_THETA = 1e-4; the first Adam step moves tau by
# about lr_time = 1e-3, so a row with an angular twist of 1e-2 rad/s stays under it and one of 1 .. 300 rad/s is far above it
RATES = dict(lr_trans=1e-3, lr_rot=2e-5, lr_time=1e-3)


def _camera(view=None):
    from gaussian_lic_amd.camera import synthetic_camera
    return synthetic_camera(W_, H_, view)


@functools.lru_cache(maxsize=None)
def _designed(n):
    """n rows and twists, the same for every n on the rows they share: the four se3 poses of the synthetic camera moved by seeded left increments
    (float32 arrays recomposed from a float64 pose, as a host loads them); row j's angular twist is 1e-2 (j % 3 == 0: the series branch under
    RATES), else of the order 10^(j % 3 - 1), thirty times that where j % 7 == 3; the twist of every row with j % 5 == 4 is zero."""
    rng = np.random.default_rng(77)
    base = [ref.mat(_camera(v).world_view_transform.reshape(16)) for v in ("se3_a", "se3_b", "se3_c", "se3_d")]
    projection = np.asarray(_camera().projection_matrix, np.float64).reshape(16)
    view, proj, campos, twist = (np.empty((n, k), np.float32) for k in (16, 16, 3, 6))
    for j in range(n):
        d = rng.normal(size=6) * np.r_[[0.2] * 3, [0.1] * 3]
        xi = rng.normal(size=6)
        xi[3:] *= 1e-2 if j % 3 == 0 else (10.0 ** (j % 3 - 1)) * (1.0 + 29.0 * (j % 7 == 3))
        if j % 5 == 4:
            xi[:] = 0.0
        view[j], proj[j], campos[j] = ref.recompose(ref.retract(ref.flat(base[j % 4]), d), projection)
        twist[j] = xi
    return view, proj, campos, twist


class Guarded:
    """A shared PoseSet of n designed rows whose device arrays each sit between two runs of guard words."""

    def __init__(self, n, **kw):
        from gaussian_lic_amd import trainer
        self.ps = ps = trainer.PoseSet(n, _camera(), gpu(), shared=True, **kw)
        view, proj, campos, twist = _designed(n)
        for name, a in (("view", view), ("proj", proj), ("campos", campos), ("twist", twist)):
            getattr(ps, name).copy_(torch.from_numpy(a))
        self.bufs = {}
        for name in NAMES:
            t = getattr(ps, name)
            buf, words = guarded(t.numel(), dtype=t.dtype)
            words.copy_(t.reshape(-1))
            setattr(ps, name, words.view(t.shape))
            self.bufs[name] = (buf, t.numel())

    def intact(self):
        return all(guards_intact(buf, n) for buf, n in self.bufs.values())

    def snapshot(self):
        return {k: getattr(self.ps, k).clone() for k in NAMES}

    def host(self):
        """The set on the host as pose_shared_ref takes it (float32 values held in float64)."""
        ps = self.ps
        f = lambda t: t.cpu().numpy().astype(np.float64)
        return dict(view=f(ps.view), proj=f(ps.proj), campos=f(ps.campos), twist=f(ps.twist), sm=f(ps.sm), sv=f(ps.sv), ssteps=int(ps.ssteps[0]),
                    X=f(ps.X).reshape(3, 4), tau=float(ps.tau[0]))


def _grads(seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return tuple((rng.normal(size=n) * scale).astype(np.float32) for n in (16, 16, 3))


def _dev(grads):
    return tuple(torch.from_numpy(np.ascontiguousarray(g)).to(gpu()) for g in grads)


def _gap(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


def _state_gap(got, want):
    """Largest gap over the rows' three arrays (row by row, as the per-view test measures), the moments, X and tau."""
    worst = 0.0
    for k in ROW:
        num = np.abs(got[k] - want[k]).max(axis=1)
        worst = max(worst, float((num / np.maximum(np.abs(want[k]).max(axis=1), 1e-30)).max()))
    for k in ("sm", "sv", "X"):
        worst = max(worst, _gap(got[k], want[k]))
    return max(worst, abs(got["tau"] - want["tau"]) / max(abs(want["tau"]), 1e-30))


def _same(a, b, names):
    for k in names:
        assert torch.equal(bits(a[k]), bits(b[k])), k


def _call(ps, word, grads, skip=None):
    """gslic_pose_step_shared on a raw device word (any value) and skip word."""
    from gaussian_lic_amd import _lib
    dv, dp, dc = grads
    d = ps._shared_descriptor(word, skip)
    _lib.check(_lib.lib().gslic_pose_step_shared(ctypes.byref(d), _lib.ptr(dv), _lib.ptr(dp), _lib.ptr(dc), _lib.ptr(ps.shared_grad),
                                                 _lib.current_stream_ptr()))


# ------------------------------------------------------------------------------------------------ pinned to gslic_pose_step
@pytest.mark.parametrize("rates", [dict(lr_trans=1e-3, lr_rot=2e-5), dict(lr_trans=1e-2, lr_rot=0.3)], ids=["series", "closed"])
def test_one_view_and_lr_time_0_is_gslic_pose_step_on_bits(rates):
    """V = 1, lr_time = 0: view, proj, campos and the first six moments equal gslic_pose_step's on a copy of the set, with a twist that is not zero
    (d_tau is a signed zero, so d_x + d_tau xi is d_x).  The same rule: no allowance.  Three steps, compared after each."""
    g = Guarded(1, lr_time=0.0, **rates)
    ps = g.ps
    ps.twist.copy_(torch.tensor([[0.3, -1.0, 2.0, 0.5, -0.25, 4.0]]))
    per_view = ps.clone()
    for k in range(3):
        grads = _dev(_grads(300 + k, 10.0 ** (k - 1)))
        ps.shared_adam_step(0, grads)
        per_view.adam_step(0, grads)
        for name in ROW:
            assert torch.equal(bits(getattr(ps, name)), bits(getattr(per_view, name))), (k, name)
        assert torch.equal(bits(ps.sm[:6]), bits(per_view.m[0])) and torch.equal(bits(ps.sv[:6]), bits(per_view.v[0])), k
        assert torch.equal(bits(ps.shared_grad[:6]), bits(per_view.grad)) and int(ps.ssteps[0]) == int(per_view.steps[0]) == k + 1
    assert float(ps.tau[0]) == 0.0 and bool(ps.sm[6] != 0) and bool((ps.m == 0).all()) and int(ps.steps[0]) == 0   # the per-view state is not touched
    assert not torch.equal(ps.view.cpu(), torch.from_numpy(_designed(1)[0])) and g.intact()                         # the row went somewhere


# ------------------------------------------------------------------------------------------------ against the float64 rule
def _run_against_ref(n, views, scale=1.0):
    g = Guarded(n, **RATES)
    ps = g.ps
    want = g.host()
    proj64 = ps.projection.cpu().numpy().astype(np.float64)
    state_gap = grad_gap = 0.0
    thetas = []
    for k, view in enumerate(views):
        grads = _grads(500 + 7 * n + k, scale)
        before = want
        ps.shared_adam_step(view, _dev(grads))
        want, g7 = sref.step(want, proj64, grads, view, RATES["lr_trans"], RATES["lr_rot"], RATES["lr_time"])
        if k == 0:
            delta, *_ = sref.adam7(g7, before["sm"], before["sv"], before["ssteps"], RATES["lr_trans"], RATES["lr_rot"], RATES["lr_time"])
            thetas = np.linalg.norm(delta[3:6] + delta[6] * before["twist"][:, 3:], axis=1)
        got = g.host()
        assert got["ssteps"] == want["ssteps"] == k + 1
        grad_gap = max(grad_gap, _gap(ps.shared_grad.cpu().numpy(), g7))
        state_gap = max(state_gap, _state_gap(got, want))
        assert all(np.isfinite(got[a]).all() for a in ROW + ("sm", "sv", "X"))
    assert g.intact()
    return state_gap, grad_gap, thetas, g


@pytest.mark.parametrize("n", SIZES)
def test_kernel_against_the_float64_rule(n):
    """Two steps with row 0's gradient and one with row V - 1's (another start: V = 1 has only row 0), twists and lr_time != 0; theta on both sides
    of GSLIC_POSE_SERIES_THETA among the rows of the first call (V >= 3)."""
    worst_state = worst_grad = 0.0
    for views, scale in (((0, 0), 1.0), ((n - 1,), 1e-2)):
        s, gr, thetas, _g = _run_against_ref(n, views, scale)
        print(f"shared step V={n} views {views} scale {scale:g}: state gap {s:.3e} grad gap {gr:.3e}, theta of the first call "
              f"{thetas.min():.3e} .. {thetas.max():.3e}")
        worst_state, worst_grad = max(worst_state, s), max(worst_grad, gr)
        if n >= 3 and views[0] == 0:   # (row V - 1 may be one of the zero-twist rows: then g_tau and d_tau are zero and every row takes d_x)
            assert 0 < (thetas < ref.SERIES_THETA).sum() < n, "both branches of the exp in one call"
    print(f"shared step V={n}: largest state gap {worst_state:.3e} (bar {STATE_MARGIN:.3e}), largest grad gap {worst_grad:.3e} (bar {GRAD_MARGIN:.3e})")
    assert worst_state <= STATE_MARGIN and worst_grad <= GRAD_MARGIN


@pytest.mark.parametrize("n", [3, 257])
def test_a_view_word_outside_the_set_writes_nothing(n):
    grads = _dev(_grads(9))
    for bad in (-1, n, 1 << 30):
        g = Guarded(n, **RATES)
        g.ps.shared_grad.fill_(-3.0)
        before = g.snapshot()
        _call(g.ps, torch.tensor([bad], dtype=torch.int32, device=gpu()), grads)
        _same(g.snapshot(), before, NAMES)
        assert g.intact(), bad


def test_rows_do_not_depend_on_V():
    """The first three rows of a V = 257 call equal the V = 3 call on bits (same rows, same twists, same stepped view), and so do the shared state
    and the gradient; two runs of one call give the same bits."""
    out = []
    for n in (3, 257, 257):
        g = Guarded(n, **RATES)
        for k in range(2):
            g.ps.shared_adam_step(1, _dev(_grads(40 + k)))
        out.append(g.snapshot())
        assert g.intact()
    small, big, again = out
    for k in ROW + ("twist",):
        assert torch.equal(bits(big[k][:3]), bits(small[k])), k
    _same(big, small, SHARED + ("shared_grad",))
    _same(big, again, NAMES)
    assert not torch.equal(big["view"][3:], Guarded(257, **RATES).ps.view[3:])       # the rows behind moved as well


# ------------------------------------------------------------------------------------------------ no-ops on bits
@pytest.mark.parametrize("n", [3, 65])
def test_no_ops_on_bits(n):
    grads = _grads(11)
    dg = _dev(grads)
    everything_but_grad = tuple(k for k in NAMES if k != "shared_grad")
    # the skip word (one of the bits 1 | 2 | 8 | 16): nothing but grad_out
    for word in (1, 2, 8, 16, 4 | 16):
        g = Guarded(n, **RATES)
        ps, before = g.ps, g.snapshot()
        ps.shared_grad.fill_(-3.0)
        _call(ps, ps._views[1:2], dg, torch.tensor([word], dtype=torch.int32, device=gpu()))
        _same(g.snapshot(), before, everything_but_grad)
        want = sref.gradient(g.host(), ps.projection.cpu().numpy().astype(np.float64), grads, 1)
        assert _gap(ps.shared_grad.cpu().numpy(), want) <= GRAD_MARGIN and g.intact(), word
    for word in (0, 4):                                                               # no skip: the set steps
        g = Guarded(n, **RATES)
        before = g.snapshot()
        _call(g.ps, g.ps._views[1:2], dg, torch.tensor([word], dtype=torch.int32, device=gpu()))
        assert int(g.ps.ssteps[0]) == 1 and not torch.equal(g.ps.view, before["view"]) and g.intact(), word
    # a NaN or an inf in the gradient: only grad_out, ssteps stays
    for bad in (float("nan"), float("inf")):
        g = Guarded(n, **RATES)
        before = g.snapshot()
        poisoned = tuple(a.copy() for a in grads)
        poisoned[0][13] = bad
        g.ps.shared_adam_step(1, _dev(poisoned))
        _same(g.snapshot(), before, everything_but_grad)
        assert not bool(torch.isfinite(g.ps.shared_grad).all()) and g.intact()
    # g finite and g_tau not (an infinite twist coordinate on the stepped row): the same
    g = Guarded(n, **RATES)
    g.ps.twist[1, 0] = float("inf")
    before = g.snapshot()
    g.ps.shared_adam_step(1, dg)
    _same(g.snapshot(), before, everything_but_grad)
    assert bool(torch.isfinite(g.ps.shared_grad[:6]).all()) and not bool(torch.isfinite(g.ps.shared_grad[6])) and g.intact()
    # all three rates zero: moments and count move, no pose, X or tau bit does
    g = Guarded(n, lr_trans=0.0, lr_rot=0.0, lr_time=0.0)
    before = g.snapshot()
    g.ps.shared_adam_step(1, dg)
    after = g.snapshot()
    _same(after, before, ROW + ("X", "tau", "twist", "m", "v", "steps", "projection", "grad"))
    assert int(after["ssteps"][0]) == 1 and bool((after["sm"] != 0).all()) and bool((after["sv"] > 0).all()) and g.intact()
    # d_x = 0 and d_tau != 0: a row of zero twist keeps its bits while its neighbours move; X keeps its bits, tau moves
    g = Guarded(n, lr_trans=0.0, lr_rot=0.0, lr_time=1e-3)
    g.ps.twist[2] = 0.0
    before = g.snapshot()
    g.ps.shared_adam_step(1, dg)
    after = g.snapshot()
    zero = [j for j in range(n) if not bool(before["twist"][j].any())]
    moving = [j for j in range(n) if j not in zero]
    assert 2 in zero and moving
    for k in ROW:
        assert torch.equal(bits(after[k][zero]), bits(before[k][zero])), k
        assert all(not torch.equal(after[k][j], before[k][j]) for j in moving), k
    assert torch.equal(bits(after["X"]), bits(before["X"])) and float(after["tau"][0]) != 0.0 and g.intact()
    # a row whose d_j is not finite (an infinite twist on another row than the stepped one) keeps its bits
    g = Guarded(n, **RATES)
    g.ps.twist[0, 4] = float("inf")
    before = g.snapshot()
    g.ps.shared_adam_step(1, dg)
    after = g.snapshot()
    for k in ROW:
        assert torch.equal(bits(after[k][0]), bits(before[k][0])) and not torch.equal(after[k][1], before[k][1]), k
    assert bool(torch.isfinite(after["view"]).all()) and g.intact()


# ------------------------------------------------------------------------------------------------ gslic_pose_calibrate_rows
def _loaded_set(**kw):
    """Three rows loaded from three cameras (the host's route), between guard words."""
    from gaussian_lic_amd import trainer
    cams = [_camera(v) for v in ("se3_c", "se3_d", 2)]
    ps = trainer.PoseSet(3, cams[0], gpu(), shared=True, **kw)
    for i in (1, 2):
        ps.load(i, cams[i])
    return ps, cams


def test_calibrate_rows_at_the_identity_keeps_the_matrix():
    """X = I, tau = 0: rows 1 and 2 within the Gram-Schmidt rounding of a float32 matrix, row 0 on bits.
    Observed on one MI355X: 9.934e-08 of the array's largest magnitude (the bar is STATE_MARGIN, what one step is held to)."""
    ps, cams = _loaded_set()
    ps.twist.copy_(torch.from_numpy(_designed(3)[3]))
    before = {k: getattr(ps, k).clone() for k in ROW}
    ps.calibrate_rows(1, 2)
    gap = max(_gap(getattr(ps, k)[j].cpu().numpy(), before[k][j].cpu().numpy()) for k in ROW for j in (1, 2))
    print(f"calibrate_rows at X = I, tau = 0: largest gap to the loaded row {gap:.3e} (bar {STATE_MARGIN:.3e})")
    assert gap <= STATE_MARGIN
    for k in ROW:
        assert torch.equal(bits(getattr(ps, k)[0]), bits(before[k][0])), k


def test_a_row_loaded_calibrated_matches_the_row_that_was_moved():
    """K = 4 extrinsic-only steps (lr_time = 0), then row 1 is loaded again from its camera with calibrated=True: it matches the row the steps
    moved, at the margin one step is held to against the float64 rule; the other rows keep their bits."""
    ps, cams = _loaded_set(lr_trans=5e-3, lr_rot=1e-2, lr_time=0.0)
    ps.twist.copy_(torch.from_numpy(_designed(3)[3]))
    for k in range(4):
        ps.shared_adam_step(k % 3, _dev(_grads(60 + k)))
    moved = {k: getattr(ps, k).clone() for k in ROW}
    ps.load(1, cams[1], calibrated=True)
    gap = max(_gap(getattr(ps, k)[1].cpu().numpy(), moved[k][1].cpu().numpy()) for k in ROW)
    away = _gap(ps.view[1].cpu().numpy(), cams[1].world_view_transform.reshape(16))
    print(f"load(calibrated=True) after 4 steps: gap to the moved row {gap:.3e} (bar {STATE_MARGIN:.3e}); the row is {away:.3e} from its camera")
    assert gap <= STATE_MARGIN and away > 1e-3
    for k in ROW:
        assert torch.equal(bits(getattr(ps, k)[[0, 2]]), bits(moved[k][[0, 2]])), k
    assert ps.steps.tolist() == [0, 0, 0] and int(ps.ssteps[0]) == 4
    X = ps.extrinsic()
    assert abs(np.linalg.det(X[:3, :3]) - 1.0) < 1e-5 and ps.time_offset() == 0.0


def test_calibrate_rows_against_the_float64_rule():
    """257 designed rows, an X and a tau that four steps produced, rows [1, 257) calibrated (two workgroups, the second partial): against
    pose_shared_ref.calibrate_rows; row 0 and the guard words untouched."""
    g = Guarded(257, lr_trans=5e-3, lr_rot=1e-2, lr_time=1e-3)
    ps = g.ps
    for k in range(4):
        ps.shared_adam_step(k, _dev(_grads(80 + k)))
    ps.twist[7, 1] = float("inf")                                                     # a row whose tau xi is not finite keeps its bits
    before = g.snapshot()
    want = sref.calibrate_rows(g.host(), ps.projection.cpu().numpy().astype(np.float64), 1, 256)
    ps.calibrate_rows(1, 256)
    got = g.host()
    gap = 0.0
    for k in ROW:
        num = np.abs(got[k] - want[k]).max(axis=1)
        gap = max(gap, float((num / np.maximum(np.abs(want[k]).max(axis=1), 1e-30)).max()))
    print(f"calibrate_rows on 256 rows: largest gap to the float64 rule {gap:.3e} (bar {STATE_MARGIN:.3e}), tau {got['tau']:.3e}")
    assert gap <= STATE_MARGIN and got["tau"] != 0.0
    after = g.snapshot()
    for k in ROW:
        assert torch.equal(bits(after[k][[0, 7]]), bits(before[k][[0, 7]])) and not torch.equal(after[k][1], before[k][1]), k
    _same(after, before, tuple(k for k in NAMES if k not in ROW))
    assert g.intact()


def test_argument_checks():
    assert run_argument_cases() > 0                                                   # every GSLIC_ERR_INVALID_ARG case, each naming its argument


# ------------------------------------------------------------------------------------------------ the paths
POSE_KEYS = ("view", "proj", "campos", "m", "v", "steps", "grad", "twist") + SHARED + ("shared_grad",)
SEQUENCE = (1, 0, 2, 1, 2, 0)


@functools.lru_cache(maxsize=None)
def _scene():
    """The smallest scene of gpu_helpers.scene_model ("a": 96 Gaussians, 40 x 24) with three views."""
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import gt_image
    import contribution_ref as cr
    _raw, W, H = cr.scene("a")
    cams = [synthetic_camera(W, H, v).to_device(gpu()) for v in (None, 3, 4)]
    gts = [gt_image(H, W, seed=30 + k).to(gpu()) for k in range(3)]
    return cams, gts, torch.zeros(3, device=gpu())


def _model():
    m, _cam = scene_model("a")
    m.training_setup()
    return m


def _shared_set(cams, **kw):
    from gaussian_lic_amd import trainer
    kw = dict(dict(lr_trans=2e-3, lr_rot=1e-3, lr_time=5e-4), **kw)
    ps = trainer.PoseSet(3, cams[0], gpu(), shared=True, **kw)
    rng = np.random.default_rng(4)
    for i in range(3):
        ps.load(i, cams[i], twist=rng.normal(size=6) * 0.5)
    return ps


def _pose_state(ps):
    return {k: getattr(ps, k).cpu().clone() for k in POSE_KEYS}


def _same_set(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), k


def _loop(adam_in_backward, sequence=SEQUENCE, **kw):
    from gaussian_lic_amd import loss, trainer
    cams, gts, bg = _scene()
    model, ps, fl = _model(), _shared_set(cams), loss.FusedLoss(0.2)
    terms = []
    for k in sequence:
        t, _vis, g = trainer.training_step_with_pose(model, cams[0], gts[k], bg, fused_loss=fl, poses=ps, view=k, shared=True,
                                                     adam_in_backward=adam_in_backward, **kw)
        assert g is ps.shared_grad
        terms.append(t.clone())
    torch.cuda.synchronize()
    return model_state(model), _pose_state(ps), torch.stack(terms).cpu()


def test_training_step_with_pose_shared_with_and_without_adam_in_backward():
    old, new = _loop(False), _loop(True)
    assert_same_state(old[0], new[0])
    _same_set(old[1], new[1])
    assert torch.equal(bits(old[2]), bits(new[2]))
    start = _pose_state(_shared_set(_scene()[0]))
    assert new[1]["ssteps"].tolist() == [len(SEQUENCE)] and new[1]["steps"].tolist() == [0, 0, 0] and float(new[1]["tau"][0]) != 0.0
    assert all(not torch.equal(new[1]["view"][j], start["view"][j]) for j in range(3)) and not torch.equal(new[1]["X"], start["X"])
    assert bool(new[1]["shared_grad"].abs().min() > 0) and not bool(new[1]["m"].any())


def test_training_step_with_pose_shared_combines_with_weight_depth_and_exposure():
    from gaussian_lic_amd import trainer
    cams, gts, bg = _scene()
    H, W = gts[0].shape[1:]
    kw = lambda: dict(weight=torch.rand(H, W, generator=torch.Generator().manual_seed(3)).to(gpu()),
                      gt_depth=(1.0 + 4.0 * torch.rand(H, W, generator=torch.Generator().manual_seed(5))).to(gpu()), lambda_depth=0.5,
                      depth_weight=(2.0 * torch.rand(H, W, generator=torch.Generator().manual_seed(6))).to(gpu()), depth_huber=0.05,
                      exposure=trainer.Exposure(3, gpu(), lr=0.01))
    old, new = _loop(False, SEQUENCE[:3], **kw()), _loop(True, SEQUENCE[:3], **kw())
    assert_same_state(old[0], new[0])
    _same_set(old[1], new[1])
    assert torch.equal(bits(old[2]), bits(new[2])) and new[2].shape == (3, 3) and new[1]["ssteps"].tolist() == [3]


def _graphed(use_graph):
    """A GraphedStep(train_pose="shared") over SEQUENCE whose first step is forced not to fit (cap_R half the view's instance count) and is
    repeated by check(): (map, set, terms of the steps that fitted when issued)."""
    from gaussian_lic_amd import trainer
    cams, gts, bg = _scene()
    model, ps = _model(), _shared_set(cams)
    with torch.no_grad():
        sizing = trainer._RawRaster(model, cams[0], bg, False, pose=ps.pose(SEQUENCE[0]))
        sizing.forward()
        R = int(sizing.state[0])
    assert R > 8
    map0, set0 = model_state(model), _pose_state(ps)
    gs = trainer.GraphedStep(model, cams[0], gts[SEQUENCE[0]], bg, use_graph=use_graph, poses=ps, view=SEQUENCE[0], train_pose="shared", cap_R=R // 2,
                             check_every=0)
    _same_set(_pose_state(ps), set0)                                                  # warm-up and capture passes left the set as it was
    gs.step()
    torch.cuda.synchronize()
    assert_same_state(map0, model_state(model))                                       # the step did not fit: neither map nor set moved
    after = _pose_state(ps)
    _same_set({k: after[k] for k in after if k != "shared_grad"}, {k: set0[k] for k in set0 if k != "shared_grad"})
    assert bool((ps.shared_grad == 0).all())                                          # (its camera gradient is zeros)
    assert gs.check() == 1 and gs.cap_R >= R and ps.ssteps.tolist() == [1]            # repeated: applied exactly once
    terms = [gs.step(gt_image=gts[k], view=k).clone() for k in SEQUENCE[1:]]
    assert gs.check() == 0
    return model_state(model), _pose_state(ps), torch.stack(terms).cpu()


@pytest.mark.parametrize("use_graph", [False], ids=["eager"])
def test_graphed_step_trains_the_shared_calibration_eager(use_graph):
    got, want = _graphed(use_graph), _loop(True)
    assert_same_state(got[0], want[0])
    _same_set(got[1], want[1])
    assert torch.equal(bits(got[2]), bits(want[2][1:])) and got[1]["ssteps"].tolist() == [len(SEQUENCE)]


def test_graphed_step_trains_the_shared_calibration_captured():
    got, want = _graphed(True), _loop(True)
    assert_same_state(got[0], want[0])
    _same_set(got[1], want[1])
    assert torch.equal(bits(got[2]), bits(want[2][1:])) and got[1]["ssteps"].tolist() == [len(SEQUENCE)]


def test_graphed_step_refusals():
    from gaussian_lic_amd import trainer
    cams, gts, bg = _scene()
    model = _model()
    plain = trainer.PoseSet(3, cams[0], gpu())
    with pytest.raises(ValueError, match="built without shared=True"):
        trainer.GraphedStep(model, cams[0], gts[0], bg, poses=plain, view=0, train_pose="shared")
    with pytest.raises(NotImplementedError, match="grad_stats"):
        trainer.GraphedStep(model, cams[0], gts[0], bg, poses=_shared_set(cams), view=0, train_pose="shared", grad_stats=trainer.GradientStats(model))
    # train_pose=True on a shared set is the per-view step as it is: the shared state is not touched
    ps = _shared_set(cams)
    start = _pose_state(ps)
    gs = trainer.GraphedStep(model, cams[0], gts[0], bg, poses=ps, view=0, train_pose=True)
    gs.step(view=1)
    assert gs.check() == 0
    after = _pose_state(ps)
    _same_set({k: after[k] for k in SHARED + ("shared_grad", "twist")}, {k: start[k] for k in SHARED + ("shared_grad", "twist")})
    assert after["steps"].tolist() == [0, 1, 0] and torch.equal(bits(after["view"][[0, 2]]), bits(start["view"][[0, 2]]))


# ------------------------------------------------------------------------------------------------ the C++ host
def test_fused_pose_shared_cpp_host(tmp_path):
    """gslic::PoseSet with shared, FusedStep::step_with_pose(shared) and the pose-set overload of pose_gradient(shared) issue the C-ABI calls of the
    Python host: after four joint steps over three views, one pose step and a calibrated load of row 2, the map, the rows, the shared state, every
    step's terms and gradient are bit-identical.  (twist.f32 and the third target go through fused_check_io's extra float32 arrays.)"""
    import fused_check_io as fio
    from gaussian_lic_amd import loss, trainer
    import contribution_ref as cr
    exe = fio.build("fused_pose_shared")
    iters, rates = 4, dict(lr_trans=2e-3, lr_rot=1e-3, lr_time=5e-4)
    cams, gts, bg = _scene()
    raw, W, H = cr.scene("a")
    ps = _shared_set(cams, **rates)
    twist = ps.twist.cpu().clone()
    d = str(tmp_path)
    fio.write_inputs(d, raw, cams, gt=gts[0], gt2=gts[1], gt3=gts[2], projection=ps.projection, twist=twist)
    fio.run(exe, d, str(cr.P_A), str(W), str(H), "0", str(iters), *(repr(rates[k]) for k in ("lr_trans", "lr_rot", "lr_time")))
    model, fl = _model(), loss.FusedLoss(0.2)
    terms, grads = [], []
    for it in range(iters):
        t, _vis, g = trainer.training_step_with_pose(model, cams[0], gts[it % 3], bg, fused_loss=fl, poses=ps, view=it % 3, shared=True, adam_in_backward=True)
        terms.append(t.clone()); grads.append(g.clone())
    grads.append(trainer.pose_gradient(model, cams[0], gts[1], bg, fused_loss=fl, poses=ps, view=1, do_step=True, shared=True)[0].clone())
    ps.load(2, cams[2], twist=twist[2], calibrated=True)
    torch.cuda.synchronize()
    rd = lambda name: fio.read(d, name, np.int32)
    for name in ROW:
        assert torch.equal(rd(f"pose_{name}.f32"), bits(getattr(ps, name).cpu()).reshape(-1)), name
    for name in ("sm", "sv", "X", "tau"):
        assert torch.equal(rd(f"shared_{name}.f32"), bits(getattr(ps, name).cpu()).reshape(-1)), name
    assert rd("shared_ssteps.i32").tolist() == ps.ssteps.tolist() == [iters + 1]
    assert torch.equal(rd("shared_grads.f32"), bits(torch.stack(grads).cpu()).reshape(-1)) and bool(torch.stack(grads).abs().min() > 0)
    assert torch.equal(rd("terms.f32"), bits(torch.stack(terms).cpu()).reshape(-1))
    rows, state = fio.read_rows(d, 0), model_state(model)
    for name, key in (("xyz", "xyz"), ("scaling", "scaling"), ("rotation", "rotation"), ("opacity", "opacity"), ("features_dc", "dc")):
        assert torch.equal(rows[key], bits(state[name]).reshape(-1)), name
        assert torch.equal(rows["m_" + key], bits(state[name + ".m"]).reshape(-1)) and torch.equal(rows["v_" + key], bits(state[name + ".v"]).reshape(-1)), name


# ------------------------------------------------------------------------------------------------ recovery
RECOVERY = dict(xi=(6e-3, -5e-3, 6e-3, 5e-3, -6e-3, 4e-3), K=24, lr=2e-4)   # 1 cm and 0.5 degrees; 24 steps of at most 2e-4 per coordinate


def _distance(X4, want4):
    """(rotation angle [rad], translation norm [m]) of X relative to `want`."""
    D = X4 @ np.linalg.inv(want4)
    c = (np.trace(D[:3, :3]) - 1.0) / 2.0
    return float(np.arccos(np.clip(c, -1.0, 1.0))), float(np.linalg.norm(D[:3, 3]))


def test_recovery_of_a_common_displacement():
    """Targets rendered from three ground-truth poses; every row displaced by ONE left increment of 0.5 degrees and 1 cm; pose_gradient(do_step=True,
    shared=True) cycled over the views with the map untouched.  X ends nearer to the inverse displacement than it started (the identity), in
    rotation angle and in translation norm — and so does the float64 rule fed the same camera gradients."""
    from gaussian_lic_amd import loss, trainer
    from gaussian_lic_amd.camera import synthetic_camera
    from gpu_helpers import training_model
    from test_pose_set_gpu import H_ as H, W_ as W, _setup
    raw, _cams, _gts, _gtd, bg = _setup(3)
    truth = [synthetic_camera(W, H, v).to_device(gpu()) for v in (None, 3, 4)]
    model = training_model(raw)
    with torch.no_grad():
        targets = [trainer._RawRaster(model, c, bg, False).forward()[0].clone() for c in truth]
    xi, K, lr = np.array(RECOVERY["xi"]), RECOVERY["K"], RECOVERY["lr"]
    ps = trainer.PoseSet(3, truth[0], gpu(), shared=True, lr_trans=lr, lr_rot=lr, lr_time=0.0)
    for i, v in enumerate((None, 3, 4)):
        ps.load(i, synthetic_camera(W, H, v).apply_pose_increment(xi).to_device(gpu()))
    want = np.linalg.inv(ref.se3_exp(xi))
    f64 = lambda t: t.cpu().numpy().astype(np.float64)
    host = sref.new_set(f64(ps.view), f64(ps.proj), f64(ps.campos))
    proj64 = f64(ps.projection)
    start = _distance(ps.extrinsic(), want)
    fl = loss.FusedLoss(0.2)
    state0 = model_state(model)
    losses = []
    for k in range(K):
        i = k % 3
        # the camera gradients of this step, for the float64 rule: the same forward, loss and camera backward ahead of the step
        with torch.no_grad():
            rr = trainer._RawRaster(model, truth[0], bg, False, pose=ps.pose(i))
            image, _d, _r = rr.forward()
            dL, _dd, _t = trainer._fused_losses(loss.FusedLoss(0.2), image, targets[i], None, None, 0.0)
            grads = tuple(t.cpu().numpy() for t in rr.backward(dL, None, camera_grads=True)[9:12])
        host, _g7 = sref.step(host, proj64, grads, i, lr, lr, 0.0)
        g, terms = trainer.pose_gradient(model, truth[0], targets[i], bg, fused_loss=fl, poses=ps, view=i, do_step=True, shared=True)
        assert g is ps.shared_grad
        losses.append(float(fl.value(terms)))
    end = _distance(ps.extrinsic(), want)
    X64 = np.eye(4); X64[:3] = host["X"]
    end64 = _distance(X64, want)
    print(f"recovery: X from the inverse displacement, start {np.degrees(start[0]):.4f} deg {start[1] * 100:.4f} cm -> device "
          f"{np.degrees(end[0]):.4f} deg {end[1] * 100:.4f} cm, float64 rule on the same gradients {np.degrees(end64[0]):.4f} deg "
          f"{end64[1] * 100:.4f} cm; loss {losses[0]:.6e} -> {losses[-1]:.6e}")
    assert_same_state(state0, model_state(model))                                     # the map is untouched
    assert end64[0] < start[0] and end64[1] < start[1]
    assert end[0] < start[0] and end[1] < start[1]
    assert int(ps.ssteps[0]) == K and ps.time_offset() == 0.0
