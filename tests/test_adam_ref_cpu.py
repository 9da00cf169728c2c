"""CPU: the numpy Adam reference of tests/adam_ref.py checked against the float64 C oracle, and the inputs of tests/test_adam_paths_gpu.py checked
for what they must have before a GPU sees them: nothing below 2^-126, and enough structure to tell a wrong kernel from a right one."""
import numpy as np
import pytest
import torch

import adam_cases as ac
from adam_ref import (adam_ref, adam_ref64, adam_wrong_groups_past_eight, adam_wrong_quad_visibility, adam_wrong_tail_skipped, quad_kinds, quad_rows,
                      same_bits, tail_elements)

U = 2.0 ** -24       # unit roundoff of float32


def _differs(a, b):
    return any(not same_bits(x, y).all() for x, y in zip(a, b))


def test_reference_agrees_with_the_float64_oracle(oracle64):
    """adam_ref against oracle64.adam on test_adam_parity's first shape, element by element.  The oracle gets the float32-rounded scalars (what the
    library's float arguments hold), so both sides evaluate the same real function and only adam_ref's own roundings separate them.  With
    u = 2^-24, every float32 operation returning x (1 + d), |d| <= u, and terms of second order in u covered by the slack in the constants:

      m' = fl(fl(b1 m) + fl(c1 g)), c1 = 1 - b1 exact (Sterbenz: b1 in [1/2, 2]).  Each product is off by u of itself and the sum by u of
           itself, which is at most the sum of the magnitudes:  |err m'| <= 2u (|b1 m| + |c1 g|)  <=  4u (|b1 m| + |c1 g|) =: 4u Sm.
      v' = fl(fl(b2 v) + fl(fl(c2 g) g)), c2 = 1 - b2 exact.  One rounding on the first term, two on the second, one on the sum:
           |err v'| <= 3u (|b2 v| + |c2 g g|)  <=  4u (|b2 v| + |c2 g g|) =: 4u Sv.  For v >= 0 nothing cancels: this is 4u relative to v'.
      p' = fl(p + t), t = fl(fl(-lr m') / fl(fl(sqrt(v')) + eps)).  The numerator carries m's error times lr plus its own rounding; the
           denominator d = sqrt(v') + eps carries half of v's relative error (2u), sqrt's rounding and the sum's (4u of d together); the
           quotient adds u:  |err t| <= 6u |t| + 4u lr Sm / d  <=  8u |t| + 4u lr Sm / d,  and the last sum adds u (|p| + |t|):
           |err p'| <= 4u (|p| + 3 |t| + lr Sm / d).
    Invisible rows: identical bits."""
    N, M = 1000, 3
    rng = np.random.default_rng(0)      # test_adam_parity's own draws, in its order
    p, g = rng.standard_normal((N, M)).astype(np.float32), rng.standard_normal((N, M)).astype(np.float32)
    m, v = (0.1 * rng.standard_normal((N, M))).astype(np.float32), (0.01 * rng.random((N, M))).astype(np.float32)
    vis = rng.random(N) < 0.6
    lr, b1, b2, eps = (float(np.float32(x)) for x in (ac.LR, ac.B1, ac.B2, ac.EPS))
    op, om, ov = (x.astype(np.float64) for x in (p, m, v))
    oracle64.adam(op, g.astype(np.float64), om, ov, vis, lr, b1, b2, eps)
    rp, rm, rv, sub = adam_ref(p, g, m, v, vis, **ac.HYPER)
    assert not sub.any()
    p64, g64, m64, v64 = (x.astype(np.float64) for x in (p, g, m, v))
    Sm = np.abs(b1 * m64) + np.abs((1.0 - b1) * g64)
    Sv = np.abs(b2 * v64) + np.abs((1.0 - b2) * g64 * g64)
    d = np.sqrt(ov) + eps
    t = np.abs(lr * om / d)
    w = vis[:, None]
    assert (np.abs(rm - om) <= 4 * U * Sm)[vis].all() and (np.abs(rm - om)[vis] > 0).any()
    assert (np.abs(rv - ov) <= 4 * U * Sv)[vis].all()
    assert (np.abs(rp - op) <= 4 * U * (np.abs(p64) + 3 * t + lr * Sm / d))[vis].all()
    for got, start in ((rp, p), (rm, m), (rv, v)):
        assert same_bits(got, start)[~vis].all() and not same_bits(got, start)[vis].all()
    # the float64 twin is the oracle's own sequence: at most the last bit of a double apart (the compiler may order the commutative operands differently)
    tp, tm, tv = adam_ref64(p, g, m, v, vis, **ac.HYPER)
    for got, ref in ((tp, op), (tm, om), (tv, ov)):
        assert (np.abs(got - ref) <= 2.0 ** -52 * np.abs(ref)).all()
    assert (w | (tp == p64)).all()


def _no_subnormals(p, g, m, v, vis, lr=ac.LR):
    sub = adam_ref(p, g, m, v, vis, lr, ac.B1, ac.B2, ac.EPS)[3]
    assert int(sub.sum()) == 0


def test_no_input_of_the_gpu_cases_reaches_below_the_normal_range():
    """The `subnormal` share is 0 for every generator of tests/adam_cases.py, so no GPU comparison depends on the fp32 denormal mode.  (The
    all-visible mask covers every mask a case may use.)"""
    for N, M in ac.A_SHAPES + ac.B_SHAPES + [(ac.C_N, w) for w in ac.C_WIDTHS]:
        _no_subnormals(*ac.tensors(N, M, seed=N * 100 + M), np.ones(N, np.uint8))
    for (p, g, m, v, lr) in ac.e_groups():
        _no_subnormals(p, g, m, v, np.ones(ac.E_N, np.uint8), lr)
    for scale in ac.F_SCALES:
        _no_subnormals(*ac.f_tensors(scale), np.ones(ac.F_SHAPE[0], np.uint8))
    _no_subnormals(*ac.f_tensors(1.0, nonfinite=True), np.ones(ac.F_SHAPE[0], np.uint8))


@pytest.mark.parametrize("N,M", ac.D_SHAPES)
def test_no_input_of_the_large_case_reaches_below_the_normal_range(N, M):
    assert 8192 * 256 * 4 < N * M < 8192 * 256 * 4 + 8192      # a second trip for the first few blocks only
    assert ((N * M) % 4 != 0) == (N == 186501)
    _no_subnormals(*ac.tensors(N, M, seed=N * 100 + M), np.ones(N, np.uint8))


def _model_inputs(deg):
    from conftest import make_scene
    raw = make_scene("random", ac.MODEL_P, 96, 64, deg, 71)[0]
    widths = ac.GROUP_WIDTHS[deg]
    names = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")
    params = [raw[n].reshape(ac.MODEL_P, -1).numpy().astype(np.float32) for n in names]
    assert tuple(x.shape[1] for x in params) == widths
    return raw, params, ac.moments(ac.MODEL_P, widths, 72)


@pytest.mark.parametrize("deg", [3, 0])
def test_no_input_of_the_model_cases_reaches_below_the_normal_range(deg):
    """Cases (g) - (i): the model's parameters, the seeded moments, the small gradients, and the SH rows of the hand-built payloads (here from
    the plain-torch rebuild of tests/sh_rank1_ref.py, a few ulps from the rows the library's kernel gives the GPU test, which checks those again)."""
    import sh_rank1_ref
    raw, params, mom = _model_inputs(deg)
    P = ac.MODEL_P
    lrs = [1.6e-4, 2.5e-3, 2.5e-3 / 20, 5e-2, 5e-3, 1e-3]
    everything = np.ones(P, np.uint8)
    for i, g in zip((0, 3, 4, 5), ac.small_grads(P, 73)):
        _no_subnormals(params[i], g, *mom[i], everything, lrs[i])
    for n_views in (1, 3):
        rgb, campos, masks = ac.view_payload(P, n_views, 74 + n_views)
        dc, sh = sh_rank1_ref.rows_from_rgb(raw["xyz"].float(), torch.from_numpy(campos), torch.from_numpy(rgb), deg, ac.GROUP_WIDTHS[deg][2] // 3)
        seen = masks.max(0)
        _no_subnormals(params[1], dc.reshape(P, 3).numpy(), *mom[1], seen, lrs[1])
        if deg:
            _no_subnormals(params[2], sh.reshape(P, 45).numpy(), *mom[2], seen, lrs[2])


@pytest.mark.parametrize("M", ac.C_WIDTHS)
def test_quad_bookkeeping_and_visibility_patterns(M):
    """quad_rows / quad_kinds against a scalar-by-scalar count, and what section (c) needs from each pattern: mixed quads for every width but 1,
    and for "runs" a quad the kernel skips without traffic right next to a mixed one."""
    N = ac.C_N
    rows = quad_rows(N, M)
    assert rows.shape == ((N * M) // 4, 4)
    for q in (0, 1, rows.shape[0] // 2, rows.shape[0] - 1):
        assert [int(r) for r in rows[q]] == [(4 * q + k) // M for k in range(4)]
    assert len(tail_elements(N, M)) == (N * M) % 4 and (N * M) % 4 != 0
    assert (tail_elements(N, M) // M == N - 1).all() or M < 4        # the tail sits in the last row (M = 1, 3: in the last rows)
    for name in ac.C_PATTERNS:
        vis = ac.vis_pattern(name, N)
        assert vis.shape == (N,) and vis.dtype == np.uint8
        kinds = quad_kinds(vis, M)
        want = np.array([{0: 0, 4: 1}.get(sum(int(vis[(4 * q + k) // M] != 0) for k in range(4)), 2) for q in range(len(kinds))], np.int8)
        assert (kinds == want).all()
        mixed, skipped = int((kinds == 2).sum()), int((kinds == 0).sum())
        if name == "none":
            assert int(vis.sum()) == 0 and skipped == len(kinds)
        elif name == "all":
            assert mixed == 0 and skipped == 0
        elif name in ("row0", "rowlast"):
            assert int((vis != 0).sum()) == 1 and vis[0 if name == "row0" else N - 1] == 1
            assert mixed >= (1 if M % 4 else 0) or name == "rowlast"     # (the last row may end in the tail)
        elif M == 1 and name == "0101":
            assert mixed == len(kinds)
        elif name == "bytes":
            assert set(np.unique(vis)) == {0, 2, 255} and (mixed > 0 or M == 4)
        else:
            assert mixed > 0
        if name == "runs":
            assert skipped > 0 and ((kinds[:-1] == 0) & (kinds[1:] == 2)).any() and ((kinds[:-1] == 2) & (kinds[1:] == 0)).any()
            inv = np.flatnonzero(vis == 0)
            runs = np.split(inv, np.flatnonzero(np.diff(inv) != 1) + 1)
            assert min(len(r) for r in runs[:-1]) >= 4


def test_inputs_tell_a_wrong_kernel_from_a_right_one():
    """The CPU half of "each new branch is exercised": on the GPU cases' own inputs the reference differs from an evaluation that takes the whole
    quad's visibility from its first scalar's row (c: exactly the patterns with a mixed quad), skips the scalar tail (b, d), or leaves the
    groups past the eighth alone (e)."""
    for M in ac.C_WIDTHS:
        t = ac.tensors(ac.C_N, M, seed=ac.C_N * 100 + M)
        for name in ac.C_PATTERNS:
            vis = ac.vis_pattern(name, ac.C_N)
            mixed = int((quad_kinds(vis, M) == 2).sum())
            ref = adam_ref(*t, vis, **ac.HYPER)[:3]
            assert _differs(ref, adam_wrong_quad_visibility(*t, vis, **ac.HYPER)) == (mixed > 0), (M, name)
    for N, M in ac.B_SHAPES + ac.D_SHAPES[1:]:
        t = ac.tensors(N, M, seed=N * 100 + M)
        vis = ac.mask(N, seed=N + M)
        # ((3, 4) and (9, 64) have no tail: those cases run whole quads only)
        assert _differs(adam_ref(*t, vis, **ac.HYPER)[:3], adam_wrong_tail_skipped(*t, vis, **ac.HYPER)) == ((N * M) % 4 != 0), (N, M)
    groups = ac.e_groups()
    vis = ac.mask(ac.E_N, seed=50)
    right = [adam_ref(p, g, m, v, vis, lr, ac.B1, ac.B2, ac.EPS)[:3] for p, g, m, v, lr in groups]
    wrong = adam_wrong_groups_past_eight(groups, vis, ac.B1, ac.B2, ac.EPS)
    assert len(groups) == 11
    for i in range(11):
        assert _differs(right[i], wrong[i]) == (i >= 8), i
    # a group's own learning rate matters: no two groups of one width would pass with each other's
    for i, j in ((1, 7), (3, 9), (2, 10), (0, 6)):
        p, g, m, v, _ = groups[i]
        assert ac.E_WIDTHS[i] == ac.E_WIDTHS[j]
        assert _differs(right[i], adam_ref(p, g, m, v, vis, ac.E_LRS[j], ac.B1, ac.B2, ac.EPS)[:3])


def test_value_edges_of_the_reference():
    """Case (f) on the CPU: g = m = v = 0 leaves p's bits alone, and a NaN / Inf gradient stays in its own element."""
    for scale in ac.F_SCALES:
        p, g, m, v = ac.f_tensors(scale)
        rp, rm, rv, _ = adam_ref(p, g, m, v, np.ones(p.shape[0], np.uint8), **ac.HYPER)
        assert same_bits(rp.ravel()[ac.F_ZERO], p.ravel()[ac.F_ZERO]).all()
        assert not same_bits(rp.ravel()[ac.F_V0], p.ravel()[ac.F_V0]).all()
        assert np.isfinite(rp).all() and np.isfinite(rm).all() and np.isfinite(rv).all()
    p, g, m, v = ac.f_tensors(1.0, nonfinite=True)
    rp, rm, rv, _ = adam_ref(p, g, m, v, np.ones(p.shape[0], np.uint8), **ac.HYPER)
    bad = np.zeros(p.size, bool)
    bad[[ac.F_NAN, ac.F_INF]] = True
    for x in (rp, rm, rv):
        assert (~np.isfinite(x.ravel()) == bad).all()
    assert np.isnan(rm.ravel()[ac.F_NAN]) and np.isinf(rm.ravel()[ac.F_INF]) and np.isinf(rv.ravel()[ac.F_INF]) and np.isnan(rp.ravel()[ac.F_INF])
