"""-m gpu: densification on the device — the error-weighted contribution launch (gslic_contribution_accumulate_error), the clone / split selection
and emission (gslic_densify_select / gslic_densify_emit) and trainer.GaussianModel.densify on both row orders.

References, none of them the code under test: the plain contribution entry point and integer arithmetic for everything that must agree bit for bit,
the float64 replay of the forward's lists and the backward (dL_dcolor[:, 0] under dL_dpix = (e, 0, 0) is sum w e) for the error sums, the torch
restatement of the selection rule, plain torch indexing for every copied field, and the numpy / float64 restatement of the counter generator and
the split children (tests/densify_ref.py).  Scenes "a", "b", "c" are contribution_ref's.  All forwards run in strict arithmetic."""
import ctypes
import functools
import os
import types

import numpy as np
import pytest
import torch

import contribution_ref as cr
import densify_ref as dr
import fused_check_io as fio
from gpu_helpers import SENTINEL, bits, export_lists, gpu, guarded, map_snapshot, raw_forward, scene_model

pytestmark = pytest.mark.gpu

SENT_F = float(np.array([SENTINEL], np.uint32).view(np.float32)[0])


# ==================================================================================================== 1. the error accumulator
def _err_image(name, kind="random"):
    W, H = (cr.W_B, cr.H_B) if name == "b" else (cr.W_A, cr.H_A)
    if kind == "random":
        e = 2.0 * torch.rand(H, W, generator=torch.Generator().manual_seed(41))
    else:
        e = torch.full((H, W), float(kind))
    return e.to(gpu())


def _four(m, fwd, err, plain=False):
    """(max_w bits, n_pix, sum_w, err_sum) of one view as CPU tensors, through ContributionStats."""
    from gaussian_lic_amd import trainer
    st = trainer.ContributionStats(m)
    st.accumulate_from(fwd, cr.W_MIN, error=None if plain else err)
    torch.cuda.synchronize()
    out = [st.max_weight().view(torch.int32).cpu().clone(), st.pixels().cpu().clone(), st.sum_fixed().cpu().clone(), st.error_fixed().cpu().clone()]
    st.detach()
    return out


@pytest.fixture(scope="module")
def views():
    """Per scene: the model, the camera, one plain forward and the plain entry point's three arrays — computed once, left unchanged."""
    out = {}
    for name in ("a", "b"):
        m, cam = scene_model(name)
        fwd = raw_forward(m, cam)
        out[name] = (m, cam, fwd, _four(m, fwd, None, plain=True))
    return out


@pytest.mark.parametrize("name", ["a", "b"])
def test_constant_error_images(views, name):
    m, _cam, fwd, plain = views[name]
    assert bool(plain[2].any()) and not bool(plain[3].any())
    ones = _four(m, fwd, _err_image(name, 1.0))
    assert torch.equal(ones[3], ones[2])                                             # err == 1: err_sum == sum_w bit for bit
    assert all(torch.equal(a, b) for a, b in zip(ones[:3], plain[:3]))               # the other three: the old entry point's bits
    for kind in (0.0, float("nan"), -1.0, float("-inf")):
        got = _four(m, fwd, _err_image(name, kind))
        assert not bool(got[3].any()), kind
        assert all(torch.equal(a, b) for a, b in zip(got[:3], plain[:3])), kind
    four, eight, inf = (_four(m, fwd, _err_image(name, k))[3] for k in (4.0, 8.0, float("inf")))
    assert torch.equal(four, eight) and torch.equal(four, inf) and bool(four.any())
    assert bool((four >= 4 * plain[2] - 1024).all()) and bool((four <= 4 * plain[2] + 1024).all())   # (4 w is exact: the sums round alike)


def test_guard_words_and_subsets_of_the_outputs(views):
    from gaussian_lic_amd import rasterizer as rz
    m, _cam, fwd, plain = views["a"]
    P, (H, W) = m.P, fwd.hw
    R, B, _r, geom, binning, img, _s = fwd.state
    err = _err_image("a")
    g = [guarded(P, torch.int32, 0), guarded(P, torch.int32, 0), guarded(P, torch.int64, 0), guarded(P, torch.int64, 0)]
    rz.contribution_accumulate(P, H, W, R, B, geom, binning, img, cr.W_MIN, g[0][1], g[1][1], g[2][1], error=err, err_sum=g[3][1])
    torch.cuda.synchronize()
    for whole, _v in g:
        assert bool((whole[:64] == SENTINEL).all()) and bool((whole[64 + P:] == SENTINEL).all())
    assert torch.equal(g[0][1].cpu(), plain[0]) and torch.equal(g[1][1].cpu().long() & 0xffffffff, plain[1]) and torch.equal(g[2][1].cpu(), plain[2])
    full = g[3][1].cpu().clone()
    assert bool(full.any())
    only = torch.zeros(P, dtype=torch.int64, device=gpu())
    rz.contribution_accumulate(P, H, W, R, B, geom, binning, img, cr.W_MIN, None, None, None, error=err, err_sum=only)   # the three may be absent
    assert torch.equal(only.cpu(), full)
    with pytest.raises(ValueError, match="go together"):
        rz.contribution_accumulate(P, H, W, R, B, geom, binning, img, cr.W_MIN, None, None, None, error=err)


def test_runs_repeat_and_views_add_as_integers(views):
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    m, cam1, fwd, _plain = views["a"]
    cam2 = synthetic_camera(cr.W_A, cr.H_A, 5).to_device(gpu())
    err = _err_image("a")
    one, again = _four(m, fwd, err), _four(m, fwd, err)
    assert all(torch.equal(a, b) for a, b in zip(one, again)) and bool(one[3].any())
    two = _four(m, raw_forward(m, cam2), err)
    assert not torch.equal(one[3], two[3])
    st = trainer.ContributionStats(m)
    st.accumulate(cam1, w_min=cr.W_MIN, error=err)
    st.accumulate(cam2, w_min=cr.W_MIN, error=err)
    assert st.views == 2 and torch.equal(st.error_fixed().cpu(), one[3] + two[3]) and torch.equal(st.sum_fixed().cpu(), one[2] + two[2])
    assert torch.equal(st.error_sum().cpu(), trainer.fixed_to_weight(one[3] + two[3]))
    st.reset()
    assert not bool(st.error_fixed().any())
    st.detach()


@pytest.mark.parametrize("name", ["a", "b"])
def test_every_forward_and_binning_path_gives_the_same_error_sums(views, name):
    from gaussian_lic_amd import _lib
    from gaussian_lic_amd.rasterizer import CapacityBuffers
    m, cam, fwd, _plain = views[name]
    H, W = fwd.hw
    err = _err_image(name)
    want = _four(m, fwd, err)
    same = lambda got: all(torch.equal(a, b) for a, b in zip(want, got))
    old = _lib.set_binning_mode("radix")
    try:
        for mode in ("radix", "atomic"):
            _lib.set_binning_mode(mode)
            assert same(_four(m, raw_forward(m, cam), err)), mode
    finally:
        _lib.set_binning_mode(old)
    assert same(_four(m, raw_forward(m, cam, depth=True), err)), "depth forward"
    bufs = CapacityBuffers(m.P, W, H, 4096, 256, gpu())
    raw_forward(m, cam, bufs=bufs)
    assert bufs.read_status()[2] == 0 and same(_four(m, bufs, err)), "capacity forward"
    small = CapacityBuffers(m.P, W, H, max(fwd.state[0] // 3, 1), 256, gpu())       # the lists do not fit: nothing is accumulated
    raw_forward(m, cam, bufs=small)
    assert small.read_status()[2] != 0 and not any(bool(t.any()) for t in _four(m, small, err))


def test_nothing_in_view_leaves_zeros():
    m, cam = scene_model("c")
    fwd = raw_forward(m, cam)
    assert fwd.state[0] == 0
    assert not any(bool(t.any()) for t in _four(m, fwd, _err_image("a")))


def _replay_error(m, cam, fwd, err):
    H, W = fwd.hw
    d = export_lists(m, cam, fwd, ("means2D", "conic_opacity", "point_list", "ranges", "n_contrib"))
    n = lambda k: d[k].cpu().numpy()
    return dr.replay_error(n("means2D"), n("conic_opacity"), n("point_list"), n("ranges"), n("n_contrib"), W, H, m.P, err.cpu().numpy())


@pytest.mark.parametrize("name", ["a", "b"])
def test_random_error_against_the_replay_and_the_backward(views, name):
    from gaussian_lic_amd import trainer
    m, cam, fwd, _plain = views[name]
    H, W = fwd.hw
    err = _err_image(name)
    got = trainer.fixed_to_weight(_four(m, fwd, err)[3]).numpy()
    ref = _replay_error(m, cam, fwd, err)
    dL = torch.zeros(3, H, W, device=gpu())
    dL[0] = err
    with torch.no_grad():
        bwd = fwd.backward(dL)[1][:, 0].double().cpu().numpy()
    g_rep, g_bwd = dr.max_gap(got, ref), dr.max_gap(got, bwd)
    print(f"[densify gap] err_sum scene {name}: vs float64 replay {g_rep:.3e}  vs backward {g_bwd:.3e}  (bar {dr.ERR_MARGIN}; max {ref.max():.4f})")
    assert ref.max() > 0.5 and bool(((ref > 0) == (got > 0)).all())
    assert g_rep <= dr.ERR_MARGIN and g_bwd <= dr.ERR_MARGIN


# ==================================================================================================== 2. selection
def _rows(P, M, seed):
    """Random raw parameter rows on the device; the scalings straddle log(1) = 0."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    t = dict(xyz=3.0 * r(P, 3), features_dc=r(P, 3), features_rest=r(P, 3 * M), opacity=r(P, 1), scaling=1.5 * r(P, 3) - 1.0, rotation=r(P, 4))
    return {k: v.to(gpu()).contiguous() for k, v in t.items()}


NAMES = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")


def _select(t, grow, protect, tie, thr):
    from gaussian_lic_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    P = t["xyz"].shape[0]
    parent = torch.full((P + 16,), SENTINEL, dtype=torch.int32, device=gpu())
    count, split = ctypes.c_int32(-1), ctypes.c_int32(-1)
    scratch = _lib.TensorAllocator(gpu())
    u8 = lambda x: None if x is None else x.to(torch.uint8).contiguous()
    grow8, protect8, tie32 = u8(grow), u8(protect), (None if tie is None else tie.to(torch.int32).contiguous())   # (kept alive across the call)
    _lib.check(L.gslic_densify_select(P, p(t["xyz"]), p(t["features_dc"]), p(t["opacity"]), p(t["scaling"]), p(t["rotation"]), p(grow8), p(protect8),
                                      p(tie32), thr, scratch.cb, None, p(parent), ctypes.byref(count), ctypes.byref(split), _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    del grow8, protect8, tie32
    return parent, count.value, split.value


def _masks(P, seed):
    g = torch.Generator().manual_seed(seed)
    one, last = torch.zeros(P, dtype=torch.bool), torch.zeros(P, dtype=torch.bool)
    one[P // 3] = True
    last[P - 1] = True
    return {"none": torch.zeros(P, dtype=torch.bool), "all": torch.ones(P, dtype=torch.bool), "random": torch.rand(P, generator=g) < 0.3, "one": one,
            "last": last}


@pytest.mark.parametrize("P", [1, 63, 64, 65, 257, 4097])
def test_selection_equals_the_torch_rule(P):
    t = _rows(P, 0, 100 + P)
    thr = float(np.float32(0.0))
    t["scaling"][::5, 1] = thr                                                # rows AT the threshold ...
    t["scaling"][::5, 0] = -1.0
    t["scaling"][::5, 2] = -2.0                                               # ... with nothing above it: they clone
    g = torch.Generator().manual_seed(P)
    protect = (torch.rand(P, generator=g) < 0.2).to(gpu())
    tie = torch.randperm(P, generator=g).to(gpu())
    for mname, grow in _masks(P, 7 * P).items():
        grow = grow.to(gpu())
        for prot in (None, protect):
            for ti in (None, tie):
                parent, count, split = _select(t, grow, prot, ti, thr)
                want, wcount, wsplit, smask = dr.select(t["xyz"], t["features_dc"], t["opacity"], t["scaling"], t["rotation"], grow, prot, ti, thr)
                what = (P, mname, prot is not None, ti is not None)
                assert (count, split) == (wcount, wsplit), what
                assert torch.equal(parent[:count].long(), want), what
                assert bool((parent[count:] == SENTINEL).all()), what
                assert not bool(smask[::5].any())
                if mname == "all" and prot is None and P >= 63:
                    assert 0 < wsplit < wcount == P


def test_non_finite_rows_and_zero_quaternions_are_not_eligible():
    P = 65
    t = _rows(P, 0, 5)
    bad = {"xyz": (3, 1, float("nan")), "features_dc": (7, 2, float("inf")), "opacity": (11, 0, float("-inf")), "scaling": (13, 1, float("nan")),
           "rotation": (17, 3, float("inf"))}
    for name, (row, col, v) in bad.items():
        t[name][row, col] = v
    t["rotation"][23] = 0.0
    t["rotation"][29] = torch.tensor([0.0, 0.0, -0.0, 1e-30])                 # not zero, but its float32 squared norm underflows to 0: no direction
    t["rotation"][31] = torch.tensor([0.0, 3e-19, -0.0, 1e-18])               # tiny with a float32 squared norm > 0: eligible
    grow = torch.ones(P, dtype=torch.bool, device=gpu())
    parent, count, split = _select(t, grow, None, None, 0.0)
    out = {3, 7, 11, 13, 17, 23, 29}
    assert count == P - len(out) and sorted(parent[:count].tolist()) == [i for i in range(P) if i not in out]
    want, wcount, wsplit, _s = dr.select(t["xyz"], t["features_dc"], t["opacity"], t["scaling"], t["rotation"], grow, None, None, 0.0)
    assert torch.equal(parent[:count].long(), want) and (count, split) == (wcount, wsplit)


# ==================================================================================================== 3. emission
def _emit_case(P, M, with_tie, seed, thr=0.0, mask="random"):
    """Storage of P + k + 8 rows, sentinel beyond P, non-zero moments; runs select + emit.  Returns before / after snapshots and the bookkeeping."""
    from gaussian_lic_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    t = _rows(P, M, 300 + P + M)
    grow = _masks(P, 11 * P)[mask].to(gpu())
    g = torch.Generator().manual_seed(P + 1)
    tie = torch.randperm(P, generator=g).to(gpu()) if with_tie else None
    parent, k, n_split = _select(t, grow, None, tie, thr)
    cap = P + k + 8
    buf, m1, m2 = {}, {}, {}
    for i, n in enumerate(NAMES):
        w = t[n].shape[1]
        buf[n] = torch.full((cap, w), SENT_F, device=gpu())
        buf[n][:P] = t[n]
        m1[n] = torch.full((cap, w), 0.25 + i, device=gpu())
        m2[n] = torch.full((cap, w), 0.5 + i, device=gpu())
    tie_buf = None
    if with_tie:
        tie_buf = torch.full((cap,), SENTINEL, dtype=torch.int32, device=gpu())
        tie_buf[:P] = tie.to(torch.int32)
    before = {n: (buf[n].clone(), m1[n].clone(), m2[n].clone()) for n in NAMES}
    tie_before = None if tie_buf is None else tie_buf.clone()
    six = lambda d: (ctypes.c_void_p * 6)(*[(d[n].data_ptr() if d[n].numel() else None) for n in NAMES])
    _lib.check(L.gslic_densify_emit(P, k, p(parent), M, six(buf), six(m1), six(m2), p(tie_buf), thr, seed, _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    return types.SimpleNamespace(P=P, k=k, n_split=n_split, parent=parent[:k].long(), buf=buf, m1=m1, m2=m2, tie=tie_buf, before=before, tie_before=tie_before,
                                 orig=t, o=(tie if with_tie else torch.arange(P, device=gpu())), thr=thr, seed=seed)


def _xyz_gap(c):
    """Largest gap of the split children's xyz from the float64 restatement, relative to the parent's largest activated scale."""
    split = (c.orig["scaling"][c.parent] > c.thr).any(1)
    par = c.parent[split]
    new = (c.P + torch.arange(c.k, device=gpu()))[split]
    if par.numel() == 0:
        return 0.0
    n = lambda x: x.cpu().numpy()
    xyz, sc, rot, o = n(c.orig["xyz"][par]), n(c.orig["scaling"][par]), n(c.orig["rotation"][par]), n(c.o[par])
    scale = np.exp(sc.astype(np.float64)).max(1, keepdims=True)
    gap = 0.0
    for child, rows in ((0, par), (1, new)):
        ref = dr.child_xyz(xyz, sc, rot, o, c.seed, child)
        gap = max(gap, float((np.abs(n(c.buf["xyz"][rows]).astype(np.float64) - ref) / scale).max()))
    return gap


def _check_emission(P, M):
    for with_tie in (False, True):
        mask = "all" if P < 63 else "random"
        c = _emit_case(P, M, with_tie, seed=9, mask=mask)
        k, par = c.k, c.parent
        assert k > 0
        new = P + torch.arange(k, device=gpu())
        split = (c.orig["scaling"][par] > c.thr).any(1)
        assert int(split.sum()) == c.n_split
        sp, cl = par[split], par[~split]
        touched = torch.zeros(P + k + 8, dtype=torch.bool, device=gpu())
        for n in NAMES:
            b0, m10, m20 = c.before[n]
            b, m1, m2 = c.buf[n], c.m1[n], c.m2[n]
            # rows >= P + k and every row that is not a (split) parent are untouched
            keep = torch.ones(P + k + 8, dtype=torch.bool, device=gpu())
            keep[new] = False
            keep_m = keep.clone()
            keep_m[sp] = False
            if n in ("xyz", "scaling"):
                keep[sp] = False
            assert torch.equal(bits(b[keep]), bits(b0[keep])), n
            assert torch.equal(bits(m1[keep_m]), bits(m10[keep_m])) and torch.equal(bits(m2[keep_m]), bits(m20[keep_m])), n
            # moments: zero on the new rows and the split parents
            for mm in (m1, m2):
                assert not bool(bits(mm[new]).any()) and not bool(bits(mm[sp]).any()), n
            # copied fields
            if n in ("features_dc", "features_rest", "opacity", "rotation"):
                assert torch.equal(bits(b[new]), bits(b0[par])), n
            else:
                assert torch.equal(bits(b[new][~split]), bits(b0[cl])), n            # clone: bit copy of xyz and scaling too
        shr = c.orig["scaling"][sp] - torch.tensor(float(dr.SHRINK), device=gpu())    # ONE float32 subtraction
        assert torch.equal(bits(c.buf["scaling"][sp]), bits(shr)) and torch.equal(bits(c.buf["scaling"][new[split]]), bits(shr))
        if with_tie:
            assert torch.equal(c.tie[:P], c.tie_before[:P]) and torch.equal(c.tie[P:P + k].long(), new) and bool((c.tie[P + k:] == SENTINEL).all())
            assert torch.equal(torch.sort(c.o[par]).values, c.o[par])                   # new rows in the order of the parents' original indices
        if c.n_split:
            assert not bool((c.buf["xyz"][sp] == c.buf["xyz"][new[split]]).all(1).any())   # the two children differ
            assert bool(torch.isfinite(c.buf["xyz"][:P + k]).all())
        gap = _xyz_gap(c)
        print(f"[densify gap] split xyz P {P} M {M} tie {with_tie}: splits {c.n_split} gap / largest scale {gap:.3e} (bar {dr.XYZ_MARGIN})")
        assert gap <= dr.XYZ_MARGIN
        # the same seed gives the same bits, another seed other positions (and nothing else)
        again, other = _emit_case(P, M, with_tie, seed=9, mask=mask), _emit_case(P, M, with_tie, seed=10, mask=mask)
        for n in NAMES:
            assert torch.equal(bits(again.buf[n]), bits(c.buf[n])), n
            if n != "xyz":
                assert torch.equal(bits(other.buf[n]), bits(c.buf[n])), n
        if c.n_split:
            assert not torch.equal(other.buf["xyz"][sp], c.buf["xyz"][sp]) and torch.equal(bits(other.buf["xyz"][cl]), bits(c.buf["xyz"][cl]))


@pytest.mark.parametrize("M", [15, 0])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 257, 4097])
def test_emission(P, M):
    _check_emission(P, M)


@pytest.mark.parametrize("P", [3, 65])
def test_emission_of_rows_wider_than_one_workgroup_takes(P):
    """features_rest rows of 4200 dwords: more than the 4096 a workgroup of the wide launch owns, so one row is walked by a workgroup's lanes alone —
    in a copy segment (features_rest) and in two zero segments (its moments).  The smallest shape that gets there; about 1 MB of storage."""
    _check_emission(P, 1400)


def test_a_parent_index_outside_the_map_is_never_an_address():
    """gslic_densify_emit on a parent_index with entries >= P (select writes none): their new rows are left alone in all 18 arrays, the other new
    rows are those of the emission without them, bit for bit, and nothing else is touched."""
    from gaussian_lic_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    P, M, thr, seed = 65, 15, 0.0, 5
    t = _rows(P, M, 91)
    t["scaling"][2] = torch.tensor([1.0, -1.0, -1.0])                          # parent 2 splits
    t["scaling"][64] = torch.tensor([-0.5, -1.0, 0.0])                         # parent 64 (the last row, at the threshold) clones
    six = lambda d: (ctypes.c_void_p * 6)(*[d[n].data_ptr() for n in NAMES])

    def emit(parents):
        count = len(parents)
        cap = P + count + 8
        st = []
        for fill in (SENT_F, 0.25, 0.5):                                       # parameters, exp_avg, exp_avg_sq: sentinels beyond P, non-zero moments
            d = {n: torch.full((cap, t[n].shape[1]), SENT_F, device=gpu()) for n in NAMES}
            for n in NAMES:
                d[n][:P] = t[n] if fill == SENT_F else fill
            st.append(d)
        before = [{n: d[n].clone() for n in NAMES} for d in st]
        index = torch.tensor(parents, dtype=torch.int32, device=gpu())
        _lib.check(L.gslic_densify_emit(P, count, p(index), M, six(st[0]), six(st[1]), six(st[2]), None, thr, seed, _lib.current_stream_ptr()))
        torch.cuda.synchronize()
        return st, before

    (got, before), (want, _b) = emit([2, -1, 64, 70]), emit([2, 64])          # (-1: the 32 bits of 0xffffffff)
    for g, b, w in zip(got, before, want):
        for n in NAMES:
            what = (n, g is got[0])
            assert torch.equal(bits(g[n][P + 0]), bits(w[n][P + 0])) and torch.equal(bits(g[n][P + 2]), bits(w[n][P + 1])), what   # as without them
            assert not bool((bits(w[n][P:P + 2]) == SENTINEL).any()), what                                                            # (and written)
            assert bool((bits(g[n][P + 1]) == SENTINEL).all()) and bool((bits(g[n][P + 3]) == SENTINEL).all()), what                 # left alone
            assert bool((bits(g[n][P + 4:]) == SENTINEL).all()), what                                                                 # the guard rows
            rest = torch.arange(P, device=gpu()) != 2
            assert torch.equal(bits(g[n][:P][rest]), bits(b[n][:P][rest])), what                                                     # every other old row
            assert torch.equal(bits(g[n][2]), bits(w[n][2])), what                                                                   # the split parent
    for d in got[1:]:
        for n in NAMES:
            assert not bool(bits(d[n][2]).any()) and not bool(bits(d[n][P + 0]).any()) and not bool(bits(d[n][P + 2]).any()), n     # zero moments
    for n in ("features_dc", "features_rest", "opacity", "rotation"):
        assert torch.equal(bits(got[0][n][2]), bits(before[0][n][2])), n                                                             # no thread writes these


def test_tiny_quaternions_split_to_finite_children():
    """Rows whose quaternion is tiny: those with a float32 squared norm of 0 are not eligible (a split would divide by it), the others split into
    finite children that meet the float64 restatement like every other row."""
    from gaussian_lic_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    P, M, thr, seed = 65, 0, float("-inf"), 4                                  # every eligible row splits
    t = _rows(P, M, 77)
    t["rotation"][::4] = t["rotation"][::4] * 1e-18                            # squared norm about 1e-36: a normal float32
    dead = torch.arange(1, P, 8)
    t["rotation"][dead] = t["rotation"][dead] * 1e-30                          # squared norm underflows to 0
    grow = torch.ones(P, dtype=torch.bool, device=gpu())
    parent, k, n_split = _select(t, grow, None, None, thr)
    want, wk, ws, _s = dr.select(t["xyz"], t["features_dc"], t["opacity"], t["scaling"], t["rotation"], grow, None, None, thr)
    assert k == wk == n_split == ws == P - dead.numel() and torch.equal(parent[:k].long(), want)
    buf = {n: torch.cat([t[n], torch.full((k, t[n].shape[1]), SENT_F, device=gpu())]) for n in NAMES}
    m1 = {n: torch.ones_like(buf[n]) for n in NAMES}
    m2 = {n: torch.ones_like(buf[n]) for n in NAMES}
    six = lambda d: (ctypes.c_void_p * 6)(*[(d[n].data_ptr() if d[n].numel() else None) for n in NAMES])
    _lib.check(L.gslic_densify_emit(P, k, p(parent), M, six(buf), six(m1), six(m2), None, thr, seed, _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(buf["xyz"]).all()) and bool(torch.isfinite(buf["scaling"]).all())
    assert torch.equal(bits(buf["xyz"][dead.to(gpu())]), bits(t["xyz"][dead.to(gpu())]))          # ineligible rows are untouched
    c = types.SimpleNamespace(P=P, k=k, parent=parent[:k].long(), buf=buf, orig=t, o=torch.arange(P, device=gpu()), thr=thr, seed=seed)
    gap = _xyz_gap(c)
    print(f"[densify gap] split xyz, tiny quaternions: splits {n_split} gap / largest scale {gap:.3e} (bar {dr.XYZ_MARGIN})")
    assert gap <= dr.XYZ_MARGIN


def test_all_clone_and_all_split_thresholds():
    for thr, frac in ((float("inf"), 0.0), (float("-inf"), 1.0)):
        c = _emit_case(257, 15, True, seed=3, thr=thr, mask="all")
        assert c.k == 257 and c.n_split == int(frac * 257)
        if frac == 0.0:
            for n in NAMES:
                assert torch.equal(bits(c.buf[n][257:514]), bits(c.orig[n][c.parent])), n
                assert torch.equal(bits(c.buf[n][:257]), bits(c.orig[n])), n


# ==================================================================================================== 4. the model
W, H, NP = 64, 48, 3000


def _scene():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd.synthetic import random_scene
    return random_scene(NP, W, H, sh_degree=3, seed=3)


def _trained(raw, order, steps=2, **kw):
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import gt_image
    dev = gpu()
    m = trainer.GaussianModel({k: (v.clone() if torch.is_tensor(v) else v) for k, v in raw.items()}, dev, order=order, **kw)
    m.training_setup()
    cam = synthetic_camera(W, H).to_device(dev)
    gt, bg = gt_image(H, W).to(dev), torch.zeros(3, device=dev)
    for _ in range(steps):
        trainer.training_step_fused(m, cam, gt, bg)
    return m, cam, gt, bg


def _median_scale(m):
    return float(torch.exp(m.scaling.detach().double()).max(1).values.median())


def test_both_row_orders_densify_to_the_same_map():
    from gaussian_lic_amd.rasterizer import render
    raw = _scene()
    a, cam, gt, bg = _trained(raw, "insertion", capacity=2 * NP)
    d, _c, _g, _b = _trained(raw, "morton", capacity=2 * NP, resort_fraction=None)
    grow = torch.rand(NP, generator=torch.Generator().manual_seed(1)).to(gpu()) < 0.3      # in ORIGINAL order
    s = _median_scale(a)
    ka, sa, _pa = a.densify(grow, s, seed=5)
    kd, sd, pd = d.densify(grow[d.tie_rank[:NP].long()], s, seed=5)
    assert (ka, sa) == (kd, sd) and 0 < sa < ka == int(grow.sum())
    assert a.P == d.P == NP + ka and a.layout_version == 1
    assert torch.equal(torch.sort(d.tie_rank.long()).values, torch.arange(d.P, device=gpu()))
    assert torch.equal(d.tie_rank[pd].long(), torch.sort(d.tie_rank[pd].long()).values)
    sa_, sd_ = map_snapshot(a), map_snapshot(d, d.original_order())
    for k in sa_:
        assert torch.equal(bits(sa_[k]), bits(sd_[k])), k
    with torch.no_grad():
        ia, id_ = render(cam, a, bg)[0], render(cam, d, bg)[0]
    assert torch.equal(bits(ia), bits(id_)) and bool(torch.isfinite(ia).all())


@pytest.mark.parametrize("order", ["insertion", "morton"])
def test_clone_then_prune_restores_the_map_and_training_goes_on(order):
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.synthetic import lidar_scene
    dev = gpu()
    m, cam, gt, bg = _trained(_scene(), order, resort_fraction=None)             # no spare capacity: the storage grows
    before, tie0 = map_snapshot(m), (None if m._tie is None else m._tie[:NP].clone())
    grow = torch.rand(NP, generator=torch.Generator().manual_seed(2)).to(dev) < 0.25
    with pytest.raises(ValueError, match="max_new"):
        m.densify(grow, None, max_new=int(grow.sum()) - 1)
    assert m.P == NP and m.layout_version == 0 and all(torch.equal(bits(v), bits(map_snapshot(m)[k])) for k, v in before.items())   # untouched
    k, n_split, parents = m.densify(grow, None, max_new=int(grow.sum()))         # split_scale None: every row clones
    assert k == int(grow.sum()) and n_split == 0 and m.P == NP + k and m.capacity >= NP + k
    assert torch.equal(torch.sort(parents).values, grow.nonzero().squeeze(1))
    for n in m.NAMES:
        assert torch.equal(bits(m._buf[n][NP:NP + k]), bits(m._buf[n][parents])) and not bool(m._m[n][NP:NP + k].any()) and not bool(m._v[n][NP:NP + k].any())
    drop = torch.zeros(m.P, dtype=torch.bool, device=dev)
    drop[NP:] = True
    n_removed, _kept = m.prune(drop=drop)
    assert n_removed == k and m.P == NP
    after = map_snapshot(m)
    for key in before:
        assert torch.equal(bits(before[key]), bits(after[key])), key
    if tie0 is not None:
        assert torch.equal(m._tie[:NP], tie0)
    # a split densify, a fused step, then extend: ties stay a permutation of 0..P-1
    k2, s2, _p = m.densify(grow, _median_scale(m), seed=1)
    assert k2 == k and 0 < s2 < k2
    terms, _ = trainer.training_step_fused(m, cam, gt, bg)
    assert bool(torch.isfinite(terms).all()) and all(bool(torch.isfinite(m._buf[n][:m.P]).all()) for n in m.NAMES)
    frame = lidar_scene(500, W, H, sh_degree=3, seed=77)
    col = (frame["features_dc"].reshape(-1, 3) * 0.28209479177387814 + 0.5).to(dev)
    Rcw = torch.from_numpy(cam.world_view_transform[:3, :3].T.copy())
    tcw = torch.from_numpy(cam.world_view_transform[3, :3].copy())
    u_pix = m.xyz.detach()[:, 0] * (0.675 * W) / m.xyz.detach()[:, 2].abs().clamp_min(0.2) + 0.4857 * W
    m.prune(drop=u_pix > 0.5 * W)                                                # room in the right half of the image for LiDAR points
    P1 = m.P
    k3 = m.extend(cam, frame["xyz"].to(dev), col, frame["xyz"][:, 2].contiguous().to(dev), Rcw, tcw, (float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy)))
    assert k3 > 0 and m.P == P1 + k3
    if order == "morton":
        assert torch.equal(torch.sort(m.tie_rank.long()).values, torch.arange(m.P, device=dev))
    trainer.training_step_fused(m, cam, gt, bg)


def test_attached_stats_follow_a_densify():
    from gaussian_lic_amd import trainer
    m, cam, gt, bg = _trained(_scene(), "morton", steps=1, resort_fraction=None)
    st = trainer.ContributionStats(m)
    with torch.no_grad():
        err = (trainer.render(cam, m, bg)[0] - gt).abs().mean(0)
    st.accumulate(cam, error=err)
    loose = trainer.ContributionStats(m)
    loose.detach()
    old = [t.clone() for t in (st._max[:NP], st._npix[:NP], st._sum[:NP], st._err[:NP])]
    assert all(bool(t.any()) for t in old)
    grow = st.grow_mask(error_above=float(st.error_sum().median()), min_pixels=1)
    assert torch.equal(grow.bool(), (st.error_fixed() > int(trainer.weight_to_fixed(float(st.error_sum().median())))) & (st.pixels() >= 1))
    thr = trainer.densify_threshold(_median_scale(m))
    was_split = grow.bool() & (m._buf["scaling"][:NP] > thr).any(1)
    k, n_split, parents = m.densify(grow, _median_scale(m))
    assert 0 < n_split == int(was_split.sum()) < k == int(grow.sum())
    new = [st._max[:m.P], st._npix[:m.P], st._sum[:m.P], st._err[:m.P]]
    for o, n in zip(old, new):
        assert not bool(n[NP:].any()) and not bool(n[:NP][was_split].any()) and torch.equal(n[:NP][~was_split], o[~was_split])
    assert st.error_fixed().shape[0] == m.P and st.views == 1
    with pytest.raises(RuntimeError, match="rows changed"):
        loose.error_fixed()
    # the fourth array also follows prune() and resort()
    st.accumulate(cam, error=err)
    e0 = st.error_fixed().clone()
    perm = m.resort()
    assert torch.equal(st.error_fixed(), e0[perm])
    _n, kept = m.prune(drop=st.drop_mask(pixels_below=1))
    assert torch.equal(st.error_fixed(), e0[perm][kept])


def test_graphed_step_refuses_a_stale_layout_after_densify():
    from gaussian_lic_amd import trainer
    m, cam, gt, bg = _trained(_scene(), "morton", steps=1, capacity=2 * NP)
    gs = trainer.GraphedStep(m, cam, gt, bg, check_every=0)
    gs.step()
    assert gs.check() == 0
    k, _s, _p = m.densify(torch.arange(m.P, device=gpu()) % 7 == 0, _median_scale(m))
    assert k > 0
    with pytest.raises(RuntimeError, match="rows changed since this step was built"):
        gs.step()
    gs2 = trainer.GraphedStep(m, cam, gt, bg, check_every=0)
    terms = gs2.step()
    assert gs2.check() == 0 and bool(torch.isfinite(terms).all())


def test_densify_before_training_setup():
    """No optimizer yet: densify() grows the storage, zero moments included, and training_setup() afterwards binds the grown map."""
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import gt_image
    dev = gpu()
    raw = _scene()
    for order in ("insertion", "morton"):
        m = trainer.GaussianModel({k: (v.clone() if torch.is_tensor(v) else v) for k, v in raw.items()}, dev, order=order, resort_fraction=None)
        assert m.optimizer is None
        before = map_snapshot(m)
        grow = torch.arange(NP, device=dev) % 3 == 0
        k, n_split, parents = m.densify(grow, _median_scale(m), seed=2)
        assert m.optimizer is None and k == int(grow.sum()) and 0 < n_split < k and m.P == NP + k and m.xyz.shape[0] == m.P
        split = (before["scaling"][parents] > trainer.densify_threshold(_median_scale_of(before["scaling"]))).any(1)
        assert int(split.sum()) == n_split
        for n in m.NAMES:
            assert not bool(m._m[n][:m.P].any()) and not bool(m._v[n][:m.P].any()), n
            if n not in ("xyz", "scaling"):
                assert torch.equal(bits(m._buf[n][:NP]), bits(before[n])) and torch.equal(bits(m._buf[n][NP:m.P]), bits(before[n][parents])), n
        assert torch.equal(bits(m._buf["xyz"][NP:m.P][~split]), bits(before["xyz"][parents[~split]]))
        m.training_setup()
        cam = synthetic_camera(W, H).to_device(dev)
        terms, _ = trainer.training_step_fused(m, cam, gt_image(H, W).to(dev), torch.zeros(3, device=dev))
        assert bool(torch.isfinite(terms).all())


def _median_scale_of(scaling):
    return float(torch.exp(scaling.double()).max(1).values.median())


# ==================================================================================================== 5. the C++ host
@pytest.mark.parametrize("order", ["insertion", "morton"])
def test_fused_densify_cpp_host(tmp_path, order):
    """gslic::FusedStep::accumulate_contribution(..., error) and gslic::FusedStep::densify issue the calls of the Python host: after two steps, one
    view accumulated with an error image, a densify of the rows above the median error sum (clones and splits) and two more steps, all 19 arrays
    (6 parameters, 12 moments, the tie rank) and err_sum are bit-identical to the Python model's, on both row orders."""
    from gaussian_lic_amd import trainer
    exe = fio.build("fused_densify")
    iters, seed = 2, 11
    m, cam, gt, bg = _trained(_scene(), order, steps=0, resort_fraction=None)
    d = str(tmp_path)
    fio.write_inputs(d, m, cam, gt=gt, tie_rank=m.tie_rank)
    for _ in range(iters):
        trainer.training_step_fused(m, cam, gt, bg)
    with torch.no_grad():
        err = (trainer.render(cam, m, bg)[0] - gt).abs().mean(0).contiguous()
    fio.write(d, "err", err)
    st = trainer.ContributionStats(m)
    st.accumulate(cam, w_min=cr.W_MIN, error=err)
    error_above = float(st.error_sum()[st.error_fixed() > 0].median())
    lim = int(trainer.weight_to_fixed(error_above))
    split_scale = _median_scale(m)
    k, n_split, parents = m.densify(st.grow_mask(error_above), split_scale, seed=seed)
    assert 0 < n_split < k < NP
    for _ in range(iters):
        trainer.training_step_fused(m, cam, gt, bg)
    r = fio.run(exe, d, str(NP), str(W), str(H), "3", str(iters), repr(cr.W_MIN), str(lim), repr(split_scale), str(seed))
    assert f"densify added {k} splits {n_split} size {m.P}" in r.stdout
    rd = functools.partial(fio.read, d)
    P = m.P
    for n, f in (("xyz", "xyz"), ("features_dc", "dc"), ("features_rest", "rest"), ("opacity", "opacity"), ("scaling", "scaling"), ("rotation", "rotation")):
        for pre, src in (("", m._buf), ("m_", m._m), ("v_", m._v)):
            assert torch.equal(rd(pre + f + ".f32", np.int32), bits(src[n][:P]).cpu().reshape(-1)), pre + f
    if order == "morton":
        assert torch.equal(rd("tie.i32", np.int32), m.tie_rank.cpu())
    else:
        assert not os.path.exists(os.path.join(d, "out_tie.i32"))
    assert torch.equal(rd("err_sum.i64", np.int64), st.error_fixed().cpu())
    assert torch.equal(rd("parents.i64", np.int64), parents.cpu())
