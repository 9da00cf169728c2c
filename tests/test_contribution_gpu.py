"""-m gpu: per-Gaussian contribution statistics (gslic_contribution_accumulate, trainer.ContributionStats, gslic::FusedStep::accumulate_contribution).

References, none of them the code under test: the backward (dL_dcolor[:, 0] under dL_dpix = e_0 is the sum of the blend weights of a Gaussian,
and the backward is pinned to the reference's kernels), a float64 numpy replay of the lists gslic_debug_export returns (tests/contribution_ref.py),
and plain torch indexing for everything that moves rows.  All forwards run in strict arithmetic.  Scenes (contribution_ref.scene):
  a  96 Gaussians, SH degree 0, 40 x 24: 3 x 2 tiles, right column and bottom row partial        b  400 Gaussians on the one tile of 16 x 16, high
  c  scene a behind the camera: R = 0                                                               opacities: three staging batches, early stops
  d  scene a in a Morton-ordered model (tie_rank): storage rows, equal to a's after un-permuting"""
import functools

import numpy as np
import pytest
import torch

import contribution_ref as cr
import fused_check_io as fio
from conftest import rel_err
from gpu_helpers import SENTINEL, export_lists, gpu, guarded, raw_forward, same_tensors, scene_model

pytestmark = pytest.mark.gpu

TOL = 1e-4          # the bar the project applies to gradients (tests/refcompare.py: TOL; conftest.rel_err)


def _stats(m, fwds=(), cams=(), w_min=cr.W_MIN):
    from gaussian_lic_amd import trainer
    st = trainer.ContributionStats(m)
    for f in fwds:
        st.accumulate_from(f, w_min)
    for c in cams:
        st.accumulate(c, w_min=w_min)
    return st


def _arrays(st):
    """(max_w bits, n_pix, sum_w bits) as CPU tensors: what is compared bit for bit."""
    torch.cuda.synchronize()
    return st.max_weight().view(torch.int32).cpu().clone(), st.pixels().cpu().clone(), st.sum_fixed().cpu().clone()


def _replay(m, cam, fwd, **kw):
    (H, W), R, P = fwd.hw, fwd.state[0], m.P
    if R == 0:
        z = np.zeros
        return cr.replay(z((P, 2)), z((P, 4)), z(0, np.int64), z((((W + 15) // 16) * ((H + 15) // 16), 2), np.int64), z((H, W), np.int64), W, H, P, **kw)
    d = export_lists(m, cam, fwd, ("means2D", "conic_opacity", "point_list", "ranges", "n_contrib"))
    n = lambda k: d[k].cpu().numpy()
    return cr.replay(n("means2D"), n("conic_opacity"), n("point_list"), n("ranges"), n("n_contrib"), W, H, P, **kw)


def _check_against_replay(st, rep, what):
    """max_weight within MARGIN (relative), the count inside the replay's band, exact zeros where the replay has no contributor; the replay's own
    ambiguity at w_min stays within 2 % of the visible Gaussians.  Prints the measured gap before it asserts."""
    mx, npix, sm = (t.numpy() for t in _arrays(st))
    mx = mx.view(np.float32).astype(np.float64)
    vis = rep["pairs"] > 0
    gap = float((np.abs(mx - rep["max_w"])[vis] / rep["max_w"][vis]).max()) if vis.any() else 0.0
    sgap = rel_err(st.sum_weight().cpu().numpy(), rep["sum_w"])
    print(f"[contribution gap] {what}: visible {int(vis.sum())} max_w rel gap {gap:.3e} (bar {cr.MARGIN:.1e}) sum_w rel_err {sgap:.3e} "
          f"band share {cr.band_share(rep):.4f} count outside band {int(((npix < rep['n_hi']) | (npix > rep['n_lo'])).sum())}")
    assert cr.band_share(rep) <= 0.02
    assert gap <= cr.MARGIN
    assert bool(((npix >= rep["n_hi"]) & (npix <= rep["n_lo"])).all())
    assert not mx[~vis].any() and not npix[~vis].any() and not sm[~vis].any()
    assert bool((mx[vis] > 0).all()) and bool((sm[vis] > 0).all())
    assert sgap < TOL


# ---------------------------------------------------------------------------------------------------- 1. against the backward
@pytest.mark.parametrize("name", ["a", "b"])
def test_sum_of_weights_is_the_backwards_colour_gradient(name):
    from gaussian_lic_amd.rasterizer import render
    m, cam = scene_model(name)
    fwd = raw_forward(m, cam)
    H, W = fwd.hw
    dL = torch.zeros(3, H, W, device=gpu())
    dL[0] = 1.0
    with torch.no_grad():
        grads = fwd.backward(dL)
        final_T = render(cam, m, torch.zeros(3, device=gpu()))[1]
    dL_dcolor = grads[1]
    st = _stats(m, fwds=[fwd])
    sw = st.sum_weight().cpu().numpy()
    e = rel_err(sw, dL_dcolor[:, 0].double().cpu().numpy())
    total, covered = float(sw.sum()), float((1.0 - final_T.double()).sum())
    print(f"[contribution vs backward] scene {name}: rel_err {e:.3e}  sum(sum_w) {total:.6f} sum(1 - final_T) {covered:.6f}")
    assert float(dL_dcolor[:, 0].abs().max()) > 0.5
    assert e < TOL
    assert abs(total - covered) <= TOL * covered
    assert st.views == 1


# ---------------------------------------------------------------------------------------------------- 2. against a replay
@pytest.mark.parametrize("name", ["a", "b"])
def test_statistics_match_the_float64_replay(name):
    m, cam = scene_model(name)
    fwd = raw_forward(m, cam)
    rep = _replay(m, cam, fwd)
    if name == "b":   # the list crosses staging batches and every pixel stops well before its end
        R, nc = fwd.state[0], rep["pairs"].sum()
        assert R == cr.P_B and nc > 0
        assert 128 < int(_ncontrib_max(m, cam, fwd)) < R // 2
    _check_against_replay(_stats(m, fwds=[fwd]), rep, "scene " + name)


def _ncontrib_max(m, cam, fwd):
    return export_lists(m, cam, fwd, ("n_contrib",))["n_contrib"].max()


def test_nothing_in_view_leaves_zeros():
    m, cam = scene_model("c")
    fwd = raw_forward(m, cam)
    assert fwd.state[0] == 0
    st = _stats(m, fwds=[fwd], cams=[cam])
    assert st.views == 2 and all(not bool(t.any()) for t in _arrays(st))


def test_morton_order_indexes_storage_rows():
    a, cam = scene_model("a")
    d, _cam = scene_model("a", order="morton")
    assert not torch.equal(d.tie_rank.long().cpu(), torch.arange(d.P))      # the rows really are permuted
    sa, sd = _arrays(_stats(a, cams=[cam])), _arrays(_stats(d, cams=[cam]))
    order = d.original_order().cpu()
    assert same_tensors(sa, [t[order] for t in sd])
    assert bool(sa[0].any())


# ---------------------------------------------------------------------------------------------------- 3. determinism and accumulation
def test_runs_repeat_and_views_accumulate_bit_for_bit():
    from gaussian_lic_amd.camera import synthetic_camera
    m, cam1 = scene_model("a")
    cam2 = synthetic_camera(cr.W_A, cr.H_A, 5).to_device(gpu())
    one, again, two = _arrays(_stats(m, cams=[cam1])), _arrays(_stats(m, cams=[cam1])), _arrays(_stats(m, cams=[cam2]))
    assert same_tensors(one, again)
    assert bool(two[0].any()) and not same_tensors(one, two)
    both = _stats(m, cams=[cam1, cam2])
    got = _arrays(both)
    assert both.views == 2
    assert torch.equal(got[0].view(torch.float32), torch.maximum(one[0].view(torch.float32), two[0].view(torch.float32)))
    assert torch.equal(got[1], one[1] + two[1]) and torch.equal(got[2], one[2] + two[2])
    both.reset()
    assert both.views == 0 and all(not bool(t.any()) for t in _arrays(both))


@pytest.mark.parametrize("name", ["a", "b"])
def test_every_forward_and_binning_path_gives_the_same_statistics(name):
    from gaussian_lic_amd import _lib
    from gaussian_lic_amd.rasterizer import CapacityBuffers
    m, cam = scene_model(name)
    H, W = int(cam.image_height), int(cam.image_width)
    want = _arrays(_stats(m, fwds=[raw_forward(m, cam)]))
    assert bool(want[0].any())
    old = _lib.set_binning_mode("radix")
    try:
        for mode in ("radix", "atomic"):
            _lib.set_binning_mode(mode)
            assert same_tensors(want, _arrays(_stats(m, fwds=[raw_forward(m, cam)]))), mode
    finally:
        _lib.set_binning_mode(old)
    assert same_tensors(want, _arrays(_stats(m, fwds=[raw_forward(m, cam, depth=True)]))), "depth forward"
    for depth in (False, True):
        bufs = CapacityBuffers(m.P, W, H, 4096, 256, gpu(), depth=depth)
        raw_forward(m, cam, depth=depth, bufs=bufs)
        assert bufs.read_status()[2] == 0
        assert same_tensors(want, _arrays(_stats(m, fwds=[bufs]))), f"capacity forward, depth={depth}"


# ---------------------------------------------------------------------------------------------------- 4. capacity mode
def test_capacity_overflow_accumulates_nothing_and_guards_stay():
    from gaussian_lic_amd import rasterizer as rz
    from gaussian_lic_amd.rasterizer import CapacityBuffers
    m, cam = scene_model("a")
    H, W, P = cr.H_A, cr.W_A, m.P
    R = raw_forward(m, cam).state[0]
    for cap_R, fits in ((R // 3, False), (4096, True)):
        bufs = CapacityBuffers(P, W, H, cap_R, 256, gpu())
        raw_forward(m, cam, bufs=bufs)
        assert (bufs.read_status()[2] == 0) == fits
        g = [guarded(P, torch.int32, 7), guarded(P, torch.int32, 7), guarded(P, torch.int64, 7)]
        rz.contribution_accumulate(P, H, W, bufs.cap_R, bufs.cap_B, bufs.geom, bufs.binning, bufs.img, cr.W_MIN, g[0][1], g[1][1], g[2][1])
        torch.cuda.synchronize()
        for whole, _view in g:
            assert bool((whole[:64] == SENTINEL).all()) and bool((whole[64 + P:] == SENTINEL).all())
        changed = [bool((view != 7).any()) for _whole, view in g]
        assert changed == [fits] * 3, (cap_R, changed)
    # any subset of the outputs may be absent
    fwd = raw_forward(m, cam)
    full = _arrays(_stats(m, fwds=[fwd]))
    R, B, _r, geom, binning, img, _s = fwd.state
    only = torch.zeros(P, dtype=torch.int32, device=gpu())
    rz.contribution_accumulate(P, H, W, R, B, geom, binning, img, cr.W_MIN, None, only, None)
    rz.contribution_accumulate(P, H, W, R, B, geom, binning, img, cr.W_MIN, None, None, None)
    assert torch.equal(only.cpu().long(), full[1])


# ---------------------------------------------------------------------------------------------------- 5. rows follow the map
def test_statistics_follow_the_rows_through_prune_extend_resort():
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.synthetic import lidar_scene
    dev = gpu()
    m, cam = scene_model("a", order="morton", capacity=4 * cr.P_A, resort_fraction=None)
    st = _stats(m, cams=[cam])
    old = _arrays(st)
    # drop_mask is the torch expression on the returned arrays
    mask = st.drop_mask(pixels_below=1)
    assert mask.dtype == torch.uint8 and torch.equal(mask.nonzero(), (st.pixels() < 1).nonzero())
    both = st.drop_mask(max_weight_below=0.3, pixels_below=4)
    assert torch.equal(both.nonzero(), ((st.max_weight() < float(np.float32(0.3))) | (st.pixels() < 4)).nonzero())
    assert 0 < int(mask.sum()) < int(both.sum()) < m.P
    assert not bool(st.drop_mask().any())
    # prune: the kept rows' statistics are old[kept]
    detached = _stats(m, cams=[cam])
    detached.detach()
    n, kept = m.prune(drop=mask)
    assert n == int(mask.sum()) and m.P == cr.P_A - n
    assert same_tensors(_arrays(st), [t[kept.cpu()] for t in old]) and st.views == 1
    assert not bool(st._max[m.P:].any()) and not bool(st._npix[m.P:].any()) and not bool(st._sum[m.P:].any())
    with pytest.raises(RuntimeError, match="rows changed"):
        detached.max_weight()
    with pytest.raises(RuntimeError, match="rows changed"):
        detached.accumulate(cam)
    # a fresh accumulate on the pruned map equals the replay on the pruned map
    fwd = raw_forward(m, cam)
    _check_against_replay(_stats(m, fwds=[fwd]), _replay(m, cam, fwd), "scene a, pruned")
    # extend: appended rows are zero, the others stay
    before = _arrays(st)
    P0 = m.P
    frame = lidar_scene(300, cr.W_A, cr.H_A, sh_degree=0, seed=77)
    col = (frame["features_dc"].reshape(-1, 3) * 0.28209479177387814 + 0.5).to(dev)
    Rcw = torch.from_numpy(cam.world_view_transform[:3, :3].T.copy())
    tcw = torch.from_numpy(cam.world_view_transform[3, :3].copy())
    k = m.extend(cam, frame["xyz"].to(dev), col, frame["xyz"][:, 2].contiguous().to(dev), Rcw, tcw, (float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy)))
    assert k > 0 and m.P == P0 + k
    after = _arrays(st)
    assert same_tensors([t[:P0] for t in after], before) and all(not bool(t[P0:].any()) for t in after)
    # ... also when the storage had to grow
    small, _c = scene_model("a")
    st_small = _stats(small, cams=[cam])
    b_small = _arrays(st_small)
    k2 = small.extend(cam, frame["xyz"].to(dev), col, frame["xyz"][:, 2].contiguous().to(dev), Rcw, tcw, (float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy)))
    a_small = _arrays(st_small)
    assert k2 > 0 and small.capacity > cr.P_A and same_tensors([t[:cr.P_A] for t in a_small], b_small) and all(not bool(t[cr.P_A:].any()) for t in a_small)
    # resort: the statistics follow the permutation
    st.accumulate(cam)
    before = _arrays(st)
    stale = trainer.ContributionStats(m)
    stale.detach()
    perm = m.resort().cpu()
    assert not torch.equal(perm, torch.arange(m.P))
    assert same_tensors(_arrays(st), [t[perm] for t in before]) and st.views == 2
    with pytest.raises(RuntimeError, match="rows changed"):
        stale.pixels()


# ---------------------------------------------------------------------------------------------------- 6. the C++ host
def test_fused_contribution_cpp_host(tmp_path):
    """gslic::FusedStep::accumulate_contribution and the statistics carried through gslic::FusedStep::prune give the Python host's arrays bit
    for bit: scene (a) in Morton order, one view, a prune by drop_mask(pixels_below=1), the same view again on the pruned map."""
    exe = fio.build("fused_contribution")
    m, cam = scene_model("a", order="morton")
    d = str(tmp_path)
    w = functools.partial(fio.write, d)
    fio.write_inputs(d, m, cam, tie_rank=m.tie_rank)
    st = _stats(m, cams=[cam])

    def dump(tag):
        mx, npix, sm = _arrays(st)
        w(f"exp{tag}_max", mx.numpy(), np.int32, "i32"); w(f"exp{tag}_npix", npix.numpy().astype(np.uint32).view(np.int32), np.int32, "i32")
        w(f"exp{tag}_sum", sm.numpy(), np.int64, "i64")
    dump(1)
    n, kept = m.prune(drop=st.drop_mask(pixels_below=1))
    assert 0 < n < cr.P_A
    w("exp_kept", kept.cpu().numpy(), np.int32, "i32")
    st.accumulate(cam)
    dump(2)
    r = fio.run(exe, d, str(cr.P_A), str(cr.W_A), str(cr.H_A), "0", repr(cr.W_MIN), "1")
    assert f"contribution check ok rows {cr.P_A} kept {m.P}" in r.stdout
