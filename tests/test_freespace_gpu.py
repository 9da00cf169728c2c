"""-m gpu: free-space statistics (gslic_contribution_accumulate_free_space, trainer.ContributionStats.accumulate(free_space=...), floater_mask,
free_space_bound, gslic::FusedStep::accumulate_free_space).

References, none of them the code under test: the plain and the error-weighted entry points (merged, and held to their own references by
test_contribution_gpu.py / test_densify_gpu.py) for everything that is bit for bit, torch comparisons on the exported float32 depths for the
predicate, torch indexing for everything that moves rows, and the float64 replay of tests/freespace_ref.py for the one toleranced test.  All
forwards run in strict arithmetic.  Scenes a, b, c and the Morton twin d: contribution_ref.scene."""
import functools

import numpy as np
import pytest
import torch

import contribution_ref as cr
import freespace_ref as fr
import fused_check_io as fio
from gpu_helpers import SENTINEL, bits, export_lists, gpu, guarded, raw_forward, same_tensors, scene_model

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")


def _const(fwd_or_hw, value):
    H, W = fwd_or_hw if isinstance(fwd_or_hw, tuple) else fwd_or_hw.hw
    return torch.full((int(H), int(W)), float(value), device=gpu())


def _five(m, fwd, near=None, error=None):
    """(max_w bits, n_pix, sum_w, free_sum, meas_sum) of one view as CPU tensors through ContributionStats; with `error` a sixth: err_sum."""
    from gaussian_lic_amd import trainer
    st = trainer.ContributionStats(m)
    st.accumulate_from(fwd, cr.W_MIN, error=error, free_space=near)
    torch.cuda.synchronize()
    out = [st.max_weight().view(torch.int32).cpu().clone(), st.pixels().cpu().clone(), st.sum_fixed().cpu().clone(), st.free_fixed().cpu().clone(),
           st.measured_fixed().cpu().clone()]
    if error is not None:
        out.append(st.error_fixed().cpu().clone())
    assert st.views == 1
    st.detach()
    return out


@pytest.fixture(scope="module")
def views():
    """Per scene: the model, the camera, one plain forward, the plain entry point's arrays and the exported float32 depths — computed once, left
    unchanged."""
    out = {}
    for name in ("a", "b"):
        m, cam = scene_model(name)
        fwd = raw_forward(m, cam)
        z = export_lists(m, cam, fwd, ("depths",))["depths"].cpu().clone()
        out[name] = (m, cam, fwd, _five(m, fwd), z)
    return out


# ---------------------------------------------------------------------------------------------------- 1. bit for bit against the merged entry points
@pytest.mark.parametrize("name", ["a", "b"])
def test_constant_bounds(views, name):
    m, _cam, fwd, plain, _z = views[name]
    assert bool(plain[2].any()) and not bool(plain[3].any()) and not bool(plain[4].any())       # zeros before the first use
    inf = _five(m, fwd, _const(fwd, INF))
    assert torch.equal(inf[3], inf[2]) and torch.equal(inf[4], inf[2])                           # +inf: free == meas == sum_w, bits
    assert same_tensors(inf[:3], plain[:3])                                                             # the base three: the plain entry point's bits
    for v in (0.0, NAN, -1.0):
        got = _five(m, fwd, _const(fwd, v))
        assert not bool(got[3].any()) and not bool(got[4].any()), v
        assert same_tensors(got[:3], plain[:3]), v
    tiny = _five(m, fwd, _const(fwd, 1e-30))                                                     # measured, and in front of everything
    assert torch.equal(tiny[4], plain[2]) and not bool(tiny[3].any()) and same_tensors(tiny[:3], plain[:3])


@pytest.mark.parametrize("name", ["a", "b"])
def test_the_comparison_is_strict(views, name):
    m, _cam, fwd, plain, z = views[name]
    vis = (plain[2] != 0).nonzero().squeeze(1)
    zs = z[vis]
    g = int(vis[torch.argsort(zs)[vis.numel() // 2]])                                            # a visible Gaussian of median depth
    z0 = z[g].clone()
    at = _five(m, fwd, _const(fwd, float(z0)))
    assert float(torch.tensor(float(z0), dtype=torch.float32)) == float(z0)
    front = z < z0                                                                               # float32 < float32, as the kernel compares
    assert bool(front[vis].any()) and bool((~front)[vis].any())
    assert int(at[3][g]) == 0 and torch.equal(at[4], plain[2])
    assert torch.equal(at[3][front], plain[2][front]) and not bool(at[3][~front].any())
    nxt = float(np.nextafter(np.float32(z0), np.float32(np.inf)))
    up = _five(m, fwd, _const(fwd, nxt))
    assert int(up[3][g]) == int(plain[2][g]) != 0
    assert torch.equal(up[3][z < nxt], plain[2][z < nxt])


def _mask_images(H, W, busiest):
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    checker = ((yy + xx) % 2 == 0)
    single = torch.zeros(H, W, dtype=torch.bool); single.view(-1)[busiest] = True                # the pixel with the longest list of contributors
    last_col = torch.zeros(H, W, dtype=torch.bool); last_col[:, W - 1] = True                    # scene (a): the partial tile column's last pixel
    return {"checkerboard": checker, "single pixel": single, "last column": last_col}


@pytest.mark.parametrize("name", ["a", "b"])
def test_zero_inf_masks_equal_the_error_entry_point(views, name):
    m, cam, fwd, plain, _z = views[name]
    H, W = fwd.hw
    busiest = int(export_lists(m, cam, fwd, ("n_contrib",))["n_contrib"].reshape(-1).argmax())
    for kind, mask in _mask_images(int(H), int(W), busiest).items():
        near = torch.where(mask, torch.tensor(INF), torch.tensor(0.0)).to(gpu())
        got = _five(m, fwd, near)
        err = _five(m, fwd, None, error=mask.float().to(gpu()))[5]
        assert torch.equal(got[3], err) and torch.equal(got[4], err), kind
        assert same_tensors(got[:3], plain[:3]), kind
        assert bool(err.any()) and not torch.equal(err, plain[2]), kind


def test_guard_words_and_absent_base_outputs(views):
    from gaussian_lic_amd import rasterizer as rz
    m, _cam, fwd, plain, _z = views["a"]
    P, (H, W) = m.P, fwd.hw
    R, B, _r, geom, binning, img, _s = fwd.state
    near = fr.bound_image("a").to(gpu())
    want = _five(m, fwd, near)
    g = [guarded(P, torch.int32, 0), guarded(P, torch.int32, 0), guarded(P, torch.int64, 0), guarded(P, torch.int64, 0), guarded(P, torch.int64, 0)]
    rz.contribution_accumulate(P, H, W, R, B, geom, binning, img, cr.W_MIN, g[0][1], g[1][1], g[2][1], near_bound=near, free_sum=g[3][1], meas_sum=g[4][1])
    torch.cuda.synchronize()
    for whole, _v in g:
        assert bool((whole[:64] == SENTINEL).all()) and bool((whole[64 + P:] == SENTINEL).all())
    assert torch.equal(g[0][1].cpu(), plain[0]) and torch.equal(g[1][1].cpu().long() & 0xffffffff, plain[1]) and torch.equal(g[2][1].cpu(), plain[2])
    assert torch.equal(g[3][1].cpu(), want[3]) and torch.equal(g[4][1].cpu(), want[4]) and bool(want[3].any())
    assert not torch.equal(want[3], want[4]) and not torch.equal(want[4], plain[2])
    # the base three all absent: the two sums are still accumulated
    f2, m2 = torch.zeros(P, dtype=torch.int64, device=gpu()), torch.zeros(P, dtype=torch.int64, device=gpu())
    rz.contribution_accumulate(P, H, W, R, B, geom, binning, img, cr.W_MIN, None, None, None, near_bound=near, free_sum=f2, meas_sum=m2)
    assert torch.equal(f2.cpu(), want[3]) and torch.equal(m2.cpu(), want[4])
    # any one of them absent
    only = torch.zeros(P, dtype=torch.int32, device=gpu())
    f3, m3 = torch.zeros_like(f2), torch.zeros_like(m2)
    rz.contribution_accumulate(P, H, W, R, B, geom, binning, img, cr.W_MIN, None, only, None, near_bound=near, free_sum=f3, meas_sum=m3)
    assert torch.equal(only.cpu().long(), plain[1]) and torch.equal(f3.cpu(), want[3]) and torch.equal(m3.cpu(), want[4])


def test_runs_repeat_and_views_add_as_integers(views):
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    m, cam1, fwd, _plain, _z = views["a"]
    cam2 = synthetic_camera(cr.W_A, cr.H_A, 5).to_device(gpu())
    near = fr.bound_image("a").to(gpu())
    one, again = _five(m, fwd, near), _five(m, fwd, near)
    assert same_tensors(one, again) and bool(one[3].any())
    two = _five(m, raw_forward(m, cam2), near)
    assert not torch.equal(one[3], two[3]) and not torch.equal(one[4], two[4])
    st = trainer.ContributionStats(m)
    st.accumulate(cam1, w_min=cr.W_MIN, free_space=near)
    st.accumulate(cam2, w_min=cr.W_MIN, free_space=near)
    assert st.views == 2
    assert torch.equal(st.free_fixed().cpu(), one[3] + two[3]) and torch.equal(st.measured_fixed().cpu(), one[4] + two[4])
    assert torch.equal(st.sum_fixed().cpu(), one[2] + two[2]) and torch.equal(st.pixels().cpu(), one[1] + two[1])
    assert torch.equal(st.free_weight().cpu(), trainer.fixed_to_weight(one[3] + two[3]))
    assert torch.equal(st.measured_weight().cpu(), trainer.fixed_to_weight(one[4] + two[4]))
    st.reset()
    assert st.views == 0 and not bool(st.free_fixed().any()) and not bool(st.measured_fixed().any())
    st.detach()


@pytest.mark.parametrize("name", ["a", "b"])
def test_every_forward_and_binning_path_gives_the_same_sums(views, name):
    from gaussian_lic_amd import _lib
    from gaussian_lic_amd.rasterizer import CapacityBuffers
    m, cam, fwd, _plain, _z = views[name]
    H, W = fwd.hw
    near = fr.bound_image(name).to(gpu())
    want = _five(m, fwd, near)
    assert bool(want[3].any())
    old = _lib.set_binning_mode("radix")
    try:
        for mode in ("radix", "atomic"):
            _lib.set_binning_mode(mode)
            assert same_tensors(want, _five(m, raw_forward(m, cam), near)), mode
    finally:
        _lib.set_binning_mode(old)
    assert same_tensors(want, _five(m, raw_forward(m, cam, depth=True), near)), "depth forward"
    for depth in (False, True):
        bufs = CapacityBuffers(m.P, W, H, 4096, 256, gpu(), depth=depth)
        raw_forward(m, cam, depth=depth, bufs=bufs)
        assert bufs.read_status()[2] == 0 and same_tensors(want, _five(m, bufs, near)), f"capacity forward, depth={depth}"
    small = CapacityBuffers(m.P, W, H, max(fwd.state[0] // 3, 1), 256, gpu())                   # the lists do not fit: nothing is touched
    raw_forward(m, cam, bufs=small)
    assert small.read_status()[2] != 0 and not any(bool(t.any()) for t in _five(m, small, near))


def test_nothing_in_view_leaves_zeros():
    m, cam = scene_model("c")
    fwd = raw_forward(m, cam)
    assert fwd.state[0] == 0
    assert not any(bool(t.any()) for t in _five(m, fwd, _const(fwd, INF)))


def test_both_row_orders_give_the_same_statistics(views):
    a, cam, fwd, _plain, _z = views["a"]
    d, _cam = scene_model("a", order="morton")
    assert not torch.equal(d.tie_rank.long().cpu(), torch.arange(d.P))                           # the rows really are permuted
    near = fr.bound_image("a").to(gpu())
    sa, sd = _five(a, fwd, near), _five(d, raw_forward(d, cam), near)
    order = d.original_order().cpu()
    assert same_tensors(sa, [t[order] for t in sd]) and bool(sa[3].any())


def test_both_images_in_one_call(views):
    from gaussian_lic_amd import trainer
    m, cam, fwd, plain, _z = views["a"]
    near = fr.bound_image("a").to(gpu())
    err = (2.0 * torch.rand(cr.H_A, cr.W_A, generator=torch.Generator().manual_seed(41))).to(gpu())
    free_only, err_only = _five(m, fwd, near), _five(m, fwd, None, error=err)
    both = _five(m, fwd, near, error=err)                                                        # (_five asserts views == 1)
    assert same_tensors(both[:3], plain[:3])                                                            # nothing is counted twice
    assert torch.equal(both[3], free_only[3]) and torch.equal(both[4], free_only[4]) and torch.equal(both[5], err_only[5])
    st = trainer.ContributionStats(m)
    st.accumulate(cam, w_min=cr.W_MIN, error=err, free_space=near)
    assert st.views == 1 and torch.equal(st.sum_fixed().cpu(), plain[2]) and torch.equal(st.free_fixed().cpu(), free_only[3])
    with pytest.raises(ValueError, match="free_space must be a float"):
        st.accumulate(cam, free_space=near[:, :-1])
    with pytest.raises(ValueError, match="free_space must be a float"):
        st.accumulate(cam, free_space=near.cpu())
    with pytest.raises(ValueError, match="free_space must be a float"):
        st.accumulate(cam, free_space=near.long())
    assert st.views == 1
    st.detach()


# ---------------------------------------------------------------------------------------------------- 2. the float64 replay (the one toleranced test)
@pytest.mark.parametrize("name", ["a", "b"])
def test_random_bound_against_the_float64_replay(views, name):
    """Measured on one MI355X (this test's own line): see freespace_ref.FREE_GAP_A / FREE_GAP_B; the bar FREE_MARGIN is 4x the larger."""
    from gaussian_lic_amd import trainer
    m, cam, fwd, _plain, z = views[name]
    H, W = fwd.hw
    near = fr.bound_image(name)
    got = _five(m, fwd, near.to(gpu()))
    d = export_lists(m, cam, fwd, ("means2D", "conic_opacity", "point_list", "ranges", "n_contrib"))
    n = lambda k: d[k].cpu().numpy()
    rep = fr.replay(n("means2D"), n("conic_opacity"), n("point_list"), n("ranges"), n("n_contrib"), W, H, m.P, z.numpy(), near.numpy())
    shares = fr.class_shares(rep)
    g_free = fr.max_gap(trainer.fixed_to_weight(got[3]).numpy(), rep["free_sum"])
    g_meas = fr.max_gap(trainer.fixed_to_weight(got[4]).numpy(), rep["meas_sum"])
    print(f"[freespace gap] scene {name}: free_sum {g_free:.3e} meas_sum {g_meas:.3e} relative to the maxima {rep['free_sum'].max():.4f} / "
          f"{rep['meas_sum'].max():.4f} (bar {fr.FREE_MARGIN}); classes unmeasured {shares[0]:.3f} in front {shares[1]:.3f} not in front {shares[2]:.3f}")
    assert bool((shares >= fr.MIN_CLASS_SHARE).all())                                            # the condition test_freespace_cpu.py asserts on the oracle's lists
    assert rep["free_sum"].max() > 0.5 and rep["meas_sum"].max() > 0.5
    assert bool(((rep["free_sum"] > 0) == (got[3].numpy() != 0)).all()) and bool(((rep["meas_sum"] > 0) == (got[4].numpy() != 0)).all())
    assert bool((got[3] <= got[4]).all()) and bool((got[4] <= got[2]).all())                     # (all below 2^63: signed order is the unsigned one)
    assert max(g_free, g_meas) <= 1e-5                                                           # above this it is a bug, not a margin
    assert g_free <= fr.FREE_MARGIN and g_meas <= fr.FREE_MARGIN


# ---------------------------------------------------------------------------------------------------- 3. rows follow the map
NP, W, H = 2000, 64, 48


def _trained(order, steps=1, **kw):
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import gt_image, random_scene
    dev = gpu()
    m = trainer.GaussianModel(random_scene(NP, W, H, sh_degree=3, seed=3), dev, order=order, **kw)
    m.training_setup()
    cam = synthetic_camera(W, H).to_device(dev)
    gt, bg = gt_image(H, W).to(dev), torch.zeros(3, device=dev)
    for _ in range(steps):
        trainer.training_step_fused(m, cam, gt, bg)
    return m, cam, gt, bg


def _near_for(cam, m, seed=7):
    """A bound image that splits the map: uniform over the map's depth range, a quarter of the pixels unmeasured."""
    g = torch.Generator().manual_seed(seed)
    near = 1.0 + 29.0 * torch.rand(H, W, generator=g)
    near[torch.rand(H, W, generator=g) < 0.25] = 0.0
    return near.to(gpu())


def test_attached_statistics_follow_prune_extend_densify_resort():
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.synthetic import lidar_scene
    dev = gpu()
    m, cam, gt, bg = _trained("morton", capacity=3 * NP, resort_fraction=None)
    near = _near_for(cam, m)
    st = trainer.ContributionStats(m)
    st.accumulate(cam, free_space=near)
    arrays = lambda: [st._max[:m.P].clone(), st._npix[:m.P].clone(), st._sum[:m.P].clone(), st._free[:m.P].clone(), st._meas[:m.P].clone()]
    old = arrays()
    assert all(bool(t.any()) for t in old) and not torch.equal(old[3], old[4]) and [w for _a, w in st._arrays()] == [1, 1, 2, 2, 2]
    loose = trainer.ContributionStats(m)
    loose.detach()
    # densify: zeros for the new rows and the split parents, the others stay
    grow = (st.measured_fixed() > 0) & (torch.rand(NP, generator=torch.Generator().manual_seed(1)).to(dev) < 0.2)
    s = float(torch.exp(m.scaling.detach().double()).max(1).values.median())
    was_split = grow & (m._buf["scaling"][:NP] > trainer.densify_threshold(s)).any(1)
    k, n_split, _parents = m.densify(grow, s)
    assert 0 < n_split == int(was_split.sum()) < k == int(grow.sum()) and m.P == NP + k
    for o, n in zip(old, arrays()):
        assert not bool(n[NP:].any()) and not bool(n[:NP][was_split].any()) and torch.equal(n[:NP][~was_split], o[~was_split])
    with pytest.raises(RuntimeError, match="rows changed"):
        loose.free_fixed()
    with pytest.raises(RuntimeError, match="rows changed"):
        loose.floater_mask(0.5)
    # resort: the permutation
    st.accumulate(cam, free_space=near)
    before = arrays()
    perm = m.resort()
    assert not torch.equal(perm.cpu(), torch.arange(m.P))
    assert same_tensors(arrays(), [t[perm] for t in before]) and st.views == 2
    # prune by the floater mask: the kept rows
    before = arrays()
    mask = st.floater_mask(0.5, min_measured=0.01)
    assert torch.equal(mask, trainer.contribution_floater_mask(st.free_fixed(), st.measured_fixed(), 0.5, 0.01)) and 0 < int(mask.sum()) < m.P
    removed, kept = m.prune(drop=mask)
    assert removed == int(mask.sum())
    assert same_tensors(arrays(), [t[kept] for t in before])
    assert not bool(st._free[m.P:].any()) and not bool(st._meas[m.P:].any())
    # extend: appended rows are zero
    before, P0 = arrays(), m.P
    frame = lidar_scene(300, W, H, sh_degree=3, seed=77)
    col = (frame["features_dc"].reshape(-1, 3) * 0.28209479177387814 + 0.5).to(dev)
    Rcw = torch.from_numpy(cam.world_view_transform[:3, :3].T.copy())
    tcw = torch.from_numpy(cam.world_view_transform[3, :3].copy())
    u_pix = m.xyz.detach()[:, 0] * (0.675 * W) / m.xyz.detach()[:, 2].abs().clamp_min(0.2) + 0.4857 * W
    _r, kept2 = m.prune(drop=u_pix > 0.5 * W)                                                    # room in the right half for LiDAR points
    before = [t[kept2] for t in before]
    P0 = m.P
    k3 = m.extend(cam, frame["xyz"].to(dev), col, frame["xyz"][:, 2].contiguous().to(dev), Rcw, tcw, (float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy)))
    assert k3 > 0 and m.P == P0 + k3
    after = arrays()
    assert same_tensors([t[:P0] for t in after], before) and all(not bool(t[P0:].any()) for t in after)
    st.reset()
    assert not any(bool(t.any()) for t in arrays())


# ---------------------------------------------------------------------------------------------------- 4. end to end
def _wall_scene():
    """A tilted wall of Gaussians at depth ~8 (one per 4 x 4 pixels, identity camera), its LiDAR points (one per pixel centre), and FLOATERS:
    copies of twelve wall rows moved to 40 % of their depth along their rays (scaled with it: the same footprint on the screen)."""
    fx, cx, cy = 0.675 * W, 0.4857 * W, 0.5215 * H
    depth = lambda u: 8.0 + 0.01 * u
    vv, uu = torch.meshgrid(torch.arange(2.0, H, 4.0), torch.arange(2.0, W, 4.0), indexing="ij")
    u, v = uu.reshape(-1), vv.reshape(-1)
    z = depth(u)
    xyz = torch.stack([(u - cx) * z / fx, (v - cy) * z / fx, z], 1)
    n_wall = xyz.shape[0]
    inner = ((u > 12) & (u < W - 12) & (v > 10) & (v < H - 10)).nonzero().squeeze(1)
    parents = inner[torch.linspace(0, inner.numel() - 1, 12).long()]
    xyz = torch.cat([xyz, 0.4 * xyz[parents]])
    P = xyz.shape[0]
    sig = torch.cat([2.0 * z / fx, 0.4 * 2.0 * z[parents] / fx])
    g = torch.Generator().manual_seed(4)
    raw = dict(xyz=xyz.float().contiguous(), scaling=torch.log(sig).unsqueeze(1).repeat(1, 3).float().contiguous(),
               rotation=torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(P, 1).contiguous(), opacity=torch.full((P, 1), 1.5),
               features_dc=((torch.rand(P, 1, 3, generator=g) - 0.5) / 0.28209479).float().contiguous(), features_rest=torch.zeros(P, 15, 3), sh_degree=3)
    pv, pu = torch.meshgrid(torch.arange(H) + 0.5, torch.arange(W) + 0.5, indexing="ij")
    pu, pv = pu.reshape(-1), pv.reshape(-1)
    pz = depth(pu)
    points = torch.stack([(pu - cx) * pz / fx, (pv - cy) * pz / fx, pz], 1).float()
    return raw, points, n_wall


def test_planted_floaters_are_found_and_pruned_and_training_goes_on():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import gt_image
    dev = gpu()
    raw, points, n_wall = _wall_scene()
    m = trainer.GaussianModel(raw, dev)
    m.training_setup()
    P = m.P
    st = trainer.ContributionStats(m)
    for view in (None, 3):
        cam = synthetic_camera(W, H, view).to_device(dev)
        d = cam.project_depth(points.to(dev))
        near = trainer.free_space_bound(d, 0.1, 0.02)
        assert float((d > 0).float().mean()) > 0.4 and bool(((near > 0) == (d > 0)).all()) and bool((near <= d).all())
        st.accumulate(cam, free_space=near)
    assert st.views == 2
    planted = torch.zeros(P, dtype=torch.bool, device=dev)
    planted[n_wall:] = True
    frac = st.free_weight() / st.measured_weight().clamp_min(1e-30)
    print(f"[freespace end to end] wall rows {n_wall} floaters {P - n_wall}: free fraction of the wall max {float(frac[:n_wall].max()):.3f}, "
          f"of the floaters min {float(frac[n_wall:].min()):.3f}; measured weight of the floaters min {float(st.measured_weight()[n_wall:].min()):.3f}")
    mask = st.floater_mask(0.5)
    assert torch.equal(mask.bool(), planted)
    removed, kept = m.prune(drop=mask)
    assert removed == P - n_wall and torch.equal(kept, torch.arange(n_wall, device=dev))
    assert not bool(st.free_fixed().any()) and bool(st.measured_fixed().any())
    cam = synthetic_camera(W, H).to_device(dev)
    gt, bg = gt_image(H, W).to(dev), torch.zeros(3, device=dev)
    for _ in range(2):
        terms, _ = trainer.training_step_fused(m, cam, gt, bg)
        assert bool(torch.isfinite(terms).all())
    assert all(bool(torch.isfinite(m._buf[n][:m.P]).all()) for n in m.NAMES)


# ---------------------------------------------------------------------------------------------------- 5. the C++ host
def test_fused_free_space_cpp_host(tmp_path, monkeypatch):
    """gslic::FusedStep::accumulate_free_space, the floater rule computed in C++, prune(drop = mask) and resort() with the statistics handed
    along give the Python host's result bit for bit: the five accumulators, the mask, the kept index, the permutation and all 19 arrays."""
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import gt_image, random_scene
    exe = fio.build("fused_free_space")
    monkeypatch.delenv("GSLIC_RESORT", raising=False)
    dev = gpu()
    cam1, cam2 = synthetic_camera(W, H).to_device(dev), synthetic_camera(W, H, 5).to_device(dev)
    gt, bg = gt_image(H, W).to(dev), torch.zeros(3, device=dev)
    iters, w_min, fraction, min_measured = 2, trainer.ContributionStats.W_MIN, 0.6, 0.05
    m = trainer.GaussianModel(random_scene(NP, W, H, sh_degree=3, seed=9), dev)
    m.training_setup()
    d = str(tmp_path)
    near1, near2 = _near_for(cam1, m, 7), _near_for(cam2, m, 8)
    fio.write_inputs(d, m, (cam1, cam2), gt=gt, near1=near1, near2=near2)

    def steps():
        for _ in range(iters):
            trainer.training_step_fused(m, cam1, gt, bg)
    steps()
    st = trainer.ContributionStats(m)
    st.accumulate(cam1, w_min=w_min, free_space=near1)
    st.accumulate(cam2, w_min=w_min, free_space=near2)
    mask = st.floater_mask(fraction, min_measured)
    removed, kept = m.prune(drop=mask)
    assert 0 < removed < NP
    st.accumulate(cam1, w_min=w_min, free_space=near1)
    perm = m.to_morton_order(resort_fraction=None)
    steps()
    r = fio.run(exe, d, str(NP), str(W), str(H), "3", str(iters), repr(w_min), repr(fraction), repr(min_measured))
    assert f"free space pruned {removed} size {m.P}" in r.stdout
    rd = functools.partial(fio.read, d)
    P = m.P
    assert torch.equal(rd("mask.u8", np.uint8), mask.cpu()) and torch.equal(rd("kept.i64", np.int64), kept.cpu()) and torch.equal(rd("perm.i64", np.int64), perm.cpu())
    assert torch.equal(rd("max_w.i32", np.int32), st._max[:P].cpu()) and torch.equal(rd("n_pix.i32", np.int32), st._npix[:P].cpu())
    assert torch.equal(rd("sum_w.i64", np.int64), st.sum_fixed().cpu())
    assert torch.equal(rd("free_sum.i64", np.int64), st.free_fixed().cpu()) and torch.equal(rd("meas_sum.i64", np.int64), st.measured_fixed().cpu())
    assert bool(st.free_fixed().any()) and st.views == 3
    for n, f in (("xyz", "xyz"), ("features_dc", "dc"), ("features_rest", "rest"), ("opacity", "opacity"), ("scaling", "scaling"), ("rotation", "rotation")):
        for pre, src in (("", m._buf), ("m_", m._m), ("v_", m._v)):
            assert torch.equal(rd(pre + f + ".f32", np.int32), bits(src[n][:P]).cpu().reshape(-1)), pre + f
    assert torch.equal(rd("tie.i32", np.int32), m.tie_rank.cpu())
