"""-m gpu: pruning the map on the device — gslic_prune_select (which rows stay), gslic_gather_rows (one-launch compaction of every per-row
array), trainer.GaussianModel.prune on both row orders, GraphedStep's stale-layout error and the C++ host's gslic::FusedStep::prune.

The reference of every comparison is plain torch on the same tensors (x[keep_mask], x[index]), never the code under test; every comparison is
exact (indices, or int32 views of the rows, so NaN payloads count)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import fused_check_io as fio
from gpu_helpers import SENTINEL, bits, gpu, map_snapshot

pytestmark = pytest.mark.gpu

SCAN_TILE = 256 * 16       # elements one workgroup of scan_u32 covers (scan.hip: SCAN_THREADS x SCAN_ITEMS)
SHAPES = [1, 63, 64, 65, 257, SCAN_TILE + 1, 100003]
PATTERNS = ["all", "none", "first", "last", "alternating", "random30"]


def _libs():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    return _lib, _lib.lib()


def _thresholds():
    from gaussian_lic_amd.trainer import prune_thresholds
    return prune_thresholds(0.05, 3.0)


def _pattern(name, P):
    i = torch.arange(P)
    if name == "all":
        return torch.ones(P, dtype=torch.bool)
    if name == "none":
        return torch.zeros(P, dtype=torch.bool)
    if name == "first":
        return i == 0
    if name == "last":
        return i == P - 1
    if name == "alternating":
        return (i % 2) == 0
    g = torch.Generator().manual_seed(1000 + P)
    return torch.rand(P, generator=g) < 0.3


def _rows_for(keep, extras):
    """Raw parameter rows (CPU) whose keep mask under the rule is exactly `keep`.  Kept rows include rows AT either threshold (strict < and >);
    removed rows sit one float32 step beyond a threshold.  extras: some removed rows are hit through `drop` alone, and some kept rows are hit
    (well below the opacity threshold) but protected.  Returns (tensors, drop, protect)."""
    lo, hi = _thresholds()
    P = keep.numel()
    g = torch.Generator().manual_seed(7 * P + int(extras))
    i = torch.arange(P)
    t = dict(xyz=torch.randn(P, 3, generator=g), dc=torch.randn(P, 3, generator=g), rotation=torch.randn(P, 4, generator=g),
             opacity=lo + 0.5 + torch.rand(P, generator=g), scaling=hi - 0.5 - torch.rand(P, 3, generator=g))
    t["opacity"][keep & (i % 4 == 1)] = lo                          # AT the threshold: stays
    t["scaling"][keep & (i % 4 == 2), 1] = hi
    just_below = float(np.nextafter(np.float32(lo), np.float32(-np.inf)))
    just_above = float(np.nextafter(np.float32(hi), np.float32(np.inf)))
    gone = ~keep
    drop = protect = None
    by_opacity, by_scale = gone & (i % 2 == 0), gone & (i % 2 == 1)
    if extras:
        by_drop = gone & (i % 3 == 2)
        by_opacity, by_scale = by_opacity & ~by_drop, by_scale & ~by_drop
        drop = by_drop.to(torch.uint8)
        saved = keep & (i % 5 == 0)
        t["opacity"][saved] = lo - 1.0                              # hit, but protected
        protect = (saved | (keep & (i % 7 == 0))).to(torch.uint8)
    t["opacity"][by_opacity] = just_below
    for j in range(3):
        t["scaling"][by_scale & (i % 3 == j), j] = just_above
    return t, drop, protect


def _keep_mask(t, lo, hi, drop_nonfinite=True, drop=None, protect=None):
    """The rule of include/gslic_hip.h in torch, on the same tensors and the same float32 thresholds."""
    P = t["opacity"].shape[0]
    bad = torch.zeros(P, dtype=torch.bool, device=t["opacity"].device)
    if drop_nonfinite:
        for k in ("xyz", "dc", "opacity", "scaling", "rotation"):
            bad |= ~torch.isfinite(t[k].reshape(P, -1)).all(1)
    hit = (t["opacity"].reshape(P) < lo) | (t["scaling"] > hi).any(1)
    if drop is not None:
        hit |= drop.bool()
    ok = ~hit
    if protect is not None:
        ok |= protect.bool()
    return ~bad & ok


def _select(t, lo, hi, drop_nonfinite=True, drop=None, protect=None, tie=None, split=0):
    _l, L = _libs()
    P = t["opacity"].shape[0]
    dev = t["opacity"].device
    kept = torch.full((P,), -1, dtype=torch.int32, device=dev)
    new_tie = torch.full((P,), -1, dtype=torch.int32, device=dev) if tie is not None else None
    scratch = _l.TensorAllocator(dev)
    count, below = ctypes.c_int32(-1), ctypes.c_int32(-1)
    p = _l.ptr
    _l.check(L.gslic_prune_select(P, p(t["xyz"]), p(t["dc"]), p(t["opacity"]), p(t["scaling"]), p(t["rotation"]), lo, hi, int(drop_nonfinite), p(drop),
                                  p(protect), p(tie), int(split), scratch.cb, None, p(kept), p(new_tie), ctypes.byref(count), ctypes.byref(below),
                                  _l.current_stream_ptr()))
    n = count.value
    assert bool((kept[n:] == -1).all()) and (new_tie is None or bool((new_tie[n:] == -1).all()))   # nothing is written behind the count
    return kept[:n].long(), (None if new_tie is None else new_tie[:n].long()), n, below.value


def _to(t, dev):
    return {k: v.to(dev).contiguous() for k, v in t.items()}


# ---------------------------------------------------------------------------------------------------- 1 + 2. selection and dense ties
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("P", SHAPES)
def test_selection_is_exact_and_ties_stay_dense(P, pattern):
    dev = gpu()
    lo, hi = _thresholds()
    keep = _pattern(pattern, P)
    g = torch.Generator().manual_seed(31 * P)
    for extras in (False, True):
        rows, drop, protect = _rows_for(keep, extras)
        t = _to(rows, dev)
        drop = None if drop is None else drop.to(dev)
        protect = None if protect is None else protect.to(dev)
        tie = torch.randperm(P, generator=g).to(torch.int32).to(dev) if extras else None
        mask = _keep_mask(t, lo, hi, True, drop, protect)
        assert torch.equal(mask.cpu(), keep)                       # (the rows were built for this pattern: the torch rule agrees)
        want = mask.nonzero().squeeze(1)
        for split in (0, 1, P // 2, P):
            kept, new_tie, count, below = _select(t, lo, hi, True, drop, protect, tie, split)
            assert count == int(mask.sum()) and torch.equal(kept, want), (P, pattern, extras, split)
            assert below == int(mask[:split].sum()), (P, pattern, extras, split, below)
            if tie is not None:
                assert torch.equal(torch.sort(new_tie).values, torch.arange(count, device=dev))                  # a permutation of 0..count-1
                assert torch.equal(torch.argsort(new_tie), torch.argsort(tie.long()[kept]))                      # ... in the old relative order


@pytest.mark.parametrize("which", ["xyz", "dc", "opacity", "scaling", "rotation"])
def test_nonfinite_rows_go_even_when_protected(which):
    dev = gpu()
    lo, hi = _thresholds()
    P = 257
    rows, _d, _p = _rows_for(torch.ones(P, dtype=torch.bool), False)
    flat = rows[which].reshape(P, -1)
    w = flat.shape[1]
    poison = {5: math.inf, 64: -math.inf, 130: math.nan, 256: math.nan}
    for k, (r, v) in enumerate(poison.items()):
        flat[r, k % w] = v
    t = _to(rows, dev)
    protect = torch.zeros(P, dtype=torch.uint8, device=dev)
    protect[130] = 1                                               # protected and non-finite: still removed
    protect[7] = 1
    mask = _keep_mask(t, lo, hi, True, None, protect)
    assert int(mask.sum()) == P - 4 and not bool(mask[130])
    kept, _nt, count, below = _select(t, lo, hi, True, None, protect, None, 131)
    assert torch.equal(kept, mask.nonzero().squeeze(1)) and count == P - 4 and below == int(mask[:131].sum())
    # drop_nonfinite = 0: only the comparisons decide (a NaN compares false; -inf opacity is below any threshold, +inf scaling above)
    mask0 = _keep_mask(t, lo, hi, False, None, protect)
    kept0, _nt, count0, _b = _select(t, lo, hi, False, None, protect, None, 0)
    assert torch.equal(kept0, mask0.nonzero().squeeze(1)) and count0 == int(mask0.sum()) and count0 > count
    # thresholds disabled and nothing non-finite to drop: everything stays
    kept1, _nt, count1, below1 = _select(t, -math.inf, math.inf, False, None, None, None, P)
    assert count1 == P and below1 == P and torch.equal(kept1, torch.arange(P, device=dev))


# ---------------------------------------------------------------------------------------------------- 3. the gather
def _sources(P, M):
    """The map's 19 row arrays as random BIT patterns (int32 views; NaN payloads included): 6 groups x {parameter, exp_avg, exp_avg_sq} + tie_rank."""
    dev = gpu()
    g = torch.Generator(device=dev).manual_seed(P + 17 * M)
    widths = [3, 3, 3 * M, 1, 3, 4] * 3 + [1]
    return [torch.randint(-2 ** 31, 2 ** 31 - 1, (P, w), dtype=torch.int64, device=dev, generator=g).to(torch.int32) for w in widths]


def _gather(srcs, index, cap):
    _l, L = _libs()
    dsts = [torch.full((cap, s.shape[1]), SENTINEL, dtype=torch.int32, device=s.device) for s in srcs]
    arr = (_l.RowArray * len(srcs))(*[_l.RowArray(s.data_ptr() if s.numel() else None, d.data_ptr() if d.numel() else None, s.shape[1])
                                      for s, d in zip(srcs, dsts)])
    idx = index.to(torch.int32).contiguous()
    _l.check(L.gslic_gather_rows(arr, len(srcs), _l.ptr(idx), int(idx.numel()), _l.current_stream_ptr()))
    return dsts


def _check_gather(srcs, index, cap):
    n = int(index.numel())
    for k, (s, d) in enumerate(zip(srcs, _gather(srcs, index, cap))):
        assert torch.equal(d[:n], s[index]), (k, s.shape)
        assert bool((d[n:] == SENTINEL).all()), (k, "rows behind n_rows were written")


@pytest.mark.parametrize("M", [15, 0])
@pytest.mark.parametrize("P", SHAPES)
def test_gather_is_exact(P, M):
    dev = gpu()
    srcs = _sources(P, M)
    for pattern in PATTERNS:
        index = _pattern(pattern, P).nonzero().squeeze(1).to(dev)          # ("none": n_rows = 0 returns at once, nothing is written)
        _check_gather(srcs, index, P)
    g = torch.Generator().manual_seed(P)
    _check_gather(srcs, torch.randperm(P, generator=g).to(dev), P)         # a full permutation: the shape of resort()


def test_gather_other_widths_and_more_arrays_than_one_launch_takes():
    """Widths without a compile-time divisor (2, 9, 4096 = one workgroup's chunk exactly), a row wider than a chunk (5000 dwords: the lanes walk
    the row), and 40 arrays (two launches of at most 32)."""
    dev = gpu()
    g = torch.Generator(device=dev).manual_seed(5)
    P = 301
    rnd = lambda w: torch.randint(-2 ** 31, 2 ** 31 - 1, (P, w), dtype=torch.int64, device=dev, generator=g).to(torch.int32)
    srcs = [rnd(w) for w in (2, 9, 4096, 5000, 45, 1)] + [rnd(2) for _ in range(34)]
    assert len(srcs) == 40
    index = torch.randperm(P, generator=torch.Generator().manual_seed(6))[:200].to(dev)
    _check_gather(srcs, index, P)


# ---------------------------------------------------------------------------------------------------- 4 - 6. the model
W, H, NP = 64, 48, 3000


def _scene(kind):
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd.synthetic import lidar_scene, random_scene
    return (random_scene if kind == "random" else lidar_scene)(NP, W, H, sh_degree=3, seed=3)


def _trained(raw, order, steps=3, **kw):
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


def _limits(m):
    """Limits in the activated domain that remove a fair share of THIS map: the median opacity and the 90 % quantile of the largest extent."""
    op = torch.sigmoid(m.opacity.detach().double()).reshape(-1)
    sc = torch.exp(m.scaling.detach().double()).max(1).values
    return float(op.median().clamp(1e-6, 1 - 1e-6)), float(torch.quantile(sc, 0.9))


def _model_mask(m, min_opacity, max_scale, drop, protect):
    from gaussian_lic_amd.trainer import prune_thresholds
    lo, hi = prune_thresholds(min_opacity, max_scale)
    P = m.P
    t = dict(xyz=m._buf["xyz"][:P], dc=m._buf["features_dc"][:P].reshape(P, 3), opacity=m._buf["opacity"][:P].reshape(P), scaling=m._buf["scaling"][:P],
             rotation=m._buf["rotation"][:P])
    return _keep_mask(t, lo, hi, True, drop, protect)


@pytest.mark.parametrize("order", ["insertion", "morton"])
@pytest.mark.parametrize("kind", ["random", "lidar"])
def test_model_after_prune_equals_torch_indexing(kind, order):
    dev = gpu()
    m, _cam, _gt, _bg = _trained(_scene(kind), order)
    assert any(float(m._m[n][:m.P].abs().max()) > 0 for n in m.NAMES)          # (the moments are non-zero: the steps did something)
    g = torch.Generator().manual_seed(11)
    drop = (torch.rand(NP, generator=g) < 0.1).to(dev)
    protect = (torch.rand(NP, generator=g) < 0.05).to(dev)
    lim = _limits(m)
    before = map_snapshot(m, tie=True)
    mask = _model_mask(m, lim[0], lim[1], drop, protect)
    sorted_before, version, cap = m._sorted_P, m.layout_version, m.capacity
    n_removed, kept = m.prune(lim[0], lim[1], drop=drop, protect=protect)
    Pn = int(mask.sum())
    assert 0 < Pn < NP and n_removed == NP - Pn and m.P == Pn and m.capacity == cap and m.layout_version == version + 1
    assert kept.dtype == torch.int64 and torch.equal(kept, mask.nonzero().squeeze(1))
    assert m._sorted_P == int(mask[:sorted_before].sum())
    for i, n in enumerate(m.NAMES):
        assert torch.equal(bits(getattr(m, n).detach()), bits(before[n][mask])), n
        st = m.optimizer.state[i]
        assert torch.equal(bits(st["exp_avg"]), bits(before[n + ".m"][mask])) and torch.equal(bits(st["exp_avg_sq"]), bits(before[n + ".v"][mask])), n
        assert getattr(m, n).data_ptr() == m._buf[n].data_ptr() == m.optimizer.params[i].data_ptr()        # the optimizer sees the new tensors
    if order == "insertion":
        assert m.tie_rank is None and m.original_order() is None
    else:
        old = before["tie"][mask]
        assert torch.equal(torch.sort(m.tie_rank.long()).values, torch.arange(Pn, device=dev))
        assert torch.equal(m.original_order(), torch.argsort(old))
    # nothing to remove: the storage is left alone
    ptrs = [m._buf[n].data_ptr() for n in m.NAMES]
    n0, kept0 = m.prune()
    assert n0 == 0 and torch.equal(kept0, torch.arange(Pn, device=dev)) and ptrs == [m._buf[n].data_ptr() for n in m.NAMES]
    assert m.layout_version == version + 1


def test_prune_before_training_setup_and_to_nothing():
    from gaussian_lic_amd import trainer
    dev = gpu()
    raw = _scene("random")
    m = trainer.GaussianModel({k: (v.clone() if torch.is_tensor(v) else v) for k, v in raw.items()}, dev, order="morton")
    before = map_snapshot(m, tie=True)
    mask = _model_mask(m, 0.5, None, None, None)
    n, kept = m.prune(min_opacity=0.5)
    assert n == NP - int(mask.sum()) and torch.equal(kept, mask.nonzero().squeeze(1))
    for name in m.NAMES:
        assert torch.equal(bits(getattr(m, name).detach()), bits(before[name][mask])), name
    m.training_setup()
    n, kept = m.prune(drop=torch.ones(m.P, dtype=torch.bool, device=dev))      # every row: an empty map
    assert m.P == 0 and kept.numel() == 0 and m.xyz.shape == (0, 3) and m.tie_rank.numel() == 0 and m._sorted_P == 0


@pytest.mark.parametrize("kind", ["random", "lidar"])
def test_pruned_orders_export_and_render_alike(kind, tmp_path):
    """The same ORIGINAL rows pruned from an insertion-order and a Morton model: byte-identical save_map, bit-identical strict render."""
    from gaussian_lic_amd import io_ply
    from gaussian_lic_amd.rasterizer import render
    dev = gpu()
    raw = _scene(kind)
    a, cam, gt, bg = _trained(raw, "insertion")
    b, _c, _g, _b = _trained(raw, "morton")
    lim = _limits(a)
    g = torch.Generator().manual_seed(12)
    drop_orig = (torch.rand(NP, generator=g) < 0.1).to(dev)                    # by ORIGINAL index
    tie_b = b.tie_rank.long().clone()
    na, kept_a = a.prune(lim[0], lim[1], drop=drop_orig)
    nb, kept_b = b.prune(lim[0], lim[1], drop=drop_orig[tie_b])
    assert na == nb and 0 < na < NP
    assert torch.equal(torch.sort(tie_b[kept_b]).values, kept_a)               # the same original rows survive
    pa, pb = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    assert io_ply.save_map(a, pa) == io_ply.save_map(b, pb) == NP - na
    assert open(pa, "rb").read() == open(pb, "rb").read()
    with torch.no_grad():
        ia, Ta, _, va, ra = render(cam, a, bg)
        ib, Tb, _, vb, rb = render(cam, b, bg)
    order = b.original_order()
    assert torch.equal(bits(ia), bits(ib)) and torch.equal(bits(Ta), bits(Tb)) and torch.equal(ra, rb[order])


@pytest.mark.parametrize("order", ["insertion", "morton"])
def test_training_goes_on_bit_for_bit_and_extend_keeps_ties_dense(order):
    """Rows invisible in a view (radii == 0) produce no instances, the backward is deterministic and Adam is per row: dropping exactly those rows
    leaves every kept row's parameters and moments after one further step on that view bit-identical to the unpruned model's."""
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.rasterizer import render
    from gaussian_lic_amd.synthetic import lidar_scene
    dev = gpu()
    raw = _scene("random")
    full, cam, gt, bg = _trained(raw, order, capacity=2 * NP, resort_fraction=None)
    cut, _c, _g, _b = _trained(raw, order, capacity=2 * NP, resort_fraction=None)
    with torch.no_grad():
        radii = render(cam, cut, bg)[4]
    invisible = radii == 0
    assert 0 < int(invisible.sum()) < NP
    n, kept = cut.prune(drop=invisible, drop_nonfinite=False)
    assert n == int(invisible.sum()) and torch.equal(kept, (~invisible).nonzero().squeeze(1))
    ta, _ = trainer.training_step_fused(full, cam, gt, bg)
    tb, _ = trainer.training_step_fused(cut, cam, gt, bg)
    assert torch.equal(bits(ta), bits(tb))
    for name in full.NAMES:
        assert torch.equal(bits(cut._buf[name][:cut.P]), bits(full._buf[name][:NP][kept])), name
        assert torch.equal(bits(cut._m[name][:cut.P]), bits(full._m[name][:NP][kept])), name + ".m"
        assert torch.equal(bits(cut._v[name][:cut.P]), bits(full._v[name][:NP][kept])), name + ".v"
    # extend() behind a prune that emptied the right half of the image: the new rows' ties P0..P0+k-1 collide with nothing
    u_pix = cut.xyz.detach()[:, 0] * (0.675 * W) / cut.xyz.detach()[:, 2].abs().clamp_min(0.2) + 0.4857 * W
    cut.prune(drop=u_pix > 0.5 * W)
    P0 = cut.P
    frame = lidar_scene(500, W, H, sh_degree=3, seed=77)
    pts = frame["xyz"].to(dev)
    col = (frame["features_dc"].reshape(-1, 3) * 0.28209479177387814 + 0.5).to(dev)
    Rcw = torch.from_numpy(cam.world_view_transform[:3, :3].T.copy())
    tcw = torch.from_numpy(cam.world_view_transform[3, :3].copy())
    k = cut.extend(cam, pts, col, frame["xyz"][:, 2].contiguous().to(dev), Rcw, tcw, (float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy)))
    assert k > 0 and cut.P == P0 + k
    if order == "morton":
        assert torch.equal(torch.sort(cut.tie_rank.long()).values, torch.arange(P0 + k, device=dev))
        assert cut._sorted_P <= P0
    trainer.training_step_fused(cut, cam, gt, bg)
    assert all(bool(torch.isfinite(cut._buf[name][:cut.P]).all()) for name in cut.NAMES)


def test_graphed_step_refuses_a_stale_layout():
    from gaussian_lic_amd import trainer
    m, cam, gt, bg = _trained(_scene("random"), "morton", steps=1)
    gs = trainer.GraphedStep(m, cam, gt, bg, check_every=0)
    gs.step()
    assert gs.check() == 0
    n, _kept = m.prune(min_opacity=_limits(m)[0])
    assert n > 0
    with pytest.raises(RuntimeError, match="rows changed since this step was built"):
        gs.step()
    gs2 = trainer.GraphedStep(m, cam, gt, bg, check_every=0)
    terms = gs2.step()
    assert gs2.check() == 0 and bool(torch.isfinite(terms).all())


# ---------------------------------------------------------------------------------------------------- 7. the C++ host
def test_fused_prune_cpp_host(tmp_path):
    """gslic::FusedStep::prune issues the calls of GaussianModel.prune: after two steps, a prune with the same limits and two more steps on a map
    handed over in Morton order (tie_rank), kept indices, parameters and the position moments are bit-identical to the Python host's."""
    from gaussian_lic_amd import trainer
    exe = fio.build("fused_prune")
    iters, min_opacity, max_scale = 2, 0.3, 1.0
    m, cam, gt, bg = _trained(_scene("random"), "morton", steps=0)
    d = str(tmp_path)
    fio.write_inputs(d, m, cam, gt=gt, tie_rank=m.tie_rank)
    r = fio.run(exe, d, str(NP), str(W), str(H), "3", str(iters), repr(min_opacity), repr(max_scale))
    for _ in range(iters):
        trainer.training_step_fused(m, cam, gt, bg)
    n_removed, kept = m.prune(min_opacity, max_scale)
    assert 0 < n_removed < NP and f"prune removed {n_removed} size {m.P}" in r.stdout
    for _ in range(iters):
        trainer.training_step_fused(m, cam, gt, bg)
    rd = lambda name, shape: fio.read(d, name + ".f32", np.float32).numpy().reshape(shape)
    np.testing.assert_array_equal(rd("kept", (m.P,)).astype(np.int64), kept.cpu().numpy())
    for name, t in (("xyz", m.xyz), ("scaling", m.scaling), ("rotation", m.rotation), ("opacity", m.opacity), ("dc", m.features_dc), ("rest", m.features_rest),
                    ("m_xyz", m._m["xyz"][:m.P]), ("v_xyz", m._v["xyz"][:m.P])):
        np.testing.assert_array_equal(rd(name, tuple(t.shape)), t.detach().cpu().numpy(), err_msg=name)
