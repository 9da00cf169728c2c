"""-m gpu: keeping the map in Morton order from the library — gslic_morton_order (the exact key rule and the stable sort), gslic_permute_rows (every
row array re-ordered in place), trainer.GaussianModel.resort / to_morton_order on top of them and the C++ host's gslic::FusedStep::resort.

The yardstick of the keys and of the permutation is tests/resort_ref.py: the header's rule in numpy float32 and a stable np.argsort.  The
yardstick of the row move is torch indexing on the same tensors.  Every comparison is exact (integers, or int32 views of the rows)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import fused_check_io as fio
import resort_ref as ref
from gpu_helpers import bits, gpu, guarded, guards_intact, same_map

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257, 4097, 70001]     # a partial wave, one wave and one over, more than one sort tile of 4096, many workgroups


def _libs():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    return _lib, _lib.lib()


def _order(xyz, box):
    """gslic_morton_order with guard words around both outputs -> (perm, keys_sorted) as uint32 numpy arrays."""
    _l, L = _libs()
    P, dev = int(xyz.shape[0]), xyz.device
    pbuf, perm = guarded(P, device=dev)
    kbuf, keys = guarded(P, device=dev)
    scratch = _l.TensorAllocator(dev)
    _l.check(L.gslic_morton_order(P, _l.ptr(xyz), _l.ptr(box), scratch.cb, None, ctypes.c_void_p(perm.data_ptr()), ctypes.c_void_p(keys.data_ptr()),
                                  _l.current_stream_ptr()))
    torch.cuda.synchronize()
    assert guards_intact(pbuf, P) and guards_intact(kbuf, P)
    return perm.cpu().numpy().view(np.uint32), keys.cpu().numpy().view(np.uint32)


def _cloud(kind, P):
    """(xyz float32 [P,3] CPU, [boxes]).  lattice: positions on a 7 x 7 x 7 lattice, so that most keys tie and the sort's stability decides the
    permutation.  wild: a random cloud with 1 % of the rows outside the box, one row each of NaN, +inf and -inf (as P allows), under a regular box
    and under one with a zero-extent axis."""
    g = torch.Generator().manual_seed(31 * P + len(kind))
    if kind == "lattice":
        xyz = torch.randint(0, 7, (P, 3), generator=g).float() * torch.tensor([0.5, 1.0 / 3.0, 0.7]) + torch.tensor([-1.5, -1.0, 0.1])
        return xyz.contiguous(), [torch.tensor([-1.5, -1.0, 0.1, 1.5, 1.0, 4.3])]
    lo, hi = torch.tensor([-2.0, 0.25, -7.0]), torch.tensor([3.0, 1.75, 11.0])
    xyz = lo + (hi - lo) * torch.rand(P, 3, generator=g)
    out = torch.rand(P, generator=g) < 0.01
    if P > 8:
        out[8] = True
    xyz[out] = (xyz[out] - (lo + hi) / 2) * 3.0 + (lo + hi) / 2        # three times as far from the centre: most of them leave the box
    for row, v in enumerate((float("nan"), float("inf"), float("-inf"))):
        if P > 4 * row + 1:
            xyz[4 * row + 1, row] = v
    flat = torch.cat([lo, hi]).clone()
    flat[4] = flat[1]                                                  # hi_y == lo_y: a zero-extent axis
    return xyz.contiguous(), [torch.cat([lo, hi]), flat]


@pytest.mark.parametrize("kind", ["lattice", "wild"])
@pytest.mark.parametrize("P", SIZES)
def test_keys_and_permutation_match_the_rule_on_bits(P, kind):
    dev = gpu()
    xyz_c, boxes = _cloud(kind, P)
    xyz = xyz_c.to(dev)
    for box_c in boxes:
        box = box_c.to(dev)
        want_perm, want_keys = ref.morton_perm(xyz_c.numpy(), box_c.numpy())
        perm, keys = _order(xyz, box)
        assert np.array_equal(keys, want_keys)                         # the key rule, bit for bit
        assert np.array_equal(perm, want_perm)                         # ... and the stable order
        if kind == "lattice" and P >= 4097:
            assert np.unique(want_keys).size <= 343 < P                # (the keys do tie: stability decided)
        perm2, keys2 = _order(xyz, box)                                # a repeat is bit-identical
        assert np.array_equal(perm2, perm) and np.array_equal(keys2, keys)
        moved = xyz[torch.from_numpy(perm.astype(np.int64)).to(dev)].contiguous()
        perm3, keys3 = _order(moved, box)                              # already in order: the identity
        assert np.array_equal(perm3, np.arange(P, dtype=np.uint32)) and np.array_equal(keys3, keys)
    # keys_sorted is optional
    _l, L = _libs()
    pbuf, only = guarded(P, device=dev)
    scratch = _l.TensorAllocator(dev)
    _l.check(L.gslic_morton_order(P, _l.ptr(xyz), _l.ptr(box), scratch.cb, None, ctypes.c_void_p(only.data_ptr()), None, _l.current_stream_ptr()))
    torch.cuda.synchronize()
    assert guards_intact(pbuf, P) and np.array_equal(only.cpu().numpy().view(np.uint32), perm)


@pytest.mark.parametrize("copy", ["memcpy", "kernel"])     # the way back: one copy per array (the default), or the one launch of the A/B switch
@pytest.mark.parametrize("which", ["identity", "reversal", "random"])
def test_permute_rows_matches_torch_indexing_in_place(which, copy, monkeypatch):
    monkeypatch.setenv("GSLIC_PERMUTE_COPY", copy)
    _l, L = _libs()
    dev = gpu()
    cap, n = 8300, 8200                       # width 1: three workgroups of 4096 rows; width 45: 91 rows per workgroup; rows behind n stay
    widths = [1, 2, 3, 4, 45]
    g = torch.Generator().manual_seed(5)
    arrays = [torch.randint(-2 ** 31, 2 ** 31 - 1, (cap, w), generator=g, dtype=torch.int64).to(torch.int32).to(dev) for w in widths]
    before = [a.clone() for a in arrays]
    ptrs = [a.data_ptr() for a in arrays]
    perm = {"identity": torch.arange(n), "reversal": torch.arange(n - 1, -1, -1), "random": torch.randperm(n, generator=g)}[which].to(dev)
    perm32 = perm.to(torch.int32)
    arr = (_l.RowArray * len(widths))(*[_l.RowArray(a.data_ptr(), a.data_ptr(), w) for a, w in zip(arrays, widths)])
    need = 4 * n * sum(widths)
    assert L.gslic_permute_rows_staging_bytes(arr, len(widths), n) == L.gslic_scratch_round_up(need)
    sbuf, staging = guarded(need // 4, device=dev)                    # exactly the sum: the rounding is advice for an allocator
    _l.check(L.gslic_permute_rows(arr, len(widths), _l.ptr(perm32), n, ctypes.c_void_p(staging.data_ptr()), need, _l.current_stream_ptr()))
    torch.cuda.synchronize()
    assert guards_intact(sbuf, need // 4)
    for a, b, p, w in zip(arrays, before, ptrs, widths):
        assert a.data_ptr() == p
        assert torch.equal(a[:n], b[:n][perm]), w
        assert torch.equal(a[n:], b[n:]), w                            # rows from n_rows on are untouched
    # fewer rows than one workgroup's share, an array of width 0 in the list, a staging buffer larger than needed
    small = [torch.arange(10 * w, dtype=torch.int32, device=dev).reshape(10, w) for w in (3, 45)]
    keep = [s.clone() for s in small]
    p7 = torch.tensor([6, 0, 5, 1, 4, 2, 3], dtype=torch.int32, device=dev)
    arr = (_l.RowArray * 3)(_l.RowArray(small[0].data_ptr(), small[0].data_ptr(), 3), _l.RowArray(None, None, 0),
                            _l.RowArray(small[1].data_ptr(), small[1].data_ptr(), 45))
    st = torch.empty(4096, dtype=torch.uint8, device=dev)
    _l.check(L.gslic_permute_rows(arr, 3, _l.ptr(p7), 7, _l.ptr(st), 4096, _l.current_stream_ptr()))
    torch.cuda.synchronize()
    for s, k in zip(small, keep):
        assert torch.equal(s[:7], k[:7][p7.long()]) and torch.equal(s[7:], k[7:])


# ---------------------------------------------------------------------------------------------------- the model
W, H, NP = 320, 192, 30000


def _scene(seed=5, quantum=0.5):
    """The small scene of tests/test_morton_order_gpu.py (depths quantised so that thousands of Gaussians tie), without the right 30 % of the
    image: that is where extend() inserts LiDAR points."""
    from gaussian_lic_amd.synthetic import random_scene
    raw = random_scene(NP, W, H, sh_degree=3, seed=seed)
    z = raw["xyz"][:, 2]
    zq = torch.where(z > 0.3, (z / quantum).round().clamp_min(1.0) * quantum, z)
    raw["xyz"] = torch.stack([raw["xyz"][:, 0] * zq / z, raw["xyz"][:, 1] * zq / z, zq], 1).contiguous()
    u_pix = raw["xyz"][:, 0] * (0.675 * W) / raw["xyz"][:, 2].abs().clamp_min(0.2) + 0.4857 * W
    keep = u_pix < 0.7 * W
    return {k: (v[keep].contiguous() if torch.is_tensor(v) else v) for k, v in raw.items()}


def _frame(cam, dev, n=4000, seed=77):
    from gaussian_lic_amd.synthetic import lidar_scene
    frame = lidar_scene(n, W, H, sh_degree=3, seed=seed)
    pts = frame["xyz"].to(dev)
    col = (frame["features_dc"].reshape(-1, 3) * 0.28209479177387814 + 0.5).to(dev)
    rsp = frame["xyz"][:, 2].contiguous().to(dev)
    Rcw = torch.from_numpy(cam.world_view_transform[:3, :3].T.copy())
    tcw = torch.from_numpy(cam.world_view_transform[3, :3].copy())
    return pts, col, rsp, Rcw, tcw, (float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy))


def _grown(raw, order, cam, gt, bg, dev, steps=2):
    """A model of the scene, trained `steps` steps, extended by one LiDAR frame (no automatic re-sort) and trained again: a Morton model then has
    an unsorted tail and moved positions, and every moment is non-zero."""
    from gaussian_lic_amd import trainer
    m = trainer.GaussianModel({k: (v.clone() if torch.is_tensor(v) else v) for k, v in raw.items()}, dev, order=order, capacity=2 * raw["xyz"].shape[0],
                              resort_fraction=None)
    m.training_setup()
    for _ in range(steps):
        trainer.training_step_fused(m, cam, gt, bg)
    assert m.extend(cam, *_frame(cam, dev)) > 0
    for _ in range(steps):
        trainer.training_step_fused(m, cam, gt, bg)
    return m


def _storage(m):
    return [(n, bits(t[:m.P]).clone()) for _d, n, t, _w, _z in m._row_arrays()]


def test_model_resort_is_the_reference_permutation_in_place_and_the_map_is_unchanged(monkeypatch):
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.rasterizer import render
    from gaussian_lic_amd.synthetic import gt_image
    dev = gpu()
    cam = synthetic_camera(W, H).to_device(dev)
    gt, bg = gt_image(H, W).to(dev), torch.zeros(3, device=dev)
    raw = _scene()
    monkeypatch.delenv("GSLIC_RESORT", raising=False)
    a, b, c = (_grown(raw, o, cam, gt, bg, dev) for o in ("insertion", "morton", "morton"))
    same_map(a, b)
    assert all(torch.equal(x, y) for (_n, x), (_n2, y) in zip(_storage(b), _storage(c)))     # (c is b again: it takes the torch route below)
    st = trainer.ContributionStats(b)
    with torch.no_grad():
        err = (render(cam, b, bg)[0] - gt).abs().mean(0).contiguous()
    st.accumulate(cam, error=err)
    stats_before = [x[:b.P].clone() for x, _w in st._arrays()]
    assert len(stats_before) == 4 and all(bool(x.any()) for x in stats_before)
    # the yardstick: the header's rule on the pre-call positions and box
    xyz0 = b._buf["xyz"][:b.P].clone()
    box0 = trainer.morton_box(xyz0)
    want, _keys = ref.morton_perm(xyz0.cpu().numpy(), box0.cpu().numpy())
    addresses = [t.data_ptr() for _d, _n, t, _w, _z in b._row_arrays()] + [x.data_ptr() for x, _w in st._arrays()]
    lv, rv, sorts = b.layout_version, b._rows_version, len(b.sort_ms)
    old = _storage(b)
    perm = b.resort()
    assert perm.dtype == torch.int64 and perm.device.type == "cuda" and np.array_equal(perm.cpu().numpy(), want.astype(np.int64))
    assert not torch.equal(perm.cpu(), torch.arange(b.P))
    assert [t.data_ptr() for _d, _n, t, _w, _z in b._row_arrays()] + [x.data_ptr() for x, _w in st._arrays()] == addresses
    assert b.layout_version == lv and b._rows_version == rv + 1 and b._sorted_P == b.P and len(b.sort_ms) == sorts + 1
    for (n, x), (_n, y) in zip(_storage(b), old):
        assert torch.equal(x, y[perm]), n                               # every array moved by the permutation returned
    for x, y in zip(stats_before, [x[:b.P] for x, _w in st._arrays()]):
        assert torch.equal(y, x[perm])                                  # the attached statistics follow the rows
    st.accumulate(cam)                                                  # ... and stay usable
    # the torch route (GSLIC_RESORT=torch) on the identical model: the same permutation and the same 19 arrays, bit for bit
    monkeypatch.setenv("GSLIC_RESORT", "torch")
    perm_t = c.resort()
    monkeypatch.delenv("GSLIC_RESORT")
    assert torch.equal(perm_t, perm)
    for (n, x), (_n, y) in zip(_storage(b), _storage(c)):
        assert torch.equal(x, y), n
    # still the insertion-order twin's map: the image, and fused steps after the re-sort
    same_map(a, b)
    with torch.no_grad():
        ia, ib = render(cam, a, bg)[0], render(cam, b, bg)[0]
    assert torch.equal(ia, ib)
    for _ in range(2):
        la, _x = trainer.training_step_fused(a, cam, gt, bg)
        lb, _y = trainer.training_step_fused(b, cam, gt, bg)
    assert torch.equal(torch.as_tensor(la), torch.as_tensor(lb))
    same_map(a, b)
    # to_morton_order(): the insertion-order twin becomes a Morton model with b's storage (b re-sorted on the same positions first)
    b.resort()
    with pytest.raises(AssertionError, match="insertion order"):
        a.resort()
    pa = a.to_morton_order()
    assert a.order == "morton" and a.resort_fraction == 0.1 and a._sorted_P == a.P and sorted(pa.cpu().tolist()) == list(range(a.P))
    # The same storage — up to what the rule leaves open: rows of EQUAL key stay in their storage order before the call, which is the original order
    # in `a` and the order of an earlier sort (other positions, another box) in `b`; this scene has such rows (its depths are quantised).  So: the
    # same key at every row, and the same rows once every run of equal keys is listed by original index — for `a` that listing is the identity.
    def canonical(m):
        xyz = m._buf["xyz"][:m.P]
        keys = ref.morton_keys(xyz.cpu().numpy(), trainer.morton_box(xyz).cpu().numpy()).astype(np.int64)
        assert np.all(np.diff(keys) >= 0)                               # (sorted by key)
        return keys, torch.from_numpy(np.lexsort((m.tie_rank.cpu().numpy(), keys))).to(dev)
    (ka, ca), (kb, cb) = canonical(a), canonical(b)
    assert np.array_equal(ka, kb) and torch.equal(ca.cpu(), torch.arange(a.P))
    moved = int((cb.cpu() != torch.arange(b.P)).sum())
    print(f"to_morton_order: {moved} of {b.P} rows of the twin sit elsewhere inside a run of equal keys ({b.P - np.unique(kb).size} rows share a key)")
    for (n, x), (_n, y) in zip(_storage(a), _storage(b)):
        assert torch.equal(x, y[cb]), n
    for _ in range(2):
        trainer.training_step_fused(a, cam, gt, bg); trainer.training_step_fused(b, cam, gt, bg)
    for (n, x), (_n, y) in zip(_storage(a), _storage(b)):
        assert torch.equal(x, y[cb]), n


# ---------------------------------------------------------------------------------------------------- the C++ host
def test_fused_resort_cpp_host(tmp_path, monkeypatch):
    """gslic::FusedStep::resort / set_resort_fraction issue the calls of the Python host: a first sort from insertion order, an extend() whose tail
    passes the fraction (the rule re-sorts), a prune() followed by resort(), training steps before and after each — all 19 arrays, the three
    permutations and err_sum are bit-identical to the Python model's."""
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.rasterizer import render
    from gaussian_lic_amd.synthetic import gt_image
    exe = fio.build("fused_resort")
    monkeypatch.delenv("GSLIC_RESORT", raising=False)
    dev = gpu()
    cam = synthetic_camera(W, H).to_device(dev)
    gt, bg = gt_image(H, W).to(dev), torch.zeros(3, device=dev)
    raw = _scene(seed=9)
    P0 = int(raw["xyz"].shape[0])
    iters, fraction, w_min, n_pts = 2, 0.05, trainer.ContributionStats.W_MIN, 4000
    m = trainer.GaussianModel({k: (v.clone() if torch.is_tensor(v) else v) for k, v in raw.items()}, dev)
    m.training_setup()
    d = str(tmp_path)
    pts, col, rsp, Rcw, tcw, intr = _frame(cam, dev, n=n_pts)
    fio.write_inputs(d, m, cam, scalars_extra=intr, gt=gt, pts=pts, col=col, rsp=rsp, Rcw=Rcw, tcw=tcw)

    def steps():
        for _ in range(iters):
            trainer.training_step_fused(m, cam, gt, bg)
    steps()
    with torch.no_grad():
        err = (render(cam, m, bg)[0] - gt).abs().mean(0).contiguous()
    fio.write(d, "err", err)
    st = trainer.ContributionStats(m)
    st.accumulate(cam, w_min=w_min, error=err)
    perm0 = m.to_morton_order(resort_fraction=fraction)                 # the first sort, from insertion order
    steps()
    seen, resort = [], m.resort
    m.resort = lambda: seen.append(resort()) or seen[-1]                # (extend() does not return the permutation of the re-sort it triggers)
    k = m.extend(cam, pts, col, rsp, Rcw, tcw, intr)
    del m.resort
    assert k > fraction * (P0 + k) and len(seen) == 1 and m._sorted_P == m.P == P0 + k                    # the rule re-sorted
    steps()
    # limits (activated domain) that remove a fair share of THIS map: the median opacity and the 90 % quantile of the largest extent
    min_opacity = float(torch.sigmoid(m.opacity.detach().double()).median().clamp(1e-6, 1 - 1e-6))
    max_scale = float(torch.quantile(torch.exp(m.scaling.detach().double()).max(1).values, 0.9))
    removed, _kept = m.prune(min_opacity=min_opacity, max_scale=max_scale)
    assert removed > 0 and m._sorted_P == m.P > 1000                    # (a compaction keeps the sorted block sorted)
    perm2 = m.resort()
    steps()
    r = fio.run(exe, d, str(P0), str(W), str(H), "3", str(iters), str(n_pts), repr(fraction), repr(min_opacity), repr(max_scale), repr(w_min))
    assert f"resort extended {k} resorts 2 pruned {removed} size {m.P}" in r.stdout
    rd = functools.partial(fio.read, d)
    P = m.P
    for n, f in (("xyz", "xyz"), ("features_dc", "dc"), ("features_rest", "rest"), ("opacity", "opacity"), ("scaling", "scaling"), ("rotation", "rotation")):
        for pre, src in (("", m._buf), ("m_", m._m), ("v_", m._v)):
            assert torch.equal(rd(pre + f + ".f32", np.int32), bits(src[n][:P]).cpu().reshape(-1)), pre + f
    assert torch.equal(rd("tie.i32", np.int32), m.tie_rank.cpu())
    assert torch.equal(rd("err_sum.i64", np.int64), st.error_fixed().cpu())
    assert torch.equal(rd("perm0.i64", np.int64), perm0.cpu()) and torch.equal(rd("perm2.i64", np.int64), perm2.cpu())
    assert torch.equal(rd("perm1.i64", np.int64), seen[0].cpu()) and seen[0].numel() == P0 + k
