"""-m gpu: the LiDAR depth image in the library (gslic_lidar_zbuffer_add / gslic_lidar_zbuffer_resolve, trainer.LidarDepth, gslic::LidarDepth).

Every comparison is on bits; the rule has no tolerance.  References, none of them the code under test: Camera.project_depth and
trainer.free_space_bound (merged torch code) at footprint 0, the numpy transcription of tests/lidar_depth_ref.py (held against project_depth by
test_lidar_depth_cpu.py) for the index image and the footprints, and torch's max_pool2d as an independent route for the windowed minimum."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import fused_check_io as fio
import lidar_depth_ref as lr
from gpu_helpers import SENTINEL as SENTINEL32, bits, gpu

pytestmark = pytest.mark.gpu

SENTINEL64 = 0x5A5A5A5A5A5A5A5A


def _same_bits(a, b):
    return torch.equal(bits(a).cpu(), bits(torch.as_tensor(b)).cpu())


def _trainer():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    return trainer


def _image(W, H, view, pts, footprint=0, margins=None, index=True, count=True):
    """(LidarDepth, resolve dict) of one sweep of `pts` (numpy [n,3]) seen from synthetic_camera(W, H, view)."""
    trainer = _trainer()
    ld = trainer.LidarDepth(W, H, gpu())
    base = ld.add(lr.camera(W, H, view), torch.from_numpy(np.array(pts)).to(gpu()))
    assert base == 0 and ld.n_points == len(pts)
    return ld, ld.resolve(footprint=footprint, margins=margins, index=index, count=count)


# ------------------------------------------------------------------------------------------- 1. footprint 0 against the existing functions
@pytest.mark.parametrize("W,H", lr.SIZES)
def test_footprint_0_equals_project_depth_and_free_space_bound(W, H):
    trainer = _trainer()
    measured = nonpositive = 0
    for view in lr.VIEWS:
        cam = lr.camera(W, H, view)
        for n in lr.COUNTS:
            pts, _notes = lr.cloud(W, H, n, view)
            want = cam.project_depth(torch.from_numpy(pts.copy()).to(gpu()))
            ref = lr.images_of(W, H, n, view)
            for ma, mr in lr.MARGINS:
                _ld, out = _image(W, H, view, pts, margins=(ma, mr))
                depth = out["depth"]
                assert depth.shape == (H, W) and depth.dtype == torch.float32 and _same_bits(depth, want), (view, n)
                assert _same_bits(out["near"], trainer.free_space_bound(want, ma, mr)), (view, n, ma, mr)
                assert out["index"].dtype == torch.int32 and torch.equal(out["index"].cpu(), torch.from_numpy(ref["index"])), (view, n)
                assert torch.equal(out["index"] == -1, depth == 0)
                assert int(out["n_measured"]) == int((depth > 0).sum()) == ref["n_measured"]
                if ma == 100.0:
                    nonpositive += int(((out["near"] <= 0) & (depth > 0)).sum())
                    assert not bool((out["near"] > 0).any())
            measured += ref["n_measured"]
            assert _same_bits(trainer.lidar_depth_image(cam, torch.from_numpy(pts.copy()).to(gpu())), want)
    assert measured > 0 and nonpositive > 0


# ------------------------------------------------------------------------------------------- 2. footprints
@pytest.mark.parametrize("r", lr.FOOTPRINTS)
@pytest.mark.parametrize("W,H", lr.SIZES)
def test_footprints_equal_the_windowed_minimum_of_the_keys(W, H, r):
    margins = lr.MARGINS[1]
    grew = 0
    for view in lr.VIEWS:
        for n in lr.COUNTS:
            pts, _notes = lr.cloud(W, H, n, view)
            ref, ref0 = lr.images_of(W, H, n, view, r, margins), lr.images_of(W, H, n, view)
            _ld, out = _image(W, H, view, pts, footprint=r, margins=margins)
            assert _same_bits(out["depth"], torch.from_numpy(ref["depth"])), (view, n)
            assert torch.equal(out["index"].cpu(), torch.from_numpy(ref["index"])), (view, n)
            assert _same_bits(out["near"], torch.from_numpy(ref["near"])), (view, n)
            assert int(out["n_measured"]) == ref["n_measured"], (view, n)
            # the independent torch route: min-pool of the footprint-0 depth with +inf for empty
            d0 = torch.from_numpy(ref0["depth"]).to(gpu())
            d_inf = torch.where(d0 > 0, d0, torch.full_like(d0, float("inf")))
            pooled = -torch.nn.functional.max_pool2d(-d_inf[None, None], 2 * r + 1, 1, r)[0, 0]
            assert _same_bits(out["depth"], torch.where(torch.isinf(pooled), torch.zeros_like(pooled), pooled)), (view, n)
            grew += ref["n_measured"] - ref0["n_measured"]
    assert grew > 0


# ------------------------------------------------------------------------------------------- 3. sweeps
def test_sweeps_accumulate_and_clear_empties():
    trainer = _trainer()
    W, H, view = 37, 23, "se3_c"
    cam = lr.camera(W, H, view)
    a, b = lr.cloud(W, H, 257, view)[0], lr.cloud(W, H, 65, view, seed=1, plant=False)[0]   # (no planted rows in b: they would tie with a's)
    ta, tb = torch.from_numpy(a.copy()).to(gpu()), torch.from_numpy(b.copy()).to(gpu())
    _ld, whole = _image(W, H, view, np.concatenate([a, b]))
    ld = trainer.LidarDepth(W, H, gpu())
    assert ld.add(cam, ta) == 0 and ld.add(cam, tb) == 257 and ld.n_points == 322
    ab = ld.resolve(index=True, count=True)
    assert _same_bits(ab["depth"], whole["depth"]) and torch.equal(ab["index"], whole["index"]) and int(ab["n_measured"]) == int(whole["n_measured"])
    assert bool((ab["index"] >= 257).any()) and bool(((ab["index"] >= 0) & (ab["index"] < 257)).any())    # both sweeps won pixels
    ld.clear()
    assert ld.add(cam, tb) == 0 and ld.add(cam, ta) == 65
    ba = ld.resolve(index=True)
    assert _same_bits(ba["depth"], whole["depth"])
    rebased = torch.where(ba["index"] < 0, ba["index"], torch.where(ba["index"] >= 65, ba["index"] - 65, ba["index"] + 257))
    assert torch.equal(rebased, whole["index"])
    ld.clear()
    none = ld.resolve(index=True, count=True)
    assert not bool(none["depth"].any()) and bool((none["index"] == -1).all()) and int(none["n_measured"]) == 0
    assert ld.add(cam, ta[:0]) == 0
    none = ld.resolve(footprint=3, margins=(0.1, 0.02), index=True, count=True)
    assert not bool(none["depth"].any()) and not bool(none["near"].any()) and bool((none["index"] == -1).all()) and int(none["n_measured"]) == 0
    ld.add(cam, ta)
    one = ld.resolve(index=True)
    only_a = _image(W, H, view, a)[1]
    assert _same_bits(one["depth"], only_a["depth"]) and torch.equal(one["index"], only_a["index"])       # nothing of the earlier sweeps is left


# ------------------------------------------------------------------------------------------- 4. determinism and bounds
def test_repeats_shuffles_guard_words_on_a_side_stream():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    L = _lib.lib()
    dev = gpu()
    W, H, n, view, r, margins = 37, 23, 4097, "se3_d", 3, lr.MARGINS[1]
    cam = lr.camera(W, H, view)
    pts, notes = lr.cloud(W, H, n, view)
    R, t = lr.pose_f32(cam)
    d_R, d_t = torch.from_numpy(R.copy()).to(dev), torch.from_numpy(t.copy()).to(dev)
    N = W * H
    side = torch.cuda.Stream()

    def run(points, footprint):
        """One add + one resolve through the C ABI on guarded buffers, on the side stream.  Returns (depth, index, near, count) on the CPU."""
        d_p = torch.from_numpy(np.array(points)).to(dev)
        z = torch.full((N + 64,), SENTINEL64, dtype=torch.int64, device=dev)
        f = [torch.full((N + 64,), SENTINEL32, dtype=torch.int32, device=dev) for _ in range(3)]
        c = torch.full((65,), SENTINEL32, dtype=torch.int32, device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            sp = ctypes.c_void_p(side.cuda_stream)
            at = lambda x, o: ctypes.c_void_p(x.data_ptr() + o * x.element_size())
            _lib.check(L.gslic_lidar_zbuffer_add(len(points), _lib.ptr(d_p), _lib.ptr(d_R), _lib.ptr(d_t), float(cam.fx), float(cam.fy), float(cam.cx),
                                                 float(cam.cy), W, H, at(z, 32), 1, 0, sp))
            _lib.check(L.gslic_lidar_zbuffer_resolve(W, H, at(z, 32), footprint, margins[0], margins[1], at(f[0], 32), at(f[1], 32), at(f[2], 32),
                                                     at(c, 32), sp))
        side.synchronize()
        for g, s in ((z, SENTINEL64), (f[0], SENTINEL32), (f[1], SENTINEL32), (f[2], SENTINEL32)):
            assert bool((g[:32] == s).all()) and bool((g[32 + N:] == s).all())
        assert bool((c[:32] == SENTINEL32).all()) and bool((c[33:] == SENTINEL32).all())
        img = lambda x: x[32:32 + N].reshape(H, W).cpu().clone()
        return img(f[0]), img(f[1]), img(f[2]), int(c[32])

    for footprint in (0, r):
        ref = lr.images_of(W, H, n, view, footprint, margins)
        first = run(pts, footprint)
        assert torch.equal(first[0], torch.from_numpy(ref["depth"]).view(torch.int32)) and torch.equal(first[1], torch.from_numpy(ref["index"]))
        assert torch.equal(first[2], torch.from_numpy(ref["near"]).view(torch.int32)) and first[3] == ref["n_measured"]
        for _ in range(4):                                                                                   # five runs in all
            again = run(pts, footprint)
            assert all(torch.equal(x, y) for x, y in zip(first[:3], again[:3])) and first[3] == again[3]
    # a shuffled order: the same depth, the same points after mapping back — but for the bit-equal pair, where the lower NEW index wins
    first = run(pts, 0)
    perm = np.random.default_rng(5).permutation(n)
    shuffled = run(pts[perm], 0)
    assert torch.equal(shuffled[0], first[0]) and shuffled[3] == first[3]
    back = torch.from_numpy(perm)[shuffled[1].long().clamp_min(0)]
    back = torch.where(shuffled[1] < 0, shuffled[1].long(), back)
    i_lo, i_hi = notes["equal_z"]
    assert i_lo < i_hi and np.array_equal(pts[i_lo].view(np.int32), pts[i_hi].view(np.int32))
    pix = first[1] == i_lo
    assert int(pix.sum()) == 1 and not bool((first[1] == i_hi).any())                                       # the lower index won
    assert torch.equal(back[~pix], first[1].long()[~pix])
    new_lo = min(int(np.nonzero(perm == i_lo)[0][0]), int(np.nonzero(perm == i_hi)[0][0]))
    assert int(shuffled[1][pix]) == new_lo and int(back[pix]) in (i_lo, i_hi)


# ------------------------------------------------------------------------------------------- 5. consumers
NP, SW, SH, NPTS = 400, 64, 64, 600
LAMBDA_DEPTH, MARGINS = 0.1, (0.1, 0.02)


def _scene():
    """A 64 x 64 scene of a few hundred Gaussians (as test_freespace_gpu.py builds), its camera and target, and a LiDAR sweep over it."""
    trainer = _trainer()
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import gt_image, lidar_scene, random_scene
    dev = gpu()
    m = trainer.GaussianModel(random_scene(NP, SW, SH, sh_degree=3, seed=3), dev)
    m.training_setup()
    cam = synthetic_camera(SW, SH).to_device(dev)
    points = lidar_scene(NPTS, SW, SH, sh_degree=0, seed=21)["xyz"].contiguous()
    return m, cam, gt_image(SH, SW).to(dev), torch.zeros(3, device=dev), points


def _rows(m):
    return {pre + n: bits(src[n][:m.P]).cpu().reshape(-1).clone() for n in m.NAMES for pre, src in (("", m._buf), ("m_", m._m), ("v_", m._v))}


def _five(st):
    return [st._max[:st.model.P].cpu().clone(), st._npix[:st.model.P].cpu().clone(), st.sum_fixed().cpu().clone(), st.free_fixed().cpu().clone(),
            st.measured_fixed().cpu().clone()]


def _consume(depth, near):
    """One depth-supervised fused step on `depth`, then one free-space accumulation with `near`: (rows, five accumulators, model)."""
    trainer = _trainer()
    m, cam, gt, bg, _points = _scene()
    trainer.training_step_fused(m, cam, gt, bg, gt_depth=depth, lambda_depth=LAMBDA_DEPTH)
    st = trainer.ContributionStats(m)
    st.accumulate(cam, free_space=near)
    torch.cuda.synchronize()
    out = _rows(m), _five(st)
    st.detach()
    return out


def test_library_images_feed_the_step_and_the_statistics_like_the_torch_ones():
    trainer = _trainer()
    _m, cam, _gt, _bg, points = _scene()
    d_pts = points.to(gpu())
    ld = trainer.LidarDepth(SW, SH, gpu())
    ld.add(cam, d_pts)
    lib = ld.resolve(margins=MARGINS)
    torch_depth = cam.project_depth(d_pts)
    torch_near = trainer.free_space_bound(torch_depth, *MARGINS)
    assert 0.05 < float((torch_depth > 0).float().mean()) < 0.5                                            # sparse returns, as a sweep gives
    rows_lib, five_lib = _consume(lib["depth"], lib["near"])
    rows_torch, five_torch = _consume(torch_depth, torch_near)
    for k in rows_torch:
        assert torch.equal(rows_lib[k], rows_torch[k]), k
    assert all(torch.equal(x, y) for x, y in zip(five_lib, five_torch))
    assert bool(five_torch[3].any()) and bool(five_torch[4].any())
    rows_plain, _ = _consume(None, torch_near)
    assert not torch.equal(rows_plain["xyz"], rows_torch["xyz"])                                            # the depth term really took part


# ------------------------------------------------------------------------------------------- 6. the C++ host
def test_fused_lidar_depth_cpp_host(tmp_path):
    """gslic::LidarDepth feeding FusedStep::step and accumulate_free_space gives the Python host's four images, its 18 parameter and moment arrays
    and its five accumulators, bit for bit."""
    trainer = _trainer()
    exe = fio.build("fused_lidar_depth")
    footprint, w_min = 0, trainer.ContributionStats.W_MIN   # test 5's setting
    m, cam, gt, bg, points = _scene()
    R, t = lr.pose_f32(cam)
    d = str(tmp_path)
    fio.write_inputs(d, m, cam, gt=gt, points=points,
                     lidar=np.concatenate([R, t, np.array([cam.fx, cam.fy, cam.cx, cam.cy, MARGINS[0], MARGINS[1], LAMBDA_DEPTH, w_min], np.float32)]))

    ld = trainer.LidarDepth(SW, SH, gpu())
    ld.add(cam, points.to(gpu()))
    im = ld.resolve(footprint=footprint, margins=MARGINS, index=True, count=True)
    trainer.training_step_fused(m, cam, gt, bg, gt_depth=im["depth"], lambda_depth=LAMBDA_DEPTH)
    st = trainer.ContributionStats(m)
    st.accumulate(cam, w_min=w_min, free_space=im["near"])
    r = fio.run(exe, d, str(NP), str(SW), str(SH), "3", str(NPTS), str(footprint))
    assert f"lidar measured {int(im['n_measured'])} base 0" in r.stdout
    rd = functools.partial(fio.read, d)
    assert torch.equal(rd("lidar_depth.f32", np.int32), bits(im["depth"]).cpu().reshape(-1)) and bool(im["depth"].any())
    assert torch.equal(rd("lidar_near.f32", np.int32), bits(im["near"]).cpu().reshape(-1))
    assert torch.equal(rd("lidar_index.i32", np.int32), im["index"].cpu().reshape(-1))
    assert int(rd("lidar_count.i32", np.int32)[0]) == int(im["n_measured"]) > 0
    P = m.P
    for n, f in (("xyz", "xyz"), ("features_dc", "dc"), ("features_rest", "rest"), ("opacity", "opacity"), ("scaling", "scaling"), ("rotation", "rotation")):
        for pre, src in (("", m._buf), ("m_", m._m), ("v_", m._v)):
            assert torch.equal(rd(pre + f + ".f32", np.int32), bits(src[n][:P]).cpu().reshape(-1)), pre + f
    assert torch.equal(rd("max_w.i32", np.int32), st._max[:P].cpu()) and torch.equal(rd("n_pix.i32", np.int32), st._npix[:P].cpu())
    assert torch.equal(rd("sum_w.i64", np.int64), st.sum_fixed().cpu())
    assert torch.equal(rd("free_sum.i64", np.int64), st.free_fixed().cpu()) and torch.equal(rd("meas_sum.i64", np.int64), st.measured_fixed().cpu())
    assert bool(st.free_fixed().any()) and bool(st.measured_fixed().any())
    st.detach()
