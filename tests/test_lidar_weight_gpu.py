"""-m gpu: the weighted LiDAR resolve (gslic_lidar_zbuffer_resolve_weighted, trainer.LidarDepth.resolve(weight=, dist2=), gslic::LidarDepth).

Every comparison is on bits; the rule has no tolerance.  The yardstick is the numpy restatement of tests/lidar_weight_ref.py (a brute-force scan of
the window's cells, pinned by test_lidar_weight_cpu.py), trainer.range_weight on the depth image COPIED TO THE CPU, and the existing
gslic_lidar_zbuffer_resolve for the four images both calls write.  Nothing is compared with a division made by torch on the GPU.

Every case goes through the C ABI on a side stream with guard words around the z-buffer and the six outputs, five times over.  The (falloff,
sigma_rel) pair rotates through FALLOFFS x SIGMAS from case to case and footprint to footprint, so every pair meets every footprint and size; a
second call at falloff 0 is held against range_weight.  There is no figure to report: the images are equal or they are not."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import fused_check_io as fio
import lidar_depth_ref as lr
import lidar_weight_ref as wr
from gpu_helpers import SENTINEL, assert_same_state, bits, gpu, guarded, guards_intact, model_state, scene_model

pytestmark = pytest.mark.gpu

SENTINEL64 = 0x5A5A5A5A5A5A5A5A
MARGINS = (0.1, 0.02)
COMBOS = list(itertools.product(wr.FALLOFFS, wr.SIGMAS))   # 3 x 2
F32_IMAGES, ALL_IMAGES = ("depth", "near", "weight"), ("depth", "index", "near", "weight", "dist2")


def _trainer():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    return trainer


def _L():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def _side():
    return torch.cuda.Stream()


def _range_weight_cpu(depth_bits, sigma_abs, sigma_rel):
    """trainer.range_weight of a depth image given as its int32 bits on the CPU: the bits of the weight, computed on the CPU."""
    assert depth_bits.device.type == "cpu"
    return bits(_trainer().range_weight(depth_bits.view(torch.float32), sigma_abs, sigma_rel))


class _Buffer:
    """A z-buffer of W x H keys on the device between guard words."""

    def __init__(self, zb, W, H):
        self.W, self.H, self.N = W, H, W * H
        self.host = np.ascontiguousarray(zb, np.uint64)
        self.buf, self.words = guarded(self.N, torch.int64, sentinel=SENTINEL64)
        self.words.copy_(torch.from_numpy(self.host.view(np.int64)))

    def call(self, r, sigmas=None, falloff=0.0, weighted=True):
        """One call through the C ABI on the side stream, every output between guard words: gslic_lidar_zbuffer_resolve_weighted (weighted=True)
        or gslic_lidar_zbuffer_resolve.  Returns the images as int32 CPU tensors [H,W] (the floats as their bits) and "n_measured"."""
        _lib = _L()
        L, N = _lib.lib(), self.N
        names = ALL_IMAGES if weighted else ("depth", "index", "near")
        out = {k: guarded(N) for k in names}
        cnt = guarded(1)
        side = _side()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            sp = ctypes.c_void_p(side.cuda_stream)
            p = lambda k: _lib.ptr(out[k][1])
            if weighted:
                sa, sr = sigmas
                _lib.check(L.gslic_lidar_zbuffer_resolve_weighted(self.W, self.H, _lib.ptr(self.words), r, MARGINS[0], MARGINS[1], sa, sr, falloff,
                                                                  p("depth"), p("index"), p("near"), _lib.ptr(cnt[1]), p("weight"), p("dist2"), sp))
            else:
                _lib.check(L.gslic_lidar_zbuffer_resolve(self.W, self.H, _lib.ptr(self.words), r, MARGINS[0], MARGINS[1], p("depth"), p("index"),
                                                         p("near"), _lib.ptr(cnt[1]), sp))
        side.synchronize()
        assert guards_intact(self.buf, N, SENTINEL64) and guards_intact(cnt[0], 1)
        assert torch.equal(self.words.cpu(), torch.from_numpy(self.host.view(np.int64)))                   # zbuf is only read
        for k in names:
            assert guards_intact(out[k][0], N), k
        res = {k: out[k][1].reshape(self.H, self.W).cpu().clone() for k in names}
        res["n_measured"] = int(cnt[1][0])
        return res


def _same(a, b, names):
    return all(torch.equal(a[k], b[k]) for k in names) and a["n_measured"] == b["n_measured"]


def _check_buffer(zb, W, H, turn):
    """Everything the issue asks of one z-buffer, at every footprint.  Returns the restatement's images per footprint."""
    z = _Buffer(zb, W, H)
    refs = {}
    for i, r in enumerate(wr.FOOTPRINTS):
        falloff, (sa, sr) = COMBOS[(turn + i) % len(COMBOS)]
        ref = wr.resolve_weighted(z.host, W, H, r, sa, sr, falloff)
        first = z.call(r, (sa, sr), falloff)
        tag = (W, H, turn, r, falloff, sr)
        assert torch.equal(first["dist2"], torch.from_numpy(ref["dist2"])), tag
        assert torch.equal(first["weight"], torch.from_numpy(ref["weight"].view(np.int32))), tag
        assert torch.equal(first["depth"], torch.from_numpy(ref["depth"].view(np.int32))) and torch.equal(first["index"], torch.from_numpy(ref["index"])), tag
        assert first["n_measured"] == ref["n_measured"], tag
        plain = z.call(r, weighted=False)                                                                  # the four images both calls write
        assert _same(first, plain, ("depth", "index", "near")), tag
        for _ in range(4):                                                                                 # five runs in all
            assert _same(first, z.call(r, (sa, sr), falloff), ALL_IMAGES), tag
        flat = first if falloff == 0.0 else z.call(r, (sa, sr), 0.0)                                       # falloff 0: range_weight at any footprint
        assert torch.equal(flat["weight"], _range_weight_cpu(flat["depth"], sa, sr)), tag
        assert torch.equal(flat["dist2"], first["dist2"])
        if r == 0:                                                                                         # footprint 0: range_weight at any falloff
            assert torch.equal(first["weight"], _range_weight_cpu(first["depth"], sa, sr)), tag
            assert torch.equal(first["dist2"], torch.where(first["index"] >= 0, 0, -1).int())
        assert torch.equal(first["dist2"] < 0, first["index"] < 0) and torch.equal(first["weight"] == 0, first["index"] < 0)
        refs[r] = ref
    return refs


# ------------------------------------------------------------------------------------------- 1. hand-written z-buffers
@pytest.mark.parametrize("W,H", wr.SIZES)
def test_hand_written_buffers(W, H):
    bufs = wr.planted_buffers(W, H)
    yy, xx = np.mgrid[0:H, 0:W]
    for turn, (name, zb) in enumerate(bufs.items()):
        refs = _check_buffer(zb, W, H, turn)
        # what the buffer was written for, read off the restatement the device has just been held to (so: of the device's images too)
        if name.startswith("corner") or name == "centre":
            (x, y), = [(int(i % W), int(i // W)) for i in np.nonzero(zb != wr.EMPTY)[0]]
            inside = (abs(xx - x) <= 8) & (abs(yy - y) <= 8)
            assert np.array_equal(refs[8]["dist2"], np.where(inside, (xx - x) ** 2 + (yy - y) ** 2, -1)), name
        if name == "empty":
            assert all(not refs[r]["weight"].any() and bool((refs[r]["dist2"] == -1).all()) for r in refs)
    if (W, H) == (130, 35):   # both sides of both seams: the nearer return on the far side of the seam wins, at the distance across it
        d2, idx = refs_of_seams(bufs["seams"], W, H)
        assert idx[2, 61] == 1 and d2[2, 61] == 4 and idx[2, 66] == 1 and d2[2, 66] == 9                    # (63, 2) seen from x = 61 and x = 66
        assert idx[9, 62] == 2 and d2[9, 62] == 4 and idx[9, 67] == 2                                       # (64, 9) seen from x = 62
        assert idx[13, 5] == 3 and d2[13, 5] == 4 and idx[17, 5] == 3                                       # (5, 15) seen from y = 13 and y = 17
        assert idx[14, 20] == 4 and d2[14, 20] == 4 and idx[18, 20] == 4                                    # (20, 16) seen from y = 14
        assert idx[15, 63] == 6 and d2[15, 63] == 2 and idx[16, 64] == 6 and d2[16, 64] == 0                # the diagonal pair across the corner


def refs_of_seams(zb, W, H):
    ref = wr.resolve_weighted(zb, W, H, 3, 0.05, 0.02, 0.25)
    return ref["dist2"], ref["index"]


def test_ties_overruled_pixels_and_repeated_keys():
    """The lower index wins an equal-z pair and dist2 follows the winner, not the nearer loser; a measured pixel overruled by a nearer neighbour
    has dist2 > 0; of one key planted twice the nearer copy counts.  On the device's images (37 x 23, through trainer.LidarDepth's own buffer)."""
    trainer = _trainer()
    W, H = 37, 23
    bufs = wr.planted_buffers(W, H)

    def device_images(name, r):
        ld = trainer.LidarDepth(W, H, gpu())
        ld._add_raw(0, None, None, None, 0.0, 0.0, 0.0, 0.0)
        ld._zbuf.copy_(torch.from_numpy(bufs[name].view(np.int64)))
        out = ld.resolve(footprint=r, index=True, weight=(0.05, 0.02, 0.25), dist2=True)
        return out["index"].cpu().numpy(), out["dist2"].cpu().numpy(), out["weight"].cpu().numpy(), out["depth"].cpu()
    idx, d2, _w, _d = device_images("equal_z", 3)
    assert idx[1, 7] == 10 and d2[1, 7] == 9 and idx[1, 9] == 10 and d2[1, 9] == 1 and idx[1, 8] == 10 and d2[1, 8] == 4
    idx, d2, w, d = device_images("overruled", 1)
    assert idx[2, 3] == 1 and d2[2, 3] == 1 and d2[2, 4] == 0
    rw = trainer.range_weight(d, 0.05, 0.02).numpy()
    assert w[2, 4] == rw[2, 4] and 0 < w[2, 3] < rw[2, 3]
    idx, d2, _w, _d = device_images("same_key_twice", 3)
    assert d2[1, 3] == 2 and d2[0, 1] == 0 and d2[2, 4] == 0 and idx[1, 3] == 3


# ------------------------------------------------------------------------------------------- 2. points through add()
@pytest.mark.parametrize("W,H", wr.SIZES)
def test_points_through_add(W, H):
    """0, 1, 257 and 4097 points twice over (two sweeps accumulated), seen from the identity camera and from one SE(3) pose.  The z-buffer that
    add() built (the merged kernel, held to its own reference by test_lidar_depth_gpu.py) is read back and handed to the restatement."""
    trainer = _trainer()
    grew = 0
    for turn, (n, view) in enumerate(itertools.product((0, 1, 257, 4097), (None, "se3_c"))):
        cam = lr.camera(W, H, view)
        a, b = lr.cloud(W, H, n, view, plant=False)[0], lr.cloud(W, H, n, view, seed=1, plant=False)[0]
        ld = trainer.LidarDepth(W, H, gpu())
        assert ld.add(cam, torch.from_numpy(a.copy()).to(gpu())) == 0 and ld.add(cam, torch.from_numpy(b.copy()).to(gpu())) == n
        zb = ld._zbuf.cpu().numpy().view(np.uint64)
        refs = _check_buffer(zb, W, H, turn)
        grew += refs[3]["n_measured"] - refs[0]["n_measured"]
        if n == 4097 and W * H > 64:
            assert int((refs[1]["dist2"] > 0).sum()) > 0 and bool(((refs[0]["index"] >= 0) & (refs[1]["dist2"] > 0)).any())   # overruled pixels occur
        # the Python host, on the side stream: the same images as the C ABI gave (= the restatement's)
        r = wr.FOOTPRINTS[turn % 4]
        falloff, (sa, sr) = COMBOS[turn % len(COMBOS)]
        side = _side()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            out = ld.resolve(footprint=r, margins=MARGINS, index=True, count=True, weight=(sa, sr, falloff), dist2=True)
        side.synchronize()
        ref = wr.resolve_weighted(zb, W, H, r, sa, sr, falloff)
        assert out["weight"].dtype == torch.float32 and out["dist2"].dtype == torch.int32 and out["weight"].shape == (H, W) == out["dist2"].shape
        assert torch.equal(bits(out["weight"]).cpu(), torch.from_numpy(ref["weight"].view(np.int32))), (n, view)
        assert torch.equal(out["dist2"].cpu(), torch.from_numpy(ref["dist2"])) and int(out["n_measured"]) == ref["n_measured"]
        plain = ld.resolve(footprint=r, margins=MARGINS, index=True, count=True)
        assert all(torch.equal(bits(out[k]), bits(plain[k])) for k in ("depth", "near", "index", "n_measured"))
        two = ld.resolve(footprint=r, weight=(sa, sr))                                                      # falloff defaults to 0
        assert set(two) == {"depth", "weight"} and torch.equal(bits(two["weight"]).cpu(), _range_weight_cpu(bits(two["depth"]).cpu(), sa, sr))
        assert set(ld.resolve(footprint=r, dist2=True)) == {"depth", "dist2"}
    assert grew > 0


def test_every_falloff_and_sigma_on_one_image():
    trainer = _trainer()
    W, H, n, view, r = 130, 35, 4097, "se3_c", 3
    ld = trainer.LidarDepth(W, H, gpu())
    ld.add(lr.camera(W, H, view), torch.from_numpy(lr.cloud(W, H, n, view, plant=False)[0].copy()).to(gpu()))
    zb = ld._zbuf.cpu().numpy().view(np.uint64)
    z = _Buffer(zb, W, H)
    seen = set()
    for falloff, (sa, sr) in COMBOS:
        ref, got = wr.resolve_weighted(zb, W, H, r, sa, sr, falloff), z.call(r, (sa, sr), falloff)
        assert torch.equal(got["weight"], torch.from_numpy(ref["weight"].view(np.int32))) and torch.equal(got["dist2"], torch.from_numpy(ref["dist2"]))
        seen.add(got["weight"].numpy().tobytes())
        far = torch.from_numpy(ref["dist2"] > 0)
        rw = _range_weight_cpu(got["depth"], sa, sr).view(torch.float32)
        w = got["weight"].view(torch.float32)
        assert bool(far.any()) and (bool((w[far] < rw[far]).all()) if falloff > 0 else torch.equal(w, rw))
        if falloff == 1e30:
            assert bool((w[far] < 1e-29).all()) and bool((w[far] > 0).all())
    assert len(seen) == len(COMBOS)
    got = z.call(r, (1.0, 3e38), 3e38)   # products that overflow to +inf: weight 0, which the depth loss reads as unmeasured
    ref = wr.resolve_weighted(zb, W, H, r, 1.0, 3e38, 3e38)
    assert torch.equal(got["weight"], torch.from_numpy(ref["weight"].view(np.int32)))
    assert not bool(got["weight"][torch.from_numpy(ref["dist2"] > 0)].any())


def test_without_the_options_resolve_makes_the_old_call(monkeypatch):
    trainer = _trainer()
    L = _L().lib()
    calls = []
    for name in ("gslic_lidar_zbuffer_resolve", "gslic_lidar_zbuffer_resolve_weighted"):
        fn = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, _fn=fn, _name=name: (calls.append((_name, len(a))), _fn(*a))[1])
    W, H = 37, 23
    ld = trainer.LidarDepth(W, H, gpu())
    ld.add(lr.camera(W, H), torch.from_numpy(lr.cloud(W, H, 257)[0].copy()).to(gpu()))
    old = ld.resolve(footprint=3, margins=MARGINS, index=True, count=True)
    assert calls == [("gslic_lidar_zbuffer_resolve", 11)] and set(old) == {"depth", "near", "index", "n_measured"}
    old = ld.resolve(footprint=3, weight=None, dist2=False)
    assert calls == [("gslic_lidar_zbuffer_resolve", 11)] * 2 and set(old) == {"depth"}
    ld.resolve(footprint=3, dist2=True)
    ld.resolve(footprint=3, weight=(0.05, 0.02, 0.25))
    assert calls[2:] == [("gslic_lidar_zbuffer_resolve_weighted", 16)] * 2
    assert trainer.lidar_depth_image(lr.camera(W, H), torch.from_numpy(lr.cloud(W, H, 257)[0].copy()).to(gpu())).shape == (H, W)
    assert calls[4:] == [("gslic_lidar_zbuffer_resolve", 11)]


# ------------------------------------------------------------------------------------------- 3. end to end
LAMBDA_DEPTH, HUBER, WEIGHT, FOOTPRINT, NPTS = 0.1, 0.1, (0.05, 0.02, 0.25), 3, 300


def test_library_weight_feeds_the_step_like_the_restatements():
    import contribution_ref as cr
    trainer = _trainer()
    from gaussian_lic_amd.synthetic import gt_image, lidar_scene
    W, H = cr.W_A, cr.H_A
    points = lidar_scene(NPTS, W, H, sh_degree=0, seed=21)["xyz"].contiguous().to(gpu())
    states = []
    for which in ("library", "restatement", "none"):
        m, cam = scene_model("a")
        m.training_setup()
        ld = trainer.LidarDepth(W, H, gpu())
        ld.add(cam, points)
        out = ld.resolve(footprint=FOOTPRINT, weight=WEIGHT, dist2=True)
        ref = wr.resolve_weighted(ld._zbuf.cpu().numpy().view(np.uint64), W, H, FOOTPRINT, *WEIGHT)
        assert torch.equal(bits(out["weight"]).cpu(), torch.from_numpy(ref["weight"].view(np.int32))) and ref["n_measured"] > W * H // 4
        assert int((ref["dist2"] > 0).sum()) > int((ref["dist2"] == 0).sum()) > 0                           # mostly borrowed depths
        weight = dict(library=out["weight"], restatement=torch.from_numpy(ref["weight"].copy()).to(gpu()), none=None)[which]
        trainer.training_step_fused(m, cam, gt_image(H, W).to(gpu()), torch.zeros(3, device=gpu()), gt_depth=out["depth"], lambda_depth=LAMBDA_DEPTH,
                                    depth_weight=weight, depth_huber=HUBER)
        torch.cuda.synchronize()
        states.append(model_state(m))
    assert_same_state(states[0], states[1])
    assert not torch.equal(states[0]["xyz"], states[2]["xyz"])                                              # the weight really took part


def test_fused_lidar_weight_cpp_host(tmp_path):
    """gslic::LidarDepth::resolve with weight and dist2 feeding FusedStep::step gives the Python host's images and its 18 parameter and moment
    arrays, bit for bit."""
    trainer = _trainer()
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import gt_image, lidar_scene, random_scene
    exe = fio.build("fused_lidar_weight")
    NP, W, H = 400, 64, 64
    dev = gpu()
    m = trainer.GaussianModel(random_scene(NP, W, H, sh_degree=3, seed=3), dev)
    m.training_setup()
    cam = synthetic_camera(W, H).to_device(dev)
    gt, bg = gt_image(H, W).to(dev), torch.zeros(3, device=dev)
    points = lidar_scene(600, W, H, sh_degree=0, seed=21)["xyz"].contiguous()
    R, t = lr.pose_f32(cam)
    d = str(tmp_path)
    fio.write_inputs(d, m, cam, gt=gt, points=points,
                     lidar=np.concatenate([R, t, np.array([cam.fx, cam.fy, cam.cx, cam.cy, *WEIGHT, LAMBDA_DEPTH, HUBER], np.float32)]))
    ld = trainer.LidarDepth(W, H, dev)
    ld.add(cam, points.to(dev))
    im = ld.resolve(footprint=FOOTPRINT, index=True, count=True, weight=WEIGHT, dist2=True)
    trainer.training_step_fused(m, cam, gt, bg, gt_depth=im["depth"], lambda_depth=LAMBDA_DEPTH, depth_weight=im["weight"], depth_huber=HUBER)
    r = fio.run(exe, d, str(NP), str(W), str(H), "3", "600", str(FOOTPRINT))
    assert f"lidar measured {int(im['n_measured'])} base 0" in r.stdout
    rd = functools.partial(fio.read, d)
    assert torch.equal(rd("lidar_depth.f32", np.int32), bits(im["depth"]).cpu().reshape(-1)) and bool(im["depth"].any())
    assert torch.equal(rd("lidar_weight.f32", np.int32), bits(im["weight"]).cpu().reshape(-1)) and bool(im["weight"].any())
    assert torch.equal(rd("lidar_index.i32", np.int32), im["index"].cpu().reshape(-1))
    assert torch.equal(rd("lidar_dist2.i32", np.int32), im["dist2"].cpu().reshape(-1)) and bool((im["dist2"] > 0).any())
    assert int(rd("lidar_count.i32", np.int32)[0]) == int(im["n_measured"]) > 0
    rows = fio.read_rows(d, M=15)
    assert len(rows) == 18
    for n, f in (("xyz", "xyz"), ("features_dc", "dc"), ("features_rest", "rest"), ("opacity", "opacity"), ("scaling", "scaling"), ("rotation", "rotation")):
        for pre, src in (("", m._buf), ("m_", m._m), ("v_", m._v)):
            assert torch.equal(rows[pre + f], bits(src[n][:m.P]).cpu().reshape(-1)), pre + f
