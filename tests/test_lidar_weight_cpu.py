"""CPU-only: the C ABI of the weighted LiDAR resolve (gslic_lidar_zbuffer_resolve_weighted) — the export, every argument check (each returns
before any device work: without a GPU a HIP call would fail, not pass; the pointers are dummies that are never dereferenced) — the ValueErrors of
trainer.LidarDepth.resolve(weight=, dist2=), and the numpy restatement of tests/lidar_weight_ref.py held against trainer.range_weight on CPU tensors
and against tests/lidar_depth_ref.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lidar_depth_ref as lr
import lidar_weight_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = ctypes.c_void_p
INVALID = -1   # GSLIC_ERR_INVALID_ARG
A, B, C, D, E, G = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000   # far apart: nothing overlaps unless a case makes it
NB = 32 * 24 * 8   # bytes of the z-buffer
NAN, INF = float("nan"), float("inf")


def _lib():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    return _lib


def test_export_and_abi_version():
    _l = _lib()
    with open(os.path.join(ROOT, "include", "gslic_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+GSLIC_ABI_VERSION\s+8\b", header)
    name = "gslic_lidar_zbuffer_resolve_weighted"
    assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert name in _l.EXPORTS and hasattr(_l.lib(), name)
    assert _l.lib().gslic_abi_version() == 8


OK = dict(width=32, height=24, zbuf=A, footprint=0, margin_abs=0.0, margin_rel=0.0, sigma_abs=0.05, sigma_rel=0.02, falloff=0.25, depth_out=B,
          index_out=C, near_out=D, n_measured_out=None, weight_out=E, dist2_out=G, stream=None)
NO_IMAGES = dict(depth_out=None, index_out=None, near_out=None, weight_out=None, dist2_out=None)
ALL_FIVE = "depth_out, index_out, near_out, weight_out and dist2_out"
CASES = [
    # what the plain resolve refuses
    (dict(width=0), "width"),
    (dict(height=-1), "height"),
    (dict(zbuf=None), "zbuf"),
    (dict(footprint=-1), "footprint"),
    (dict(footprint=9), "footprint"),
    (dict(margin_abs=-0.5), "margin_abs"),
    (dict(margin_abs=NAN), "margin_abs"),
    (dict(margin_rel=-1e-9), "margin_rel"),
    (dict(margin_rel=NAN), "margin_rel"),
    (NO_IMAGES, ALL_FIVE),
    (dict(NO_IMAGES, n_measured_out=B), ALL_FIVE),
    (dict(depth_out=A), "depth_out"),                          # the same address
    (dict(depth_out=A + NB - 4), "depth_out"),                 # its first word is zbuf's last four bytes
    (dict(index_out=A - 32 * 24 * 4 + 4), "index_out"),         # its last word is zbuf's first four bytes
    (dict(near_out=A + 64), "near_out"),
    (dict(n_measured_out=A + NB - 4), "n_measured_out"),
    # the sigmas and the falloff, with a weight image
    (dict(sigma_abs=0.0), "sigma_abs"),
    (dict(sigma_abs=-1.0), "sigma_abs"),
    (dict(sigma_abs=NAN), "sigma_abs"),
    (dict(sigma_abs=INF), "sigma_abs"),
    (dict(sigma_rel=-1e-9), "sigma_rel"),
    (dict(sigma_rel=NAN), "sigma_rel"),
    (dict(sigma_rel=INF), "sigma_rel"),
    (dict(falloff=-0.25), "falloff"),
    (dict(falloff=NAN), "falloff"),
    (dict(falloff=INF), "falloff"),
    # the two new images against the z-buffer
    (dict(weight_out=A), "weight_out"),
    (dict(weight_out=A + NB - 4), "weight_out"),
    (dict(weight_out=A - 32 * 24 * 4 + 4), "weight_out"),
    (dict(dist2_out=A + 64), "dist2_out"),
    (dict(dist2_out=A - 32 * 24 * 4 + 4), "dist2_out"),
]


def _call(change):
    _l = _lib()
    a = dict(OK, **change)
    p = lambda v: None if v is None else vp(v)
    rc = _l.lib().gslic_lidar_zbuffer_resolve_weighted(
        a["width"], a["height"], p(a["zbuf"]), a["footprint"], a["margin_abs"], a["margin_rel"], a["sigma_abs"], a["sigma_rel"], a["falloff"],
        p(a["depth_out"]), p(a["index_out"]), p(a["near_out"]), p(a["n_measured_out"]), p(a["weight_out"]), p(a["dist2_out"]), a["stream"])
    return rc, _l.lib().gslic_last_error().decode()


@pytest.mark.parametrize("change,names", CASES, ids=[f"{i}:{n.split(',')[0]}" for i, (_c, n) in enumerate(CASES)])
def test_resolve_weighted_refuses_bad_arguments(change, names):
    rc, msg = _call(change)
    assert rc == INVALID and msg.startswith("lidar zbuffer resolve weighted:") and names in msg, (rc, msg)
    if "overlaps" in msg:
        assert msg.endswith("overlaps zbuf")


def test_python_layer_refuses_before_the_library(monkeypatch):
    from gaussian_lic_amd import trainer
    ld = trainer.LidarDepth(4, 3, "cpu")
    reached = []
    monkeypatch.setattr(trainer.LidarDepth, "_add_raw", lambda self, *a: reached.append(a))   # the first library call resolve() would make
    for bad in ((0.0, 0.02), (-1.0, 0.02), (NAN, 0.02), (INF, 0.02), (0.05, -0.01), (0.05, NAN), (0.05, INF)):
        with pytest.raises(ValueError, match="sigma_abs must be > 0 and sigma_rel >= 0"):
            ld.resolve(weight=bad)
        with pytest.raises(ValueError, match="sigma_abs must be > 0 and sigma_rel >= 0"):   # ... the words range_weight uses
            trainer.range_weight(torch.ones(3, 4), *bad)
    for bad in (-0.25, NAN, INF):
        with pytest.raises(ValueError, match="falloff"):
            ld.resolve(weight=(0.05, 0.02, bad))
    for bad in ((0.05,), (0.05, 0.02, 0.25, 1.0), 0.05):
        with pytest.raises(ValueError, match="weight"):
            ld.resolve(weight=bad)
    assert not reached


# ------------------------------------------------------------------------------------------- the restatement, pinned
def test_restatement_at_distance_0_is_range_weight():
    """Footprint 0 (every measured pixel has s2 = 0) at any falloff, and falloff 0 at any footprint: trainer.range_weight of the depth image."""
    from gaussian_lic_amd import trainer
    W, H, n, view = 37, 23, 257, "se3_c"
    zb = lr.zbuffer_of(W, H, n, view)
    seen = 0
    for sa, sr in wr.SIGMAS + [(1.0, 3e38)]:                  # the last: sigma_rel * d overflows, the weight is 0
        for r, fo in [(0, f) for f in wr.FALLOFFS] + [(r, 0.0) for r in wr.FOOTPRINTS]:
            got = wr.resolve_weighted(zb, W, H, r, sa, sr, fo)
            want = trainer.range_weight(torch.from_numpy(got["depth"].copy()), sa, sr).numpy()
            assert np.array_equal(got["weight"].view(np.int32), want.view(np.int32)), (sa, sr, r, fo)
            assert np.array_equal(got["dist2"] == -1, got["depth"] == 0)
            if r == 0:
                assert set(np.unique(got["dist2"])) <= {-1, 0}
            seen += int((got["weight"] > 0).sum())
            if sr == 3e38:
                far = got["depth"] > 2
                assert bool(far.any()) and not got["weight"][far].any()
    assert seen > 0
    d = wr.F(7.25)
    for s2 in (0, 1, 2, 128):
        w = wr.weight_of(d, s2, 0.05, 0.02, 0.25)              # the scalar form of the same four steps
        rw = trainer.range_weight(torch.tensor([7.25]), 0.05, 0.02).numpy()[0]
        assert w == wr.F(rw * wr.F(wr.F(1.0) / wr.F(wr.F(1.0) + wr.F(wr.F(0.25) * wr.F(s2)))))
        assert (w == rw) == (s2 == 0)
    assert wr.weight_of(d, 1, 0.05, 0.02, 1e30) > 0 and wr.weight_of(d, 1, 0.05, 0.02, 3e38) > 0   # finite products: tiny, not 0
    assert wr.weight_of(d, 128, 0.05, 0.02, 3e38) == 0                                             # the product overflows: weight 0


@pytest.mark.parametrize("W,H", lr.SIZES)
def test_restatement_key_and_depth_equal_the_depth_reference(W, H):
    for view in (None, "se3_d"):
        for n in (1, 257, 4097):
            zb = lr.zbuffer_of(W, H, n, view)
            for r in wr.FOOTPRINTS:
                got, want = wr.resolve_weighted(zb, W, H, r, 0.05, 0.02, 0.25), lr.images_of(W, H, n, view, r)
                assert np.array_equal(got["depth"].view(np.int32), want["depth"].view(np.int32)), (view, n, r)
                assert np.array_equal(got["index"], want["index"]) and got["n_measured"] == want["n_measured"], (view, n, r)
                assert np.array_equal(got["key"] == wr.EMPTY, want["index"] == -1)
                hit = got["dist2"] >= 0
                assert np.array_equal(hit, want["index"] >= 0) and int(got["dist2"].max(initial=-1)) <= 2 * r * r


def test_restatement_on_the_planted_buffers():
    """The hand-written buffers do what their names say, by the restatement alone (37 x 23, footprint 8 unless noted)."""
    W, H, r = 37, 23, 8
    bufs = wr.planted_buffers(W, H)
    yy, xx = np.mgrid[0:H, 0:W]
    for name, (x, y) in dict(corner00=(0, 0), corner10=(W - 1, 0), corner01=(0, H - 1), corner11=(W - 1, H - 1), centre=(W // 2, H // 2)).items():
        got = wr.resolve_weighted(bufs[name], W, H, r, 0.05, 0.02, 0.25)
        inside = (abs(xx - x) <= r) & (abs(yy - y) <= r)
        assert np.array_equal(got["dist2"], np.where(inside, (xx - x) ** 2 + (yy - y) ** 2, -1)), name
        assert got["dist2"].max() == 2 * r * r and got["n_measured"] == int(inside.sum())
    got = wr.resolve_weighted(bufs["equal_z"], W, H, 1, 0.05, 0.0, 0.25)
    assert got["index"][1, 9] == 10 and got["dist2"][1, 9] == 1 and got["index"][1, 8] == 11 and got["index"][1, 10] == 10
    got = wr.resolve_weighted(bufs["equal_z"], W, H, 3, 0.05, 0.0, 0.25)
    assert got["index"][1, 7] == 10 and got["dist2"][1, 7] == 9           # the winner stands 3 away, the loser 1 away
    got = wr.resolve_weighted(bufs["overruled"], W, H, 1, 0.05, 0.02, 0.25)
    assert got["index"][2, 3] == 1 and got["dist2"][2, 3] == 1 and got["dist2"][2, 4] == 0
    got = wr.resolve_weighted(bufs["same_key_twice"], W, H, 3, 0.05, 0.02, 0.25)
    assert got["dist2"][1, 3] == min(4 + 1, 1 + 1) and got["dist2"][0, 1] == 0 and got["dist2"][2, 4] == 0
    got = wr.resolve_weighted(bufs["empty"], W, H, 8, 0.05, 0.02, 0.25)
    assert not got["weight"].any() and bool((got["dist2"] == -1).all()) and got["n_measured"] == 0
