"""CPU-only: the C ABI of the LiDAR depth image (gslic_lidar_zbuffer_add / gslic_lidar_zbuffer_resolve) — the exports, every argument check (each
returns before any device work: without a GPU a HIP call would fail, not pass; the pointers are dummies that are never dereferenced) — and the
numpy reference of tests/lidar_depth_ref.py held against Camera.project_depth on CPU tensors for the clouds of test_lidar_depth_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lidar_depth_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = ctypes.c_void_p
INVALID = -1   # GSLIC_ERR_INVALID_ARG
A, B, C, D = 0x10000000, 0x20000000, 0x30000000, 0x40000000   # far apart: nothing overlaps unless a case makes it


def _lib():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    return _lib


def test_exports_and_abi_version():
    _l = _lib()
    with open(os.path.join(ROOT, "include", "gslic_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+GSLIC_ABI_VERSION\s+8\b", header)
    for name in ("gslic_lidar_zbuffer_add", "gslic_lidar_zbuffer_resolve"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _l.EXPORTS and hasattr(_l.lib(), name)
    assert _l.lib().gslic_abi_version() == 8


ADD_OK = dict(n=10, points=A, R_cw=B, t_cw=C, fx=30.0, fy=30.0, cx=16.0, cy=12.0, width=32, height=24, zbuf=D, clear=1, index_base=0, stream=None)
ADD_CASES = [
    (dict(n=-1), "n"),
    (dict(width=0), "width"),
    (dict(width=-3), "width"),
    (dict(height=0), "height"),
    (dict(zbuf=None), "zbuf"),
    (dict(zbuf=None, n=0), "zbuf"),
    (dict(points=None), "points"),
    (dict(R_cw=None), "R_cw"),
    (dict(t_cw=None), "t_cw"),
    (dict(index_base=-1), "index_base"),
    (dict(index_base=2 ** 31 - 10, n=10), "index_base"),     # index_base + n = 2^31 > 2^31 - 1
    (dict(index_base=1, n=2 ** 31 - 1), "index_base"),
]
RES_OK = dict(width=32, height=24, zbuf=A, footprint=0, margin_abs=0.0, margin_rel=0.0, depth_out=B, index_out=C, near_out=D, n_measured_out=None,
              stream=None)
NB = 32 * 24 * 8   # bytes of the z-buffer
RES_CASES = [
    (dict(width=0), "width"),
    (dict(height=-1), "height"),
    (dict(zbuf=None), "zbuf"),
    (dict(footprint=-1), "footprint"),
    (dict(footprint=9), "footprint"),
    (dict(margin_abs=-0.5), "margin_abs"),
    (dict(margin_abs=float("nan")), "margin_abs"),
    (dict(margin_rel=-1e-9), "margin_rel"),
    (dict(margin_rel=float("nan")), "margin_rel"),
    (dict(depth_out=None, index_out=None, near_out=None), "depth_out, index_out and near_out"),
    (dict(depth_out=None, index_out=None, near_out=None, n_measured_out=B), "depth_out, index_out and near_out"),
    (dict(depth_out=A), "depth_out"),                          # the same address
    (dict(depth_out=A + NB - 4), "depth_out"),                 # its first word is zbuf's last four bytes
    (dict(index_out=A - 32 * 24 * 4 + 4), "index_out"),         # its last word is zbuf's first four bytes
    (dict(near_out=A + 64), "near_out"),
    (dict(n_measured_out=A + NB - 4), "n_measured_out"),
]


def _call(fn, ok, change):
    _l = _lib()
    a = dict(ok, **change)
    p = lambda v: None if v is None else vp(v)
    if fn == "add":
        rc = _l.lib().gslic_lidar_zbuffer_add(a["n"], p(a["points"]), p(a["R_cw"]), p(a["t_cw"]), a["fx"], a["fy"], a["cx"], a["cy"], a["width"], a["height"],
                                              p(a["zbuf"]), a["clear"], a["index_base"], a["stream"])
    else:
        rc = _l.lib().gslic_lidar_zbuffer_resolve(a["width"], a["height"], p(a["zbuf"]), a["footprint"], a["margin_abs"], a["margin_rel"], p(a["depth_out"]),
                                                  p(a["index_out"]), p(a["near_out"]), p(a["n_measured_out"]), a["stream"])
    return rc, _l.lib().gslic_last_error().decode()


@pytest.mark.parametrize("change,names", ADD_CASES, ids=[f"{i}:{n}" for i, (_c, n) in enumerate(ADD_CASES)])
def test_add_refuses_bad_arguments(change, names):
    rc, msg = _call("add", ADD_OK, change)
    assert rc == INVALID and msg.startswith("lidar zbuffer add:") and names in msg, (rc, msg)


@pytest.mark.parametrize("change,names", RES_CASES, ids=[f"{i}:{n.split(',')[0]}" for i, (_c, n) in enumerate(RES_CASES)])
def test_resolve_refuses_bad_arguments(change, names):
    rc, msg = _call("resolve", RES_OK, change)
    assert rc == INVALID and msg.startswith("lidar zbuffer resolve:") and names in msg, (rc, msg)
    if "overlaps" in msg:
        assert msg.endswith("overlaps zbuf")


def test_python_layer_refuses_before_the_library():
    from gaussian_lic_amd import trainer
    with pytest.raises(ValueError, match="must not be empty"):
        trainer.LidarDepth(0, 4, "cpu")


# ------------------------------------------------------------------------------------------- the reference against Camera.project_depth (CPU tensors)
@pytest.mark.parametrize("W,H", lr.SIZES)
def test_reference_equals_project_depth_at_footprint_0(W, H):
    seen = 0
    for view in lr.VIEWS:
        cam = lr.camera(W, H, view)
        for n in lr.COUNTS:
            pts, _notes = lr.cloud(W, H, n, view)
            want = cam.project_depth(torch.from_numpy(pts.copy())).numpy()
            got = lr.images_of(W, H, n, view)
            assert np.array_equal(got["depth"].view(np.int32), want.view(np.int32)), (view, n)
            assert np.array_equal(got["index"] == -1, want == 0) and got["n_measured"] == int((want > 0).sum())
            seen += got["n_measured"]
    assert seen > 0


def test_planted_points_do_what_they_say():
    """On the identity camera, by the reference rule: the edge points land on pixel 0 / the last pixel or are dropped, the behind / zero / NaN /
    infinite points are dropped, the bit-equal pair's pixel goes to the lower index."""
    for W, H in lr.SIZES:
        cam = lr.camera(W, H)
        R, t = lr.pose_f32(cam)
        pl, notes = lr.planted(cam)
        proj = [lr._project(p, R, t, cam.fx, cam.fy, cam.cx, cam.cy) for p in pl]
        for k in (8, 9, 10, 11, 13):                       # z = 0, z < 0, NaN z, +inf z, behind the camera
            assert not (proj[k][2] > 0 and proj[k][2] < np.inf), k
        assert 0 <= proj[13][0] < W and 0 <= proj[13][1] < H          # ... which would have landed inside
        assert np.isnan(proj[12][0])                                  # a NaN coordinate (NaN * 0 makes z NaN as well)
        e = len(pl) - 8
        for axis, size in ((0, W), (1, H)):
            vals = [proj[e + 4 * axis + j][axis] for j in range(4)]
            assert vals == [-1.0, 0.0, float(size - 1), float(size)], (axis, vals)
        a, b = notes["equal_z"]
        assert np.array_equal(pl[a].view(np.int32), pl[b].view(np.int32)) and a < b
        zb = lr.zbuffer_add(lr.empty(W, H), pl, R, t, cam.fx, cam.fy, cam.cx, cam.cy, W, H)
        im = lr.resolve(zb, W, H)
        assert im["index"][0, 2] == a and im["index"][2, 3] == 1 and im["index"][1, 1] == 4       # nearest of three, nearest of two
        assert im["depth"][2, 3] == 2.0 and im["depth"][1, 1] == 2.5 and im["depth"][0, 2] == 0.25
        assert im["n_measured"] >= 3 + 3                   # the three shared pixels and at least the kept edge points' pixels
