"""CPU-only: the keyframe store's rules as tests/keyframe_ref.py restates them (round trip, the encode rule at its edges), Camera.at_level against
the level-0 pixel assignment, the level sizes, and the argument checks of gslic_keyframe_decode / gslic_keyframe_encode, which need no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import keyframe_ref as ref


def _lib():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------------- the rules
def test_round_trip_holds_for_all_256_values():
    v = np.arange(256, dtype=np.uint8)
    d = ref.decode(v.reshape(16, 16))                                   # d(v) = (float)v * float32(1/255)
    assert d.dtype == np.float32 and np.array_equal(d.reshape(-1).view(np.int32), (v.astype(np.float32) * ref.C0).view(np.int32))
    assert np.array_equal(ref.quantise(d).reshape(-1), v)               # encode(d(v)) == v: decode(encode(d(v))) == d(v) bit for bit
    q = (v.astype(np.float32) / np.float32(255.0)).astype(np.float32)   # the float32 QUOTIENT v / 255 — not d(v) for 126 values — encodes to v too
    assert np.array_equal(ref.quantise(q), v)
    assert np.array_equal(ref.decode(ref.quantise(q).reshape(16, 16)).view(np.int32), d.view(np.int32))
    assert int((q.view(np.int32) != d.reshape(-1).view(np.int32)).sum()) == 126 and np.abs(q.view(np.int32) - d.reshape(-1).view(np.int32)).max() == 1
    assert d[0, 0] == 0.0 and d[15, 15] == np.float32(255.0) * ref.C0


def test_encode_rule_at_its_edges():
    vals, want = ref.edge_values()
    assert np.array_equal(ref.quantise(vals), want)                     # float32 numpy arithmetic against the exact-arithmetic restatement
    named = {float("nan"): 0, float("inf"): 255, float("-inf"): 0, -0.0: 0, 0.0: 0, 2.0: 255, -1.0: 0,
             float(np.nextafter(np.float32(1), np.float32(2))): 255, float(np.nextafter(np.float32(1), np.float32(0))): 255}
    for x, q in named.items():
        assert int(ref.quantise(np.float32(x))) == q, x
    k = np.arange(256, dtype=np.float32)
    for centre in (k * ref.C0, k / np.float32(255.0)):                  # one ulp either side of a level stays on it
        for up in (True, False):
            x = np.clip(np.nextafter(centre.astype(np.float32), np.float32(np.inf if up else -np.inf)), 0, None).astype(np.float32)
            assert np.array_equal(ref.quantise(x), np.arange(256))
    mid = ((k[:-1] + np.float32(0.5)) / np.float32(255.0)).astype(np.float32)
    got = ref.quantise(mid).astype(np.int64)
    assert ((got == np.arange(255)) | (got == np.arange(255) + 1)).all()   # a midpoint goes to one of its two neighbours: which, the product's rounding says
    assert got.tolist() == [ref.quantise_exact(x) for x in mid]


def test_decode_is_the_integer_block_sum_times_an_exact_scale():
    rng = np.random.default_rng(3)
    u8 = rng.integers(0, 256, (9, 67, 3), dtype=np.uint8)
    for l in ref.levels(67, 9):
        S = ref.block_sums(u8, l)
        Wl, Hl = ref.level_size(67, 9, l)
        assert S.shape == (Hl, Wl, 3) and int(S.max()) <= 255 * 4 ** l
        n = 1 << l
        assert int(S[Hl - 1, Wl - 1, 2]) == int(u8[(Hl - 1) * n:Hl * n, (Wl - 1) * n:Wl * n, 2].astype(np.int64).sum())
        out = ref.decode(u8, l)
        assert out.shape == (3, Hl, Wl)
        assert np.array_equal(out, (S.astype(np.float64) * (float(ref.C0) / 4 ** l)).astype(np.float32).transpose(2, 0, 1))   # the scaling is exact
    assert float(ref.scale(4)) * 256.0 == float(ref.C0)
    assert ref.decode(np.full((16, 16), 255, np.uint8), 4)[0, 0] == ref.decode(np.full((1, 1), 255, np.uint8))[0, 0]


def test_level_sizes():
    from gaussian_lic_amd.camera import synthetic_camera
    assert ref.level_size(67, 9, 2) == (16, 2)
    cam = synthetic_camera(67, 9).at_level(2)
    assert (cam.image_width, cam.image_height) == (16, 2)
    assert ref.levels(67, 9) == [0, 1, 2, 3] and ref.levels(4, 1) == [0] and ref.levels(130, 33) == [0, 1, 2, 3, 4]
    for bad in (-1, 5):
        with pytest.raises(ValueError, match="outside"):
            synthetic_camera(67, 9).at_level(bad)
    with pytest.raises(ValueError, match="no level"):
        synthetic_camera(67, 9).at_level(4)


# ---------------------------------------------------------------------------------------------------- the camera
@pytest.mark.parametrize("level", [1, 2, 3])
def test_at_level_assigns_the_floor_of_the_level_0_pixel(level):
    """10 000 seeded points through Camera.project_depth's own arithmetic at level 0 and at level l: the level-l pixel of every point is
    floor(pixel_0 / 2^l), and a point is dropped exactly when that lands in a remainder column or row.  Exact: the intrinsics are scaled by a power
    of two, so every float32 operation of the rule gives the level-0 result times 2^-l."""
    from gaussian_lic_amd.camera import Camera, rotation_ypr
    W, H = 203, 151                                                     # remainders at every level
    cam = Camera(W, H, 131.7, 140.3, 99.4, 71.9, rotation_ypr(7.0, -4.0, 3.0), np.array([0.1, -0.05, 0.2]))
    lv = cam.at_level(level)
    s = np.float32(2.0 ** -level)
    assert (lv.image_width, lv.image_height) == (W >> level, H >> level)
    for name in ("fx", "fy", "cx", "cy"):
        assert getattr(lv, name).dtype == np.float32 and getattr(lv, name) == getattr(cam, name) * s
        assert float(getattr(lv, name)) * 2 ** level == float(getattr(cam, name))                     # exact
    assert np.array_equal(lv.R_wc, cam.R_wc) and np.array_equal(lv.t_wc, cam.t_wc) and lv.znear == cam.znear and lv.zfar == cam.zfar
    assert np.array_equal(lv.world_view_transform, cam.world_view_transform)
    rng = np.random.default_rng(100 + level)
    pts = torch.from_numpy(np.concatenate([rng.uniform(-3, 3, (10000, 2)), rng.uniform(0.3, 6.0, (10000, 1))], axis=1).astype(np.float32))

    def pixels(c):
        """Camera.project_depth's pixel assignment, point by point (its own operations in its own order), without the z-buffer."""
        R_cw = torch.from_numpy(np.ascontiguousarray(c.R_wc.T.astype(np.float32)))
        t_cw = torch.from_numpy((-c.R_wc.T @ c.t_wc).astype(np.float32))
        pc = pts[:, 0:1] * R_cw[:, 0] + pts[:, 1:2] * R_cw[:, 1] + pts[:, 2:3] * R_cw[:, 2] + t_cw
        z = pc[:, 2]
        front = z > 0
        zs = torch.where(front, z, torch.ones_like(z))
        x = torch.floor((pc[:, 0] * float(c.fx)) / zs + float(c.cx)).long()
        y = torch.floor((pc[:, 1] * float(c.fy)) / zs + float(c.cy)).long()
        keep = front & (x >= 0) & (x < c.image_width) & (y >= 0) & (y < c.image_height)
        return x, y, keep, z

    x0, y0, keep0, z = pixels(cam)
    xl, yl, keepl, zl = pixels(lv)
    assert torch.equal(z, zl)
    fx0, fy0 = torch.div(x0, 2 ** level, rounding_mode="floor"), torch.div(y0, 2 ** level, rounding_mode="floor")
    assert torch.equal(xl, fx0) and torch.equal(yl, fy0)                                             # every point, kept or not
    assert torch.equal(keepl, keep0 & (fx0 < lv.image_width) & (fy0 < lv.image_height))
    assert int(keepl.sum()) > 3000 and int((keep0 & ~keepl).sum()) > 0                               # the image is hit, and the remainder strip too
    # and the depth image itself is the positive-minimum pool of the level-0 image
    assert np.array_equal(lv.project_depth(pts).numpy(), ref.positive_min_pool(cam.project_depth(pts).numpy(), level))


# ---------------------------------------------------------------------------------------------------- the C-ABI's argument checks (no GPU)
def _decode(L, W=8, H=4, level=0, color=0x10000, mask=None, frame=0x20000, n_frames=3, out=0x30000, weight=None):
    vp = lambda a: None if a is None else ctypes.c_void_p(a)
    rc = L.gslic_keyframe_decode(W, H, level, vp(color), vp(mask), vp(frame), n_frames, vp(out), vp(weight), None)
    return rc, L.gslic_last_error().decode()


def _encode(L, W=8, H=4, image=0x10000, mask=None, color=0x20000, mask_slab=None, capacity=3, slot=0):
    vp = lambda a: None if a is None else ctypes.c_void_p(a)
    rc = L.gslic_keyframe_encode(W, H, vp(image), vp(mask), vp(color), vp(mask_slab), capacity, slot, None)
    return rc, L.gslic_last_error().decode()


@pytest.mark.parametrize("kw,name", [
    (dict(W=0), "W"), (dict(H=-1), "H"), (dict(level=-1), "level"), (dict(level=5), "level"), (dict(W=3, level=2), "W_l"), (dict(H=1, level=1), "H_l"),
    (dict(color=None), "color_slab"), (dict(frame=None), "frame"), (dict(out=None), "out"), (dict(mask=0x40000), "weight_out"), (dict(n_frames=-1), "n_frames"),
    (dict(out=0x30004), "out is not 16-byte aligned"), (dict(color=0x10008), "color_slab is not 16-byte aligned"),
    (dict(mask=0x40001, weight=0x50000), "mask_slab is not 16-byte aligned"), (dict(mask=0x40000, weight=0x50004), "weight_out is not 16-byte aligned"),
])
def test_decode_refusals_name_the_argument(kw, name):
    rc, msg = _decode(_lib().lib(), **kw)
    assert rc == -1 and name in msg and msg.startswith("keyframe decode"), msg


@pytest.mark.parametrize("kw,name", [
    (dict(W=0), "W"), (dict(H=0), "H"), (dict(capacity=0), "capacity"), (dict(slot=-1), "slot"), (dict(slot=3), "slot"), (dict(image=None), "both NULL"),
    (dict(color=None), "color_slab"), (dict(mask=0x30000), "mask_slab"), (dict(image=0x10002), "image is not 4-byte aligned"),
    (dict(mask=0x30001, mask_slab=0x40000), "mask is not 4-byte aligned"), (dict(color=0x20004), "color_slab is not 16-byte aligned"),
    (dict(mask=0x30000, mask_slab=0x40008), "mask_slab is not 16-byte aligned"),
])
def test_encode_refusals_name_the_argument(kw, name):
    rc, msg = _encode(_lib().lib(), **kw)
    assert rc == -1 and name in msg and msg.startswith("keyframe encode"), msg


def test_exports_are_declared():
    _l = _lib()
    assert "gslic_keyframe_decode" in _l.EXPORTS and "gslic_keyframe_encode" in _l.EXPORTS and _l.lib().gslic_abi_version() == 8
