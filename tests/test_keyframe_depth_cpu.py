"""CPU-only: the keyframe store's depth rules as tests/keyframe_depth_ref.py restates them (the round trip on every code, the pyramid property, the
tie rule, the edge values of the seeded frames) and the argument checks of gslic_keyframe_decode_depth / gslic_keyframe_encode_depth, which need no
GPU."""
import ctypes

import numpy as np
import pytest

import keyframe_depth_ref as ref
import keyframe_ref as kref

STEPS = [2.0 ** -9, 2.0 ** -16, 1.0]


def _lib():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    return _lib


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------------- the rules
@pytest.mark.parametrize("step", STEPS)
def test_round_trip_holds_for_all_65536_codes(step):
    codes = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    d = ref.decode(codes, None, 0, step)
    assert d.dtype == np.float32 and np.array_equal(d.astype(np.float64), codes.astype(np.float64) * step)   # k * step is exact
    assert np.array_equal(ref.encode(d, step), codes)                                                        # encode(decode_0(c)) == c
    assert np.array_equal(_bits(ref.quantised(d, step)), _bits(d))
    assert d[0, 0] == 0.0 and float(d[255, 255]) == 65535 * step
    if step == 2.0 ** -9:
        assert abs(float(d[255, 255]) - 127.998) < 1e-3 and abs(step - 0.00195) < 1e-5


def test_step_must_be_a_power_of_two_in_range():
    for e in range(-16, 1):
        assert ref.step_ok(2.0 ** e)
    for bad in (2.0 ** -17, 2.0, 0.003, 0.0, -0.5, float("nan"), float("inf"), 3 * 2.0 ** -10):
        assert not ref.step_ok(bad), bad


@pytest.mark.parametrize("W,H", [(67, 9), (130, 33), (16, 16)])
@pytest.mark.parametrize("step", STEPS[:2])
def test_decode_at_a_level_is_the_positive_minimum_pool_of_level_0(W, H, step):
    depth, weight = ref.random_depth_frames(2, W, H, 5, step)
    for f in range(2):
        codes, wc = ref.encode(depth[f], step), ref.encode_weight(weight[f])
        d0 = ref.decode(codes, None, 0, step)
        assert np.array_equal(_bits(d0), _bits(ref.quantised(depth[f], step))) and int((d0 > 0).sum()) > 0 and int((d0 == 0).sum()) > 0
        for l in (1, 2, 3):
            if min(kref.level_size(W, H, l)) < 1:
                continue
            want = kref.positive_min_pool(d0, l)
            assert np.array_equal(_bits(ref.decode(codes, None, l, step)), _bits(want)), l
            dl, wl = ref.decode(codes, wc, l, step)
            assert np.array_equal(_bits(dl), _bits(want)), l                 # the weight never changes which depth wins
            assert dl.shape == (H >> l, W >> l) and bool(((wl > 0) <= (dl > 0)).all())
    assert W % 8 == 0 or (W >> 3) * 8 < W                                     # (67, 9) and (130, 33): remainder columns and rows at every level


def test_the_largest_weight_wins_a_tie_wherever_it_stands():
    step = ref.DEFAULT_STEP
    for pos in range(16):
        codes = np.full((4, 4), 900, np.uint16)
        codes[0, 0] = 901
        wc = np.full((4, 4), 10, np.uint8)
        wc.reshape(-1)[pos] = 200
        codes.reshape(-1)[pos] = 900
        d, w = ref.decode(codes, wc, 2, step)
        assert d.shape == (1, 1) and float(d[0, 0]) == 900 * float(step)
        assert _bits(w)[0, 0] == _bits(np.float32(200) * kref.C0)
    # a nearer return beats a heavier one; weight 0 of a measured pixel decodes to weight 0 with its depth
    codes, wc = np.array([[5, 4], [0, 9]], np.uint16), np.array([[255, 0], [255, 255]], np.uint8)
    d, w = ref.decode(codes, wc, 1, step)
    assert float(d[0, 0]) == 4 * float(step) and float(w[0, 0]) == 0.0
    d, w = ref.decode(np.zeros((2, 2), np.uint16), np.full((2, 2), 255, np.uint8), 1, step)
    assert float(d[0, 0]) == 0.0 and float(w[0, 0]) == 0.0                    # nothing measured: both 0
    d0, w0 = ref.decode(codes, wc, 0, step)
    assert np.array_equal(_bits(w0), _bits(np.where(codes != 0, wc.astype(np.float32) * kref.C0, 0)))


@pytest.mark.parametrize("step", STEPS[:2])
def test_the_seeded_frames_hold_every_edge_value(step):
    W, H = 67, 9
    depth, weight = ref.random_depth_frames(3, W, H, 11, step)
    s = np.float32(step)
    edges = ref.edge_depths(step)
    for f in range(3):
        d = depth[f]
        codes = ref.encode(d, step)
        flat = d.reshape(-1)
        assert int((d == 0).sum()) > H * W // 5                                        # unmeasured pixels
        assert np.isnan(flat).any() and np.isposinf(flat).any() and (flat < 0).any()   # NaN, +inf, negative
        with np.errstate(invalid="ignore"):
            low = (flat > 0) & (flat <= s * np.float32(0.4995))                        # below half a step
            assert low.any() and (codes.reshape(-1)[low] == 0).all()
            assert (codes == 65535).any() and ((flat >= np.float32(65535.5) * s) & np.isfinite(flat)).any()   # the last code and just beyond
            assert (codes.reshape(-1)[(flat >= np.float32(65535.5) * s)] == 0).all()
            assert (codes.reshape(-1)[~(flat > 0) | ~np.isfinite(flat)] == 0).all()
        for name in ("below_boundary", "at_boundary", "above_boundary"):               # within half a step of a code boundary, both sides
            assert np.isin(edges[name][:3], flat).all(), name
        # ties inside a level-1 block under different weights
        wc = ref.encode_weight(weight[f])
        c4 = codes[:H // 2 * 2, :W // 2 * 2].reshape(H // 2, 2, W // 2, 2).transpose(0, 2, 1, 3).reshape(-1, 4)
        w4 = wc[:H // 2 * 2, :W // 2 * 2].reshape(H // 2, 2, W // 2, 2).transpose(0, 2, 1, 3).reshape(-1, 4)
        ties = 0
        for c, w in zip(c4, w4):
            m = c[c > 0].min() if (c > 0).any() else 0
            ties += int(m > 0 and (c == m).sum() > 1 and len(set(w[c == m].tolist())) > 1)
        assert ties > 0
    k = np.array([1, 2, 77, 1000, 40000, 65533])
    assert np.array_equal(ref.encode(edges["below_boundary"], step), k) and np.array_equal(ref.encode(edges["at_boundary"], step), k + 1)
    assert np.array_equal(ref.encode(edges["half_step"], step), [1, 1]) and not ref.encode(edges["below_half_step"], step).any()
    assert (ref.encode(edges["last_code"], step) == 65535).all() and not ref.encode(edges["beyond"], step).any()
    assert not ref.encode(edges["not_finite_or_positive"], step).any()


# ---------------------------------------------------------------------------------------------------- the C-ABI's argument checks (no GPU)
def _decode(L, W=8, H=4, level=0, depth=0x10000, dweight=None, frame=0x20000, n_frames=3, step=2.0 ** -9, out=0x30000, wout=None):
    vp = lambda a: None if a is None else ctypes.c_void_p(a)
    rc = L.gslic_keyframe_decode_depth(W, H, level, vp(depth), vp(dweight), vp(frame), n_frames, step, vp(out), vp(wout), None)
    return rc, L.gslic_last_error().decode()


def _encode(L, W=8, H=4, depth=0x10000, weight=None, slab=0x20000, wslab=None, capacity=3, slot=0, step=2.0 ** -9):
    vp = lambda a: None if a is None else ctypes.c_void_p(a)
    rc = L.gslic_keyframe_encode_depth(W, H, vp(depth), vp(weight), vp(slab), vp(wslab), capacity, slot, step, None)
    return rc, L.gslic_last_error().decode()


BAD_STEPS = [(dict(step=0.003), "step"), (dict(step=3 * 2.0 ** -10), "step"), (dict(step=2.0 ** -17), "step"), (dict(step=2.0), "step"),
             (dict(step=0.0), "step"), (dict(step=-0.5), "step"), (dict(step=float("nan")), "step"), (dict(step=float("inf")), "step")]


@pytest.mark.parametrize("kw,name", BAD_STEPS + [
    (dict(W=0), "W"), (dict(H=-1), "H"), (dict(level=-1), "level"), (dict(level=5), "level"), (dict(W=3, level=2), "W_l"), (dict(H=1, level=1), "H_l"),
    (dict(depth=None), "depth_slab is NULL"), (dict(frame=None), "frame"), (dict(out=None), "depth_out is NULL"), (dict(dweight=0x40000), "dweight_out is NULL"),
    (dict(n_frames=-1), "n_frames"), (dict(out=0x30004), "depth_out is not 16-byte aligned"), (dict(depth=0x10008), "depth_slab is not 16-byte aligned"),
    (dict(dweight=0x40001, wout=0x50000), "dweight_slab is not 16-byte aligned"), (dict(dweight=0x40000, wout=0x50004), "dweight_out is not 16-byte aligned"),
])
def test_decode_depth_refusals_name_the_argument(kw, name):
    rc, msg = _decode(_lib().lib(), **kw)
    assert rc == -1 and name in msg and msg.startswith("keyframe decode depth"), msg


@pytest.mark.parametrize("kw,name", BAD_STEPS + [
    (dict(W=0), "W"), (dict(H=0), "H"), (dict(capacity=0), "capacity"), (dict(slot=-1), "slot"), (dict(slot=3), "slot"), (dict(depth=None), "depth is NULL"),
    (dict(slab=None), "depth_slab is NULL"), (dict(weight=0x30000), "dweight_slab is NULL"), (dict(depth=0x10002), "depth is not 4-byte aligned"),
    (dict(weight=0x30001, wslab=0x40000), "weight is not 4-byte aligned"), (dict(slab=0x20004), "depth_slab is not 16-byte aligned"),
    (dict(weight=0x30000, wslab=0x40008), "dweight_slab is not 16-byte aligned"),
])
def test_encode_depth_refusals_name_the_argument(kw, name):
    rc, msg = _encode(_lib().lib(), **kw)
    assert rc == -1 and name in msg and msg.startswith("keyframe encode depth"), msg


def test_exports_are_declared_and_the_abi_is_unchanged():
    _l = _lib()
    assert "gslic_keyframe_decode_depth" in _l.EXPORTS and "gslic_keyframe_encode_depth" in _l.EXPORTS and _l.lib().gslic_abi_version() == 8


def test_store_constructor_refusals():
    import torch
    from gaussian_lic_amd import trainer
    with pytest.raises(ValueError, match="depth_weights=True needs depths=True"):
        trainer.KeyframeStore(8, 4, 2, torch.device("cpu"), depth_weights=True)
    for bad in (0.003, 2.0, 2.0 ** -17, 0.0, float("nan")):
        with pytest.raises(ValueError, match="depth_step"):
            trainer.KeyframeStore(8, 4, 2, torch.device("cpu"), depths=True, depth_step=bad)
    st = trainer.KeyframeStore(8, 4, 2, torch.device("cpu"), masks=True, depths=True, depth_weights=True)
    assert st.has_depths and st.has_depth_weights and st.depth_step == 2.0 ** -9 and st.nbytes == 2 * 8 * 4 * (3 + 1 + 2 + 1)
    plain = trainer.KeyframeStore(8, 4, 2, torch.device("cpu"))
    assert not plain.has_depths and not plain.has_depth_weights and plain.nbytes == 2 * 8 * 4 * 3
    assert trainer.KeyframeStore(8, 4, 2, torch.device("cpu"), depths=True, depth_step=2.0 ** -16).nbytes == 2 * 8 * 4 * 5
