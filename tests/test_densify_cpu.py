"""CPU-only: the densification surface that needs no device — the counter generator's known answers and statistics (tests/densify_ref.py, the
restatement the GPU tests hold the kernel against), the three new exports' argument checks (none of these cases may reach a HIP call: without a
GPU it would fail, not pass), the split threshold's conversion and grow_mask on hand-built integer accumulators."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import densify_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = ctypes.c_void_p


def _libs():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    return _lib, _lib.lib()


# ---------------------------------------------------------------------------------------------------- the generator
def test_hash_known_answers():
    """Validates the REFERENCE (tests/densify_ref.py, numpy only — this test does not touch the library and passes without it; the device generator is
    held to this restatement through the split-xyz comparison of test_densify_gpu.py).  Written down once from densify_ref; (seed 0, index 1) checked by hand: fmix32(0) = 0, so the key is fmix32(1) = 0x514e28b7 (MurmurHash3's
    published finaliser value), word(0) = fmix32(0x514e28b7 + 0x9e3779b9 = 0xef85a270) = 0x50653bed, u_0 = (2 (0x50653bed >> 9) + 1) / 2^24
    = 5268795 / 16777216."""
    assert int(dr.fmix32(0)) == 0 and int(dr.fmix32(1)) == 0x514E28B7 and int(dr.fmix32(0xFFFFFFFF)) == 0x81F16F39
    want = {(0, 0): (0x0, [0x92CA2F0E, 0x3CD6E3F3, 0x1B147DCC, 0x4C081DBF], [9620015, 3987171]),
            (0, 1): (0x514E28B7, [0x50653BED, 0xCC56A2EB, 0x9D03E637, 0x1362FF13], [5268795, 13391523]),
            (12345, 7): (0x93FB7174, [0xD6DAA89E, 0xB3986A0F, 0x0712471C, 0xB6BBB2D4], [14080681, 11769963]),
            (0xDEADBEEF, 4096): (0x369F9E6A, [0xF088B441, 0xDCCCD6A6, 0xEF354631, 0xA36499B2], [15763637, 14470359])}
    for (seed, o), (k, words, us) in want.items():
        assert int(dr.key(seed, [o])[0]) == k
        assert [int(dr.word(seed, [o], n)[0]) for n in range(4)] == words
        assert [int(dr.u24(seed, [o], n)[0]) for n in range(2)] == us
    assert (0x514E28B7 + 0x9E3779B9) & 0xFFFFFFFF == 0xEF85A270 and 2 * (0x50653BED >> 9) + 1 == 5268795
    # u_n is exact in float32 and strictly inside (0, 1)
    u = dr.u24(3, np.arange(4096), 5)
    assert u.min() >= 1 and u.max() < (1 << 24) and bool((u % 2 == 1).all())
    f32 = (u.astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float64)
    assert np.array_equal(f32, dr.uniform(3, np.arange(4096), 5))


@pytest.mark.parametrize("child", [0, 1])
def test_noise_is_standard_normal_over_2_17_keys(child):
    """Validates the REFERENCE's noise (numpy only; passes without the library, like test_hash_known_answers): |mean| < 0.01 and |var - 1| < 0.02 per
    component over 2^17 fixed keys."""
    z = dr.normal3(7, np.arange(1 << 17), child)          # fixed samples: deterministic
    assert np.abs(z.mean(0)).max() < 0.01 and np.abs(z.var(0) - 1.0).max() < 0.02
    assert not np.array_equal(z, dr.normal3(8, np.arange(1 << 17), child))
    assert not np.array_equal(dr.normal3(7, np.arange(64), 0), dr.normal3(7, np.arange(64), 1))


# ---------------------------------------------------------------------------------------------------- declared and bound
def test_header_declares_and_lib_binds_the_three_exports():
    _l, L = _libs()
    src = open(os.path.join(ROOT, "include", "gslic_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("gslic_contribution_accumulate_error", "gslic_densify_select", "gslic_densify_emit"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in _l.EXPORTS and hasattr(L, name)
    assert "#define GSLIC_ABI_VERSION 8" in src and L.gslic_abi_version() == 8     # additive: the ABI number stays
    assert len(L.gslic_contribution_accumulate_error.argtypes) == 13 and len(L.gslic_densify_select.argtypes) == 16
    assert len(L.gslic_densify_emit.argtypes) == 11
    for line in ("split[i]    = eligible[i] && (some scaling[i,j] > scaling_raw_split)", "clone[i]    = eligible[i] && !split[i]",
                 "u_n     = (2 * (word(n) >> 9) + 1) * 2^-24", "2^22 tile partials fit into a row"):
        assert line in src, line


def test_split_threshold_conversion():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd.trainer import densify_threshold
    for s in (0.01, 0.5, 1.0, 3.0):
        t = densify_threshold(s)
        assert t == float(np.float32(math.log(s))) and np.float32(t) == t
    assert densify_threshold(None) == math.inf and densify_threshold(math.inf) == math.inf
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="split_scale"):
            densify_threshold(bad)
    assert float(dr.SHRINK) == float(np.float32(0.4700036292457356))


# ---------------------------------------------------------------------------------------------------- argument checks
def _prm(_l, **over):
    v = dict(P=10, D=0, M=0, width=64, height=48, tan_fovx=1.0, tan_fovy=1.0, limx_neg=-1, limx_pos=1, limy_neg=-1, limy_pos=1, scale_modifier=1.0,
             prefiltered=0, debug=0, no_color=0, raw_params=0)
    v.update(over)
    return _l.RasterParams(*[v[k] for k in ("P", "D", "M", "width", "height", "tan_fovx", "tan_fovy", "limx_neg", "limx_pos", "limy_neg", "limy_pos",
                                            "scale_modifier", "prefiltered", "debug", "no_color", "raw_params")])


def test_contribution_error_validates_before_any_device_work():
    _l, L = _libs()
    buf, acc, err = vp(0x10000), vp(0x20000), vp(0x30000)
    f = lambda prm, R=5, B=5, g=buf, b=buf, i=buf, w=0.05, e=err, es=acc: L.gslic_contribution_accumulate_error(
        ctypes.byref(prm), R, B, g, b, i, w, acc, acc, acc, e, es, None)
    assert f(_prm(_l), e=None) == -1 and b"error image" in L.gslic_last_error()
    assert f(_prm(_l), es=None) == -1 and b"err_sum" in L.gslic_last_error()
    assert f(_prm(_l, P=0), e=None) == -1                      # the two pointers are required whatever the sizes
    assert f(_prm(_l), R=-1) == -1 and b"negative" in L.gslic_last_error()
    assert f(_prm(_l), B=-1) == -1
    assert f(_prm(_l, no_color=1)) == -1 and b"no_color" in L.gslic_last_error()
    assert f(_prm(_l), w=float("nan")) == -1 and b"NaN" in L.gslic_last_error()
    assert f(_prm(_l), g=None) == -1 and b"NULL forward buffer" in L.gslic_last_error()
    assert f(_prm(_l), b=None) == -1 and f(_prm(_l), i=None) == -1
    assert f(_prm(_l, P=0)) == 0 and f(_prm(_l), R=0) == 0       # the early returns of gslic_contribution_accumulate
    assert f(_prm(_l, P=0), g=None, b=None, i=None) == 0
    assert f(_prm(_l, D=4)) == -1                               # check_params comes first


def _select_args(_l, **over):
    names = ["P", "xyz", "dc", "opacity", "scaling", "rotation", "grow", "protect", "tie", "thr", "alloc", "ctx", "parent", "count", "split", "stream"]
    calls = []

    def _alloc(_ctx, n):
        calls.append(n)
        return None
    cb = _l.ALLOC_FN(_alloc)
    count, split = ctypes.c_int32(77), ctypes.c_int32(77)
    vals = dict(P=8, xyz=vp(0x10000), dc=vp(0x20000), opacity=vp(0x30000), scaling=vp(0x40000), rotation=vp(0x50000), grow=vp(0x60000), protect=None,
                tie=None, thr=0.0, alloc=cb, ctx=None, parent=vp(0x70000), count=ctypes.byref(count), split=ctypes.byref(split), stream=None)
    for k, v in over.items():
        assert k in vals
        vals[k] = _l.ALLOC_FN() if (k == "alloc" and v is None) else v
    return [vals[n] for n in names], calls, count, split, cb


def test_densify_select_validates_before_any_device_work():
    _l, L = _libs()
    args, calls, count, split, _cb = _select_args(_l, P=0)
    assert L.gslic_densify_select(*args) == 0 and count.value == 0 and split.value == 0 and calls == []     # P == 0: at once, no allocator call
    args, calls, _c, _s, _cb = _select_args(_l, P=0, xyz=None, grow=None, parent=None, alloc=None)
    assert L.gslic_densify_select(*args) == 0 and calls == []
    args, calls, _c, _s, _cb = _select_args(_l, P=-1)
    assert L.gslic_densify_select(*args) == -1 and b"negative P" in L.gslic_last_error() and calls == []
    args, calls, _c, _s, _cb = _select_args(_l, thr=float("nan"))
    assert L.gslic_densify_select(*args) == -1 and b"NaN" in L.gslic_last_error() and calls == []
    for k in ("count", "split"):
        args, calls, _c, _s, _cb = _select_args(_l, **{k: None})
        assert L.gslic_densify_select(*args) == -1 and b"NULL count" in L.gslic_last_error() and calls == []
    for k in ("xyz", "dc", "opacity", "scaling", "rotation", "grow", "parent", "alloc"):
        args, calls, count, split, _cb = _select_args(_l, **{k: None})
        assert L.gslic_densify_select(*args) == -1 and b"NULL pointer" in L.gslic_last_error(), k
        assert calls == [] and count.value == 0 and split.value == 0, k
    # a refusing allocator is reported, nothing is launched
    args, calls, _c, _s, _cb = _select_args(_l)
    assert L.gslic_densify_select(*args) == -3 and b"allocator" in L.gslic_last_error() and len(calls) == 1 and calls[0] >= 8 * 8


def _emit_args(_l, **over):
    six = lambda base, skip=(): (vp * 6)(*[(None if g in skip else base + 0x1000 * g) for g in range(6)])
    vals = dict(P=8, count=3, parent=vp(0x10000), M=15, param=six(0x100000), m=six(0x200000), v=six(0x300000), tie=None, thr=0.0, seed=1, stream=None)
    for k, v in over.items():
        assert k in vals
        vals[k] = v
    return [vals[n] for n in ("P", "count", "parent", "M", "param", "m", "v", "tie", "thr", "seed", "stream")], six


def test_densify_emit_validates_before_any_device_work():
    _l, L = _libs()
    ok = lambda **o: L.gslic_densify_emit(*_emit_args(_l, **o)[0])
    assert ok(P=0, count=0) == 0 and ok(count=0) == 0 and ok(count=0, parent=None, param=None, m=None, v=None) == 0
    for o in (dict(P=-1), dict(count=-1), dict(M=-1)):
        assert ok(**o) == -1 and b"negative" in L.gslic_last_error(), o
    assert ok(count=9) == -1 and b"every parent adds one row" in L.gslic_last_error()
    assert ok(P=0x7fffffff, count=5) == -1 and b"31 bits" in L.gslic_last_error()
    assert ok(thr=float("nan")) == -1 and b"NaN" in L.gslic_last_error()
    for k in ("parent", "param", "m", "v"):
        assert ok(**{k: None}) == -1 and b"NULL pointer" in L.gslic_last_error(), k
    six = _emit_args(_l)[1]
    for k, base in (("param", 0x100000), ("m", 0x200000), ("v", 0x300000)):
        for g in range(6):
            assert ok(**{k: six(base, skip=(g,))}) == -1 and f"group {g}".encode() in L.gslic_last_error(), (k, g)
    # features_rest may be absent at SH degree 0 — and only there (count = 0 keeps the valid case off the device)
    assert ok(M=0, count=0, param=six(0x100000, skip=(2,))) == 0
    assert ok(M=1, param=six(0x100000, skip=(2,))) == -1


# ---------------------------------------------------------------------------------------------------- grow_mask
def test_grow_mask_compares_integers():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd.trainer import contribution_grow_mask, weight_to_fixed
    one = 1 << 32
    lim = int(weight_to_fixed(2.5))
    assert lim == 5 * (one // 2)
    err = torch.tensor([0, lim - 1, lim, lim + 1, 1000 * one, -1, -(1 << 63)], dtype=torch.int64)   # the last two: bit 63 set, unsigned above every limit
    npix = torch.tensor([9, 9, 9, 9, 2, 9, 0])
    m = contribution_grow_mask(err, npix, 2.5)
    assert m.dtype == torch.uint8 and m.tolist() == [0, 0, 0, 1, 1, 1, 1]                        # strict
    assert contribution_grow_mask(err, npix, 2.5, min_pixels=3).tolist() == [0, 0, 0, 1, 0, 1, 0]
    assert contribution_grow_mask(err, npix, 0.0).tolist() == [0, 1, 1, 1, 1, 1, 1]
    # the limit is rounded to 32.32 once: 2^-33 rounds to even (0), 3 * 2^-33 to 2^-31
    assert contribution_grow_mask(torch.tensor([1], dtype=torch.int64), npix[:1], 2.0 ** -33).tolist() == [1]
    assert contribution_grow_mask(torch.tensor([2], dtype=torch.int64), npix[:1], 3 * 2.0 ** -33).tolist() == [0]
    with pytest.raises(ValueError, match="error_above"):
        contribution_grow_mask(err, npix, -1.0)


def test_stats_without_an_error_image_have_no_fourth_array_and_densify_of_an_empty_model():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    raw = dict(xyz=torch.zeros(0, 3), scaling=torch.zeros(0, 3), rotation=torch.zeros(0, 4), opacity=torch.zeros(0, 1),
               features_dc=torch.zeros(0, 1, 3), features_rest=torch.zeros(0, 15, 3), sh_degree=3)
    m = trainer.GaussianModel(raw, torch.device("cpu"))
    st = trainer.ContributionStats(m)
    assert st._err is None and st.error_fixed().numel() == 0 and st.grow_mask(1.0).numel() == 0
    k, n_split, parents = m.densify(torch.zeros(0, dtype=torch.bool), 1.0)
    assert (k, n_split) == (0, 0) and parents.dtype == torch.int64 and parents.numel() == 0 and m.layout_version == 0
    with pytest.raises(ValueError, match="grow"):
        m.densify(torch.zeros(3, dtype=torch.bool), 1.0)
    with pytest.raises(ValueError, match="split_scale"):
        m.densify(torch.zeros(0, dtype=torch.bool), 0.0)
