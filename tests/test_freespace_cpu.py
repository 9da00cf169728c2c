"""CPU-only: the free-space surface that needs no device — the float64 reference (tests/freespace_ref.py) on the C oracle's lists under constant
bounds, the condition on the random bound image of the GPU test (every class of pairs holds at least 10 % on both scenes), the floater rule and
the bound helper on hand-written cases, and the new export's argument checks (none of these cases may reach a HIP call: without a GPU it would
fail, not pass)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import contribution_ref as cr
import freespace_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def lists():
    """Per scene: the oracle's lists, its float32 depths and contribution_ref.replay's result — computed once, left unchanged."""
    out = {}
    for name in ("a", "b"):
        L = cr.oracle_lists(name)
        out[name] = (L, fr.oracle_depths(name), cr.replay(**L))
    return out


def _const(L, value):
    return np.full((L["H"], L["W"]), value, np.float32)


# ---------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("name", ["a", "b"])
def test_reference_under_constant_bounds(lists, name):
    L, z, base = lists[name]
    assert base["sum_w"].max() > 0.5
    inf = fr.replay(**L, depths=z, near=_const(L, np.inf))
    assert np.array_equal(inf["sum_w"], base["sum_w"])                       # the same walk as contribution_ref.replay
    assert np.array_equal(inf["free_sum"], inf["sum_w"]) and np.array_equal(inf["meas_sum"], inf["sum_w"])
    assert inf["classes"][0] == 0 and inf["classes"][2] == 0 and inf["classes"][1] == base["pairs"].sum()
    for v in (0.0, -1.0, np.nan):
        zero = fr.replay(**L, depths=z, near=_const(L, v))
        assert not zero["free_sum"].any() and not zero["meas_sum"].any() and np.array_equal(zero["sum_w"], base["sum_w"])
        assert zero["classes"][0] == base["pairs"].sum()
    vis = np.flatnonzero(base["pairs"] > 0)
    z0 = np.float32(np.median(z[vis]))
    mid = fr.replay(**L, depths=z, near=_const(L, z0))
    front = z < z0
    assert front[vis].any() and (~front)[vis].any()
    assert np.array_equal(mid["meas_sum"], base["sum_w"])
    assert np.array_equal(mid["free_sum"][front], base["sum_w"][front]) and not mid["free_sum"][~front].any()
    # the comparison is strict: a Gaussian AT the bound is not in front of it
    g = vis[np.argmin(np.abs(z[vis] - z0))]
    at = fr.replay(**L, depths=z, near=_const(L, z[g]))
    nxt = fr.replay(**L, depths=z, near=_const(L, np.nextafter(z[g], np.float32(np.inf))))
    assert at["free_sum"][g] == 0.0 and nxt["free_sum"][g] == base["sum_w"][g] > 0


@pytest.mark.parametrize("name", ["a", "b"])
def test_random_bound_image_fills_every_class(lists, name):
    """The CONDITION on the GPU test's image: on both scenes at least 10 % of the contributing pairs are unmeasured, 10 % measured and in front,
    10 % measured and not in front — seed and value range were picked for it (freespace_ref.BOUND_SEED / BOUND_RANGE)."""
    L, z, base = lists[name]
    near = fr.bound_image(name)
    assert near.dtype == torch.float32 and tuple(near.shape) == (L["H"], L["W"])
    n = near.numpy()
    assert np.isnan(n).sum() == 3 and (n < 0).sum() == 3 and np.isposinf(n).sum() == 3
    assert 0.3 < (n == 0).mean() < 0.5
    assert torch.equal(near.view(torch.int32), fr.bound_image(name).view(torch.int32))        # seeded: the same image in both test files
    rep = fr.replay(**L, depths=z, near=n)
    shares = fr.class_shares(rep)
    print(f"[freespace classes] scene {name}: unmeasured {shares[0]:.3f} in front {shares[1]:.3f} not in front {shares[2]:.3f}")
    assert rep["classes"].sum() == base["pairs"].sum()
    assert bool((shares >= fr.MIN_CLASS_SHARE).all())
    assert bool((rep["free_sum"] <= rep["meas_sum"]).all()) and bool((rep["meas_sum"] <= rep["sum_w"]).all())


# ---------------------------------------------------------------------------------------------------- the floater rule and the bound
def test_floater_mask_on_hand_written_accumulators():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd.trainer import contribution_floater_mask as fm, fixed_to_weight, weight_to_fixed
    one = 1 << 32
    top = -(1 << 63)                                   # bit 63 set: 2^31 as an unsigned 32.32 value
    #                 at the limit   just above     measured 0   below min   bit 63 (meas)  bit 63 (both)  all free  none free
    meas = torch.tensor([4 * one,     4 * one,       0,           one // 2,   top,           top,           3 * one,  3 * one])
    free = torch.tensor([2 * one,     2 * one + 1,   0,           one // 2,   one,           top,           3 * one,  0])
    assert fm(free, meas, 0.5).tolist() == [0, 1, 0, 1, 0, 1, 1, 0]                      # strict: exactly half stays
    assert fm(free, meas, 0.5, min_measured=1.0).tolist() == [0, 1, 0, 0, 0, 1, 1, 0]    # bit 63 reaches every limit (unsigned)
    assert fm(free, meas, 0.5, min_measured=3.0).tolist() == [0, 1, 0, 0, 0, 1, 1, 0]    # >=: a row AT min_measured counts
    assert fm(free, meas, 0.5, min_measured=3.5).tolist() == [0, 1, 0, 0, 0, 1, 0, 0]
    assert fm(free, meas, 0.0).tolist() == [1, 1, 0, 1, 1, 1, 1, 0]                      # measured == 0 never, free == 0 never (0 > 0 is false)
    assert fm(free, meas, 1.0).tolist() == [0] * 8                                       # free <= measured: nothing exceeds the whole
    out = fm(free, meas, 0.25)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (8,)
    # the rule written out: one float64 product, one comparison
    want = ((meas >= int(weight_to_fixed(1.0))) | (meas < 0)) & (meas != 0) & (fixed_to_weight(free) > np.float64(0.25) * fixed_to_weight(meas))
    assert torch.equal(fm(free, meas, 0.25, 1.0).bool(), want)
    assert float(fixed_to_weight(torch.tensor([top]))[0]) == 2.0 ** 31
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="free_fraction_above"):
            fm(free, meas, bad)
    for bad in (-1.0, float("nan"), 2.0 ** 31):
        with pytest.raises(ValueError, match="min_measured"):
            fm(free, meas, 0.5, min_measured=bad)


def test_free_space_bound_on_hand_written_depths():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd.trainer import free_space_bound
    d = torch.tensor([[0.0, -2.0, float("nan"), 10.0], [0.3, float("inf"), 1.0, 0.05]])
    got = free_space_bound(d, 0.1, 0.02)
    f = np.float32
    want = lambda x: f(x) - (f(0.1) + f(0.02) * f(x))            # the stated order, every step in float32
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 4)
    assert got[0, 0] == 0 and got[0, 1] == 0 and got[0, 2] == 0                          # not > 0: no measurement
    assert float(got[0, 3]) == float(want(10.0)) and float(got[1, 0]) == float(want(0.3)) and float(got[1, 2]) == float(want(1.0))
    assert torch.isnan(got[1, 1]) or got[1, 1] == float("inf")                           # inf - inf: either way the kernel's rule decides
    assert float(got[1, 3]) == float(want(0.05)) < 0                                     # the margin exceeds the depth: reads as not measured
    assert torch.equal(free_space_bound(d.double(), 0.0, 0.0)[0, 3:], torch.tensor([10.0]))
    assert torch.equal(free_space_bound(d, 0, 0)[1, 2:], torch.tensor([1.0, 0.05]))
    for ma, mr in ((-0.1, 0.0), (0.0, -1.0), (float("nan"), 0.0)):
        with pytest.raises(ValueError, match="margins"):
            free_space_bound(d, ma, mr)


def test_contribution_stats_refuses_a_bad_bound_before_any_launch():
    """accumulate_from validates free_space the way it validates error; the rasterizer wrapper keeps the three pointers together."""
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import rasterizer as rz
    t = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="go together"):
        rz.contribution_accumulate(4, 8, 8, 1, 1, None, None, None, 0.05, near_bound=torch.zeros(8, 8))
    with pytest.raises(ValueError, match="go together"):
        rz.contribution_accumulate(4, 8, 8, 1, 1, None, None, None, 0.05, free_sum=t, meas_sum=t)
    with pytest.raises(ValueError, match="two launches"):
        rz.contribution_accumulate(4, 8, 8, 1, 1, None, None, None, 0.05, error=torch.zeros(8, 8), err_sum=t, near_bound=torch.zeros(8, 8),
                                   free_sum=t, meas_sum=t)
    with pytest.raises(ValueError, match="near_bound must be"):
        rz.contribution_accumulate(4, 8, 8, 1, 1, None, None, None, 0.05, near_bound=torch.zeros(8, 9), free_sum=t, meas_sum=t)
    with pytest.raises(ValueError, match="accumulator"):
        rz.contribution_accumulate(4, 8, 8, 1, 1, None, None, None, 0.05, near_bound=torch.zeros(8, 8), free_sum=t[:2], meas_sum=t)


# ---------------------------------------------------------------------------------------------------- declared, bound, checked
def test_header_declares_and_lib_binds_the_export():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    L = _lib.lib()
    src = open(os.path.join(ROOT, "include", "gslic_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    name = "gslic_contribution_accumulate_free_space"
    decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\);", code, re.S)
    assert decl and len(decl.group(1).split(",")) == 14 == len(getattr(L, name).argtypes)
    assert name in _lib.EXPORTS
    assert "#define GSLIC_ABI_VERSION 8" in src and L.gslic_abi_version() == 8     # additive: the ABI number stays
    for line in ("Pixel p is MEASURED iff near_bound[p] > 0", "strict float32 <", "free_sum == meas_sum == sum_w bit for bit"):
        assert line in src, line


def _prm(_l, **over):
    v = dict(P=10, D=0, M=0, width=64, height=48, tan_fovx=1.0, tan_fovy=1.0, limx_neg=-1, limx_pos=1, limy_neg=-1, limy_pos=1, scale_modifier=1.0,
             prefiltered=0, debug=0, no_color=0, raw_params=0)
    v.update(over)
    return _l.RasterParams(*[v[k] for k in ("P", "D", "M", "width", "height", "tan_fovx", "tan_fovy", "limx_neg", "limx_pos", "limy_neg", "limy_pos",
                                            "scale_modifier", "prefiltered", "debug", "no_color", "raw_params")])


def test_free_space_validates_before_any_device_work():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib as _l
    L = _l.lib()
    buf, acc, near = vp(0x10000), vp(0x20000), vp(0x30000)
    f = lambda prm, R=5, B=5, g=buf, b=buf, i=buf, w=0.05, nb=near, fs=acc, ms=acc, base=acc: L.gslic_contribution_accumulate_free_space(
        ctypes.byref(prm), R, B, g, b, i, w, base, base, base, nb, fs, ms, None)
    for kw in (dict(nb=None), dict(fs=None), dict(ms=None)):
        assert f(_prm(_l), **kw) == -1 and b"near_bound" in L.gslic_last_error(), kw
        assert f(_prm(_l, P=0), **kw) == -1 and f(_prm(_l), R=0, **kw) == -1   # the three pointers are required whatever the sizes
    assert f(_prm(_l), R=-1) == -1 and b"negative" in L.gslic_last_error()
    assert f(_prm(_l), B=-1) == -1
    assert f(_prm(_l, no_color=1)) == -1 and b"no_color" in L.gslic_last_error()
    assert f(_prm(_l), w=float("nan")) == -1 and b"NaN" in L.gslic_last_error()
    assert f(_prm(_l), g=None) == -1 and b"NULL forward buffer" in L.gslic_last_error()
    assert f(_prm(_l), b=None) == -1 and f(_prm(_l), i=None) == -1
    assert f(_prm(_l, P=0)) == 0 and f(_prm(_l), R=0) == 0       # the early returns of gslic_contribution_accumulate
    assert f(_prm(_l, P=0), g=None, b=None, i=None) == 0
    assert f(_prm(_l, D=4)) == -1                               # check_params comes first
