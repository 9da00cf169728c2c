"""No GPU: the contribution-statistics export is declared, bound and checks its arguments before any device work; the fixed-point helpers and
drop_mask on hand-made arrays; the float64 replay of tests/contribution_ref.py on the C oracle's lists (the seeds and w_min keep the replay's own
ambiguity at w_min within 2 % of the visible Gaussians, and the scenes have the shapes the GPU tests rely on)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import contribution_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _libs():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    return _lib, _lib.lib()


def _prm(_lib, P=8, W=40, H=24, no_color=0):
    return _lib.RasterParams(P, 0, 0, W, H, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0, 0, no_color, 0, None)


def test_export_is_declared_bound_and_abi_stays():
    _lib, L = _libs()
    assert "gslic_contribution_accumulate" in _lib.EXPORTS
    assert L.gslic_abi_version() == 8
    header = open(os.path.join(ROOT, "include", "gslic_hip.h")).read()
    decl = re.search(r"int gslic_contribution_accumulate\((.*?)\);", header, re.S)
    assert decl is not None
    args = [a for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",") if a.strip()]
    assert len(args) == 11 == len(L.gslic_contribution_accumulate.argtypes)
    assert "#define GSLIC_ABI_VERSION 8" in header.replace("  ", " ")


def test_argument_errors_come_before_any_device_work():
    """Every call here passes host addresses or NULL as device buffers: an implementation that launched anything would fault."""
    _lib, L = _libs()
    fn = L.gslic_contribution_accumulate
    junk = ctypes.c_void_p(0x1000)
    ok = _prm(_lib)

    def err(*a):
        rc = fn(*a)
        return rc, L.gslic_last_error().decode()

    rc, msg = err(None, 1, 1, junk, junk, junk, 0.05, junk, junk, junk, None)
    assert rc == -1 and "NULL" in msg
    rc, msg = err(ctypes.byref(ok), -1, 1, junk, junk, junk, 0.05, junk, junk, junk, None)
    assert rc == -1 and "negative" in msg
    rc, msg = err(ctypes.byref(ok), 1, -1, junk, junk, junk, 0.05, junk, junk, junk, None)
    assert rc == -1 and "negative" in msg
    rc, msg = err(ctypes.byref(_prm(_lib, P=-1)), 1, 1, junk, junk, junk, 0.05, junk, junk, junk, None)
    assert rc == -1 and "P=-1" in msg
    rc, msg = err(ctypes.byref(_prm(_lib, no_color=1)), 1, 1, junk, junk, junk, 0.05, junk, junk, junk, None)
    assert rc == -1 and "no_color" in msg
    rc, msg = err(ctypes.byref(ok), 1, 1, junk, junk, junk, float("nan"), junk, junk, junk, None)
    assert rc == -1 and "NaN" in msg
    for hole in range(3):
        bufs = [junk, junk, junk]
        bufs[hole] = None
        rc, msg = err(ctypes.byref(ok), 1, 1, *bufs, 0.05, junk, junk, junk, None)
        assert rc == -1 and "NULL" in msg
    # nothing to do: P == 0, R == 0, no output — returns 0 without touching a buffer
    assert fn(ctypes.byref(_prm(_lib, P=0)), 5, 5, junk, junk, junk, 0.05, junk, junk, junk, None) == 0
    assert fn(ctypes.byref(ok), 0, 0, None, None, None, 0.05, junk, junk, junk, None) == 0
    assert fn(ctypes.byref(ok), 5, 5, junk, junk, junk, 0.05, None, None, None, None) == 0


def test_fixed_point_helpers_round_trip():
    from gaussian_lic_amd.trainer import FIXED_FRAC_BITS, fixed_to_weight, weight_to_fixed
    assert FIXED_FRAC_BITS == 32
    x = torch.tensor([0.0, 2.0 ** -32, 1.0 / 255.0, 0.05, 0.99, 1.0, 255.99, 256.0, 12345.678], dtype=torch.float32)
    q = weight_to_fixed(x)
    assert q.dtype == torch.int64 and q[0] == 0 and q[1] == 1 and q[5] == 1 << 32 and q[7] == 256 << 32
    assert torch.equal(fixed_to_weight(q), x.double())                       # float32 weights in this range have no bits below 2^-32
    assert int(weight_to_fixed(torch.tensor(1.5 * 2.0 ** -32, dtype=torch.float64))) == 2      # ties to even
    assert int(weight_to_fixed(torch.tensor(2.5 * 2.0 ** -32, dtype=torch.float64))) == 2
    top = torch.tensor([-1, -(1 << 63)], dtype=torch.int64)                  # bit 63 set: an unsigned sum, not a negative one
    assert fixed_to_weight(top).tolist() == [float(2 ** 32), float(2 ** 31)]
    sums = torch.tensor([3 << 32, (1 << 40) + 5], dtype=torch.int64)
    assert fixed_to_weight(sums).tolist() == [3.0, 256.0 + 5.0 / 2 ** 32]


def test_drop_mask_on_hand_made_arrays():
    from gaussian_lic_amd.trainer import contribution_drop_mask
    t = float(np.float32(0.3))
    below = float(np.nextafter(np.float32(0.3), np.float32(0)))
    mw = torch.tensor([0.0, below, t, 0.9, 0.9, 0.0], dtype=torch.float32)
    npx = torch.tensor([0, 10, 10, 3, 4, (1 << 32) - 1], dtype=torch.int64)
    assert contribution_drop_mask(mw, npx).tolist() == [0] * 6
    assert contribution_drop_mask(mw, npx, max_weight_below=0.3).tolist() == [1, 1, 0, 0, 0, 1]      # strict: a row AT the limit stays
    assert contribution_drop_mask(mw, npx, pixels_below=4).tolist() == [1, 0, 0, 1, 0, 0]
    got = contribution_drop_mask(mw, npx, max_weight_below=0.3, pixels_below=4)
    assert got.dtype == torch.uint8 and got.tolist() == [1, 1, 0, 1, 0, 1]


def test_stats_object_on_a_cpu_model_tracks_the_rows():
    """The bookkeeping of ContributionStats without a kernel: sizes, zero fill, accessors, and the stale-rows error of a detached object."""
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    raw, _W, _H = cr.scene("a")
    m = trainer.GaussianModel(cr._clone(raw), torch.device("cpu"), capacity=200)
    st = trainer.ContributionStats(m)
    assert st._max.shape == st._npix.shape == st._sum.shape == (200,) and st.views == 0 and m._attached_stats() == [st]
    st._max[:3] = torch.tensor([0.5, 0.25, 0.0]).view(torch.int32)
    st._npix[:3] = torch.tensor([7, -1, 0], dtype=torch.int32)                 # -1: the bit pattern of 2^32 - 1
    st._sum[:3] = torch.tensor([7 << 31, 1 << 32, 0])
    assert st.max_weight().dtype == torch.float32 and st.max_weight()[:3].tolist() == [0.5, 0.25, 0.0]
    assert st.pixels()[:3].tolist() == [7, (1 << 32) - 1, 0]
    assert st.sum_weight()[:3].tolist() == [3.5, 1.0, 0.0] and st.mean_weight()[:3].tolist() == [0.5, 1.0 / ((1 << 32) - 1), 0.0]
    assert st.drop_mask(max_weight_below=0.3, pixels_below=1)[:3].tolist() == [0, 1, 1]
    st.detach()
    assert m._attached_stats() == []
    m._rows_version += 1                                                         # what prune() / extend() / resort() do
    with pytest.raises(RuntimeError, match="rows changed"):
        st.max_weight()
    del st
    st2 = trainer.ContributionStats(m)
    del st2
    import gc
    gc.collect()
    assert m._attached_stats() == []                                            # the model holds weak references only


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_replay_on_the_oracles_lists(name):
    lists = cr.oracle_lists(name)
    rep = cr.replay(**lists)
    r = lists["ranges"].astype(np.int64)
    lens = r[:, 1] - r[:, 0]
    covered = (1.0 - rep["final_T"]).sum()
    assert abs(rep["sum_w"].sum() - covered) <= 1e-9 * max(covered, 1.0)        # sum_g sum_w = sum_pixels (1 - final_T): the blend telescopes
    assert cr.band_share(rep) <= 0.02                                           # the replay alone decides the counts for >= 98 % of the Gaussians
    if name == "a":
        assert len(lens) == 6 and (lens > 0).all() and (rep["pairs"] > 0).sum() > 60 and 0 < (rep["n_lo"] > 0).sum() < (rep["pairs"] > 0).sum()
    elif name == "b":
        # every pixel stopped early: a stop means T (1 - alpha) < 1e-4 with alpha <= 0.99, i.e. final T < 1e-2
        assert lens.tolist() == [cr.P_B] and 128 < int(lists["n_contrib"].max()) < cr.P_B // 2 and rep["final_T"].max() < 1e-2
    else:
        assert len(lists["point_list"]) == 0 and not rep["pairs"].any()
