"""CPU-only: the geometry-image surface that needs no device — the float64 reference (tests/geometry_ref.py) against the C oracle's float32 forward
on scenes a, b and e, the conditions on the scenes of the GPU test (scene e's three classes of pixels, the cap on ambiguous pixels), rows_under on
hand-made tensors, and the export's argument checks (none of these cases may reach a HIP call: without a GPU it would fail, not pass)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import geometry_ref as gr
from conftest import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = ctypes.c_void_p
TOL = 1e-4          # the bar the project applies to gradients (tests/refcompare.py: TOL; conftest.rel_err)


@pytest.fixture(scope="module")
def replays():
    """Per scene: (the oracle's lists, its float32 final_T, geometry_ref.replay's result) — computed once, left unchanged."""
    out = {}
    for name in ("a", "b", "e"):
        L, final_T = gr.oracle_forward(name)
        out[name] = (L, final_T, gr.replay(**L))
    return out


# ---------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("name", ["a", "b", "e"])
def test_replay_transmittance_is_the_oracles_final_T(replays, name):
    L, final_T, rep = replays[name]
    e = rel_err(rep["transmittance"], final_T)
    print(f"[geometry replay] scene {name}: transmittance vs the oracle's final_T rel_err {e:.3e}")
    assert e < TOL
    # what the rule implies for every pixel, whatever the scene
    A, T, D = rep["opacity"], rep["transmittance"], rep["depth_sum"]
    none = rep["n_pairs"] == 0
    assert np.allclose(A + T, 1.0, atol=1e-9)                              # sum of alpha T telescopes to 1 - T
    assert np.array_equal(rep["top_row"] == -1, none) and not rep["top_weight"][none].any() and not A[none].any() and not D[none].any()
    assert np.array_equal(rep["reached"], T < 0.5)                         # T only falls
    assert not rep["depth_median"][~rep["reached"]].any() and bool((rep["depth_median"][rep["reached"]] > 0).all())
    cov = ~none
    assert bool((rep["top_weight"][cov] > 0).all()) and bool((rep["top_weight"][cov] <= A[cov] * (1 + 1e-12)).all())
    z = np.asarray(L["depths"], np.float64)
    vis = np.unique(np.asarray(L["point_list"]).astype(np.int64))
    ok = A >= gr.A_MIN
    assert bool((rep["depth_norm"][ok] >= z[vis].min() * (1 - 1e-9)).all()) and bool((rep["depth_norm"][ok] <= z[vis].max() * (1 + 1e-9)).all())
    assert not rep["depth_norm"][~ok].any()


def test_scene_e_holds_every_class_of_pixels(replays):
    shares = gr.classes(replays["e"][2])
    print(f"[geometry scenes] scene e: no contributor {shares[0]:.4f}, covered / median not reached {shares[1]:.4f}, median reached {shares[2]:.4f}")
    assert min(shares) >= 0.10
    # ... and the second a_min of the GPU test moves at least 5 % of its pixels across the threshold
    A = replays["e"][2]["opacity"]
    moved = float(((A >= gr.A_MIN) & (A < gr.A_MIN_2)).mean())
    low = float(((A > 0) & (A < gr.A_MIN)).mean())
    print(f"[geometry scenes] scene e: covered with A < {gr.A_MIN}: {low:.4f}; {gr.A_MIN} <= A < {gr.A_MIN_2}: {moved:.4f}")
    assert moved >= 0.05 and low >= 0.05
    # scenes a and b have none of this, which is why e exists
    assert gr.classes(replays["a"][2])[0] == 0.0 and gr.classes(replays["b"][2])[0] == 0.0


@pytest.mark.parametrize("name", ["a", "b", "e"])
def test_ambiguous_pixels_stay_under_the_cap(replays, name):
    L = replays[name][0]
    for a_min in (gr.A_MIN, gr.A_MIN_2):
        shares = gr.ambiguous_shares(replays[name][2] if a_min == gr.A_MIN else gr.replay(**L, a_min=a_min))
        print(f"[geometry ambiguity] scene {name} a_min {a_min}: top_row {shares[0]:.4f} depth_median {shares[1]:.4f} depth_norm {shares[2]:.4f} (cap {gr.AMBIG_CAP})")
        assert max(shares) <= gr.AMBIG_CAP


def test_replay_of_empty_lists_gives_the_initial_values():
    rep = gr.replay(**gr.empty_lists(40, 24, 96))
    assert bool((rep["transmittance"] == 1.0).all()) and bool((rep["top_row"] == -1).all())
    for k in ("opacity", "depth_sum", "depth_norm", "depth_median", "top_weight"):
        assert not rep[k].any(), k


# ---------------------------------------------------------------------------------------------------- rows_under
def test_rows_under_on_hand_made_tensors():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    top = torch.tensor([[3, 3, -1, 0], [5, -1, 3, 1]], dtype=torch.int32)
    mask = torch.tensor([[1, 1, 1, 0], [0, 1, 1, 1]], dtype=torch.bool)
    got = trainer.rows_under(top, mask, 7)
    assert got.dtype == torch.bool and got.tolist() == [False, True, False, True, False, False, False]   # 3 three times, 1 once; 0 and 5 unmasked
    assert trainer.rows_under(top, torch.zeros(2, 4, dtype=torch.bool), 7).tolist() == [False] * 7         # an empty mask
    assert trainer.rows_under(top, torch.ones(2, 4, dtype=torch.bool), 7).tolist() == [True, True, False, True, False, True, False]
    assert trainer.rows_under(torch.full((2, 4), -1, dtype=torch.int32), torch.ones(2, 4, dtype=torch.bool), 3).tolist() == [False] * 3
    assert trainer.rows_under(top, mask.to(torch.uint8), 7).tolist() == got.tolist()                       # any tensor read as != 0
    assert trainer.rows_under(top, mask).shape == (6,)                                                     # default P: the largest row named + 1
    with pytest.raises(ValueError, match="rows_under"):
        trainer.rows_under(top, torch.ones(4, 2, dtype=torch.bool), 7)


# ---------------------------------------------------------------------------------------------------- declared, bound, checked
def test_header_declares_and_lib_binds_the_export():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    L = _lib.lib()
    src = open(os.path.join(ROOT, "include", "gslic_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    name = "gslic_geometry_images"
    decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\);", code, re.S)
    assert decl and len(decl.group(1).split(",")) == 15 == len(getattr(L, name).argtypes)
    assert name in _lib.EXPORTS
    assert "#define GSLIC_ABI_VERSION 8" in src and L.gslic_abi_version() == 8     # additive: the ABI number stays
    for line in ("D = D + (z alpha) T", "strict >: the frontmost wins a tie", "ONE IEEE float32 division", "There is NO fast-math variant"):
        assert line in src, line


def _prm(_l, **over):
    v = dict(P=10, D=0, M=0, width=64, height=48, tan_fovx=1.0, tan_fovy=1.0, limx_neg=-1, limx_pos=1, limy_neg=-1, limy_pos=1, scale_modifier=1.0,
             prefiltered=0, debug=0, no_color=0, raw_params=0)
    v.update(over)
    return _l.RasterParams(*[v[k] for k in ("P", "D", "M", "width", "height", "tan_fovx", "tan_fovy", "limx_neg", "limx_pos", "limy_neg", "limy_pos",
                                            "scale_modifier", "prefiltered", "debug", "no_color", "raw_params")])


def test_geometry_images_validates_before_any_device_work():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib as _l
    L = _l.lib()
    buf, img = vp(0x10000), vp(0x20000)
    # outs: the seven image pointers; every case below either fails a check or has no image to write, so no kernel is launched
    f = lambda prm, R=5, B=5, g=buf, b=buf, i=buf, a=0.05, outs=(img,) * 7: L.gslic_geometry_images(ctypes.byref(prm), R, B, g, b, i, a, *outs, None)
    assert f(_prm(_l), R=-1) == -1 and b"negative" in L.gslic_last_error()
    assert f(_prm(_l), B=-1) == -1
    assert f(_prm(_l, no_color=1)) == -1 and b"no_color" in L.gslic_last_error()
    assert f(_prm(_l), g=None) == -1 and b"NULL forward buffer" in L.gslic_last_error()
    assert f(_prm(_l), b=None) == -1 and f(_prm(_l), i=None) == -1
    only_norm = (None, None, None, img, None, None, None)
    for bad in (float("nan"), 0.0, -0.05, -float("inf")):
        assert f(_prm(_l), a=bad, outs=only_norm) == -1 and b"a_min" in L.gslic_last_error(), bad
        assert f(_prm(_l, P=0), a=bad, outs=only_norm) == -1 and f(_prm(_l), R=0, a=bad, outs=only_norm) == -1   # whatever the sizes
    assert f(_prm(_l, D=4)) == -1                               # check_params comes first
    assert f(_prm(_l, width=0)) == -1
    none = (None,) * 7
    assert f(_prm(_l), outs=none) == 0                           # nothing to write
    for bad in (float("nan"), 0.0, -1.0):                        # a_min is only read for depth_norm
        assert f(_prm(_l), a=bad, outs=none) == 0
    assert f(_prm(_l, P=0), outs=none) == 0 and f(_prm(_l), R=0, outs=none) == 0
    assert f(_prm(_l, P=0), g=None, b=None, i=None, outs=none) == 0 and f(_prm(_l), R=0, g=None, b=None, i=None, outs=none) == 0
    assert f(_prm(_l), g=None, outs=none) == -1                  # ... but the buffers of a forward with lists are checked first


def test_python_wrappers_check_their_arguments():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import rasterizer as rz, trainer
    img = torch.zeros(8, 8)
    with pytest.raises(ValueError, match="unknown image"):
        rz.geometry_images(4, 8, 8, 1, 1, None, None, None, 0.05, dict(depth=img))
    with pytest.raises(ValueError, match="top_row must be"):
        rz.geometry_images(4, 8, 8, 1, 1, None, None, None, 0.05, dict(top_row=img))
    with pytest.raises(ValueError, match="opacity must be"):
        rz.geometry_images(4, 8, 8, 1, 1, None, None, None, 0.05, dict(opacity=torch.zeros(8, 9)))
    with pytest.raises(ValueError, match="a_min must be > 0"):
        trainer._geometry_a_min(0.0, dict(depth_norm=img))
    assert trainer._geometry_a_min(0.0, dict(opacity=img)) == 0.0
    with pytest.raises(ValueError, match="no tensor for"):
        trainer._geometry_out(8, 8, "cpu", ("opacity", "top_row"), dict(opacity=img))
    with pytest.raises(ValueError, match="unknown image"):
        trainer._geometry_out(8, 8, "cpu", ("depth",), None)
    made = trainer._geometry_out(8, 8, "cpu", trainer.GEOMETRY_DEFAULT, None)
    assert tuple(made) == trainer.GEOMETRY_DEFAULT and made["top_row"].dtype == torch.int32 and made["opacity"].shape == (8, 8)
