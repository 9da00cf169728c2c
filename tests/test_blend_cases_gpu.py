"""-m gpu: the blend forward and backward on the designed scenes of tests/blend_cases.py — every structural edge of the kernels'
decomposition (group counts 1..4, pixel chunks and their padding record, the hand-off between groups of sixteen, the mask word seam, dead
buckets, inactive pixels, unblended entries, the image edge, a launch grid padded past B) reached on purpose, on an exact and on a ragged
image, in strict and in fast arithmetic, colour and depth.  tests/test_blend_cases_cpu.py proves on the CPU oracle that the scenes reach
those edges and keep every (pixel, entry) pair away from the blend's hard cuts: no comparison here has a flip allowance.

Integers (lists, n_contrib, max_contrib) are the oracle's with zero exceptions.  Floats are judged per case (blend_cases.judge): the
largest error against the fp64 oracle over the case's pixels / Gaussians, relative to the case's max-abs, at most FACTOR x max(the fp32
oracle's same figure, rowwise.FLOOR).  FACTOR: profiles/blend_cases_factors.txt (measured, doubled, rounded up; <= rowwise.MAX_FACTOR).
BLEND_CASES_REPORT=<file> appends every measured ratio to that file."""
import os

import numpy as np
import pytest
import torch

import blend_cases as bc
import rowwise as rw
from test_depth_gpu import _mode, bwd, fwd_depth, oracle_backward_depth, oracle_depth

pytestmark = pytest.mark.gpu

TENSORS = ("dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dcov3D")
_refs = {}


def _world(which, oracle32, oracle64):
    """the scene and both oracles' results on it: built once, never modified"""
    if which not in _refs:
        raw, sc, camd, cam, plan = bc.build(which)
        W, H = plan["W"], plan["H"]
        dL, gD = bc.pixel_grads(W, H)
        w = dict(raw=raw, cam=cam, plan=plan, dL=torch.from_numpy(dL), gD=torch.from_numpy(gD))
        for tag, orc in (("32", oracle32), ("64", oracle64)):
            f = orc.forward(sc, camd)
            w["f" + tag] = f
            w["depth" + tag] = oracle_depth(orc, f, W, H)[0]
            w["gc" + tag] = orc.backward(sc, camd, f, dL)
            w["gd" + tag] = oracle_backward_depth(orc, sc, camd, f, dL, gD)
        w["never"] = bc.never_blended_rows(w["f64"]["pre"], w["f64"]["bins"], plan)
        w["lists"] = bc.expected_case_lists(plan)
        _refs[which] = w
    return _refs[which]


def _report(what, ratio):
    path = os.environ.get("BLEND_CASES_REPORT")
    worst = max(ratio.items(), key=lambda kv: kv[1])
    print(f"\n[{what}] largest ratio {worst[1]:.3f} ({worst[0][0]}, case {worst[0][1]})")
    if path:
        with open(path, "a") as f:
            for (tensor, case), r in sorted(ratio.items()):
                f.write(f"{what:<28} {tensor:<12} {case:<14} {r:8.3f}\n")


def _image_ratios(got, ref32, ref64, plan, name):
    """judge() for an image: per case TILE"""
    bad, ratio = [], {}
    for c in plan["cases"]:
        x0, y0 = 16 * (c["tile"] % plan["gx"]), 16 * (c["tile"] // plan["gx"])
        sl = (Ellipsis, slice(y0, min(y0 + 16, plan["H"])), slice(x0, min(x0 + 16, plan["W"])))
        a, r32, r64 = (np.asarray(v, np.float64)[sl] for v in (got, ref32, ref64))
        scale = np.abs(r64).max()
        e, e32 = (np.abs(v - r64).max() / scale if scale > 0 else (np.inf if np.abs(v - r64).max() > 0 else 0.0) for v in (a, r32))
        bound = max(e32, rw.FLOOR)
        ratio[(name, c["name"])] = e / bound
        if not e <= bc.FACTOR * bound:
            cells = sorted(k for k, owner in bc.REQUIRED.items() if owner == c["name"])
            bad.append(f"case {c['name']} ({', '.join(cells)}): {name} off by {e:.3e} of the tile's max-abs, fp32 oracle {e32:.3e}, allowed {bc.FACTOR} x {bound:.3e}")
    return bad, ratio


def _first_bad_case(plan, got, want, what):
    """the designed case (and its cells) of the first pixel / tile whose integer differs"""
    if np.array_equal(got, want):
        return None
    for c in plan["cases"]:
        x0, y0 = 16 * (c["tile"] % plan["gx"]), 16 * (c["tile"] // plan["gx"])
        if got.ndim == 2 and not np.array_equal(got[y0:y0 + 16, x0:x0 + 16], want[y0:y0 + 16, x0:x0 + 16]) or got.ndim == 1 and got[c["tile"]] != want[c["tile"]]:
            return f"{what}: first wrong in case {c['name']} ({sorted(k for k, o in bc.REQUIRED.items() if o == c['name'])})"
    return f"{what}: wrong outside the case tiles"


def _colour_forward(w):
    from gpu_helpers import hip_forward
    return hip_forward(w["raw"], w["cam"], export=("n_contrib", "max_contrib", "ranges", "point_list"))


def _check_grads(got, w, kind, what):
    plan = w["plan"]
    P = plan["case"].size
    for k in TENSORS:
        assert not np.asarray(got[k]).reshape(P, -1)[w["never"]].any(), f"{what} {k}: a row no pixel blended is not exact zeros"
    bad, ratio = bc.judge(got, w[kind + "32"], w[kind + "64"], plan, TENSORS, bc.FACTOR, rw.FLOOR)
    _report(what, ratio)
    assert not bad, "\n".join([what] + bad)


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("which", list(bc.SCENES))
def test_forward_on_designed_cases(oracle32, oracle64, which, strict):
    from gpu_helpers import npy
    w = _world(which, oracle32, oracle64)
    plan, f64 = w["plan"], w["f64"]
    mode = "strict" if strict else "fast"
    with _mode(strict):
        f = _colour_forward(w)
        fd = fwd_depth(w["raw"], w["cam"])
    d = f["dbg"]
    ranges, plist = npy(d["ranges"]).astype(np.int64).reshape(-1, 2), npy(d["point_list"]).astype(np.int64).reshape(-1)
    for c in plan["cases"]:
        r0, r1 = ranges[c["tile"]]
        assert np.array_equal(plist[r0:r1], w["lists"][c["name"]]), f"{which} {mode}: the list of case {c['name']} is not the designed one"
    assert f["R"] == f64["num_rendered"]
    np.testing.assert_array_equal(ranges, f64["bins"]["ranges"].astype(np.int64))
    np.testing.assert_array_equal(plist[:f["R"]], f64["bins"]["point_list"].astype(np.int64))
    nc, mc = npy(d["n_contrib"]).astype(np.int64), npy(d["max_contrib"]).astype(np.int64)
    assert np.array_equal(nc, f64["n_contrib"]), _first_bad_case(plan, nc, f64["n_contrib"].astype(np.int64), f"{which} {mode} n_contrib")
    assert np.array_equal(mc, f64["max_contrib"]), _first_bad_case(plan, mc, f64["max_contrib"].astype(np.int64), f"{which} {mode} max_contrib")
    for k in ("color", "final_T"):
        np.testing.assert_array_equal(npy(f[k]), npy(fd[k]), err_msg=f"{k}: depth forward against colour forward")
    bad, ratio = [], {}
    for name, got, r32, r64 in (("color", npy(f["color"]), w["f32"]["color"], f64["color"]), ("final_T", npy(f["final_T"]), w["f32"]["final_T"], f64["final_T"]),
                                ("depth", npy(fd["depth"]), w["depth32"], w["depth64"])):
        b, r = _image_ratios(got, r32, r64, plan, name)
        bad += b
        ratio.update(r)
    _report(f"{which} {mode} forward", ratio)
    assert not bad, "\n".join([f"{which} {mode}"] + bad)


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("which", list(bc.SCENES))
def test_backward_on_designed_cases(oracle32, oracle64, which, strict):
    """strict: render_bwd_scan_kernel<false> and <true>; fast: the pipeline kernel"""
    from gpu_helpers import hip_backward
    w = _world(which, oracle32, oracle64)
    mode = "strict" if strict else "fast"
    with _mode(strict):
        g_col = hip_backward(_colour_forward(w), w["dL"])
        g_dep = bwd(fwd_depth(w["raw"], w["cam"]), w["dL"], w["gD"])
    _check_grads(g_col, w, "gc", f"{which} {mode} colour")
    _check_grads(g_dep, w, "gd", f"{which} {mode} depth")


@pytest.mark.parametrize("which", list(bc.SCENES))
def test_strict_backward_behind_a_fast_forward(oracle32, oracle64, which):
    """no decision masks recorded: the strict backward falls back to the pipeline kernel, which must give the fast backward's bits"""
    from gpu_helpers import hip_backward
    w = _world(which, oracle32, oracle64)
    with _mode(False):
        f, fd = _colour_forward(w), fwd_depth(w["raw"], w["cam"])
        fast = hip_backward(f, w["dL"]), bwd(fd, w["dL"], w["gD"])
    with _mode(True):
        fall = hip_backward(f, w["dL"]), bwd(fd, w["dL"], w["gD"])
    for a, b, kind in zip(fast, fall, ("colour", "depth")):
        assert any(np.abs(v).max() > 0 for v in a.values())
        for k in a:
            assert np.array_equal(a[k], b[k]), f"{which} {kind} {k}: the fallback differs from the fast backward"
    _check_grads(fall[0], w, "gc", f"{which} fallback colour")
    _check_grads(fall[1], w, "gd", f"{which} fallback depth")
