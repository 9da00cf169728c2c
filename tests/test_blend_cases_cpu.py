"""The designed blend scenes of tests/blend_cases.py ARE what they were designed to be, proven on the CPU oracle alone: the float64
restatement of the decisions agrees with oracle64.forward, every structural cell of REQUIRED is reached by the case that owns it, every
(pixel, entry) pair keeps the cut margins (so two correct float32 blends cannot decide differently and no comparison on these scenes needs a
flip allowance), the cases do not reach each other, and the comparator of the GPU suite passes the fp32 oracle and fails every structural
mutant of the restated backward on the case that owns the mutated edge."""
import numpy as np
import pytest

import blend_cases as bc
import rowwise as rw

from blend_cases import FACTOR     # the GPU suite's factor (profiles/blend_cases_factors.txt): the mutants must fail at it, and at the cap

TENSORS = ("dL_dmean2D", "dL_dconic", "dL_dopacity", "dL_dcolor")
FWD_RTOL = 1e-12        # restatement against oracle64, final_T and colour: the bound the issue sets
# Restated backward against oracle64, relative to a tensor's max-abs.  Both are float64 and differ in association only: a Gaussian's sum has at
# most 9 tiles x 256 pixels terms, each carries the colour-behind term scaled by 1 / (1 - alpha) <= 1 / (1 - ALPHA_MAX) = 100, each rounding is
# 2^-53 relative; twice that product (the T products and the A sums each add their own chain).  5.1e-11.
BWD_RTOL = 2 * (9 * 256) * (1.0 / (1.0 - bc.ALPHA_MAX)) * 2.0 ** -53
# "Not constant" colours, made useful: every channel's spread across a case must stand three orders above what the comparator lets pass
# (FACTOR x rowwise.FLOOR of the case's scale), so that entries taking each other's colour cannot hide inside the tolerance.
MIN_COLOUR_SPREAD = 1000 * FACTOR * rw.FLOOR
# The issue's "P in the low thousands, a forward plus a backward well under a second": at most 3000, about twice the larger scene's 1404 (measured on the
# MI355X: every forward / backward test of these scenes at 0.6 s or less, profiles/blend_cases_factors.txt).
MAX_P = 3000


@pytest.fixture(scope="module")
def world(oracle32, oracle64):
    cache = {}

    def get(which):
        if which not in cache:
            raw, sc, camd, cam, plan = bc.build(which)
            f64, f32 = oracle64.forward(sc, camd), oracle32.forward(sc, camd)
            dL, _ = bc.pixel_grads(plan["W"], plan["H"])
            g64 = bc.oracle_blend_grads(oracle64.backward(sc, camd, f64, dL))
            g32 = bc.oracle_blend_grads(oracle32.backward(sc, camd, f32, dL))
            cache[which] = dict(sc=sc, camd=camd, plan=plan, f64=f64, f32=f32, dL=dL, g64=g64, g32=g32,
                                dec=bc.decisions(sc, camd, f64["pre"], f64["bins"], plan))
        return cache[which]
    return get


@pytest.mark.parametrize("which", list(bc.SCENES))
def test_restatement_agrees_with_the_oracle(world, which):
    w = world(which)
    plan, f64, dec = w["plan"], w["f64"], w["dec"]
    W, H = plan["W"], plan["H"]
    lists = bc.expected_case_lists(plan)
    assert len({c["name"] for c in plan["cases"]}) == len(plan["cases"])
    for c in plan["cases"]:
        d = dec[c["name"]]
        assert d["n"] == c["n"], c
        np.testing.assert_array_equal(d["rows"], lists[c["name"]], err_msg=c["name"])
        for f in (f64, w["f32"]):     # both oracles hold the designed lists
            r0, r1 = f["bins"]["ranges"][c["tile"]]
            np.testing.assert_array_equal(f["bins"]["point_list"][r0:r1], lists[c["name"]], err_msg=c["name"])
        ok = d["inimg"]
        py, px = (d["ty0"] + bc.LY)[ok], (d["tx0"] + bc.LX)[ok]
        np.testing.assert_array_equal(f64["n_contrib"][py, px], d["n_contrib"][ok], err_msg=c["name"])
        assert f64["max_contrib"][c["tile"]] == d["max_contrib"], c
        np.testing.assert_allclose(d["final_T"][ok], f64["final_T"][py, px], rtol=FWD_RTOL, atol=0, err_msg=c["name"])
        col = bc.blend_image(d, f64["pre"]["rgb"][d["rows"]])
        np.testing.assert_allclose(col[ok], f64["color"][:, py, px].T, rtol=FWD_RTOL, atol=1e-300, err_msg=c["name"])
        assert np.ptp(f64["pre"]["rgb"][d["rows"]], axis=0).min() > MIN_COLOUR_SPREAD or d["n"] == 1, c     # the colours are not constant across a case
    # the fp32 oracle takes the same decisions
    np.testing.assert_array_equal(w["f32"]["n_contrib"], f64["n_contrib"])
    np.testing.assert_array_equal(w["f32"]["max_contrib"], f64["max_contrib"])


def test_every_required_cell_is_reached(world):
    cov = {}
    for which in bc.SCENES:
        for cell, names in bc.coverage(world(which)["dec"]).items():
            cov.setdefault(cell, set()).update(names)
    missing = {cell: owner for cell, owner in bc.REQUIRED.items() if owner not in cov.get(cell, ())}
    assert not missing, f"cells not reached by their case: {missing}"
    # the ragged cells on the ragged scene, by the tiles the image cuts
    rag = bc.coverage(world("ragged")["dec"])
    for k in ("x", "y", "corner"):
        assert f"ragged-{k}" in rag[f"ragged-{k}"] and f"ragged-{k}" in rag[f"ragged-{k}-mean-outside"]
    assert bc.SCENES["ragged"][0] % 16 and bc.SCENES["ragged"][1] % 16


@pytest.mark.parametrize("which", list(bc.SCENES))
def test_cut_margins_isolation_and_bucket_count(world, which):
    w = world(which)
    bc.cut_margins(w["dec"])
    assert bc.isolation(w["f64"]["pre"], w["plan"]) < 1.0 - bc.MARGIN
    r = w["f64"]["bins"]["ranges"].astype(np.int64)
    B = int(((r[:, 1] - r[:, 0] + bc.BUCKET - 1) // bc.BUCKET).sum())
    assert B % 128 != 0, B
    assert w["plan"]["case"].size <= MAX_P


@pytest.mark.parametrize("which", list(bc.SCENES))
def test_restated_backward_is_the_oracle_s(world, which):
    w = world(which)
    got = bc.backward(w["f64"]["pre"], w["f64"]["bins"], w["plan"], w["dL"])
    for k in TENSORS:
        scale = np.abs(w["g64"][k]).max()
        assert np.abs(got[k] - w["g64"][k]).max() <= BWD_RTOL * scale, k
    never = bc.never_blended_rows(w["f64"]["pre"], w["f64"]["bins"], w["plan"])
    assert never.any()
    for k in TENSORS:
        assert not np.asarray(w["g64"][k]).reshape(never.size, -1)[never].any(), k


@pytest.mark.parametrize("factor", [FACTOR, rw.MAX_FACTOR])
def test_comparator_passes_the_fp32_oracle_and_fails_every_mutant(world, factor):
    assert FACTOR <= rw.MAX_FACTOR
    for which in bc.SCENES:
        w = world(which)
        bad, _ = bc.judge(w["g32"], w["g32"], w["g64"], w["plan"], TENSORS, factor, rw.FLOOR)
        assert not bad, bad
        good = bc.backward(w["f64"]["pre"], w["f64"]["bins"], w["plan"], w["dL"])
        bad, _ = bc.judge(good, w["g32"], w["g64"], w["plan"], TENSORS, factor, rw.FLOOR)
        assert not bad, bad
    for mutant, owner in bc.MUTANTS.items():
        which = "ragged" if owner.startswith("ragged") else "exact"
        w = world(which)
        tile = next(c["tile"] for c in w["plan"]["cases"] if c["name"] == owner)
        rows = w["plan"]["case"] == [c["name"] for c in w["plan"]["cases"]].index(owner)
        # the owner's Gaussians gather gradient from its tile and the tiles around it
        gx = w["plan"]["gx"]
        around = [t for t in range(w["plan"]["T"]) if abs(t % gx - tile % gx) <= 1 and abs(t // gx - tile // gx) <= 1
                  and w["f64"]["bins"]["ranges"][t, 1] > w["f64"]["bins"]["ranges"][t, 0]]
        got = bc.backward(w["f64"]["pre"], w["f64"]["bins"], w["plan"], w["dL"], tiles=around, mutant=mutant)
        got = {k: np.where(rows.reshape(-1, *[1] * (got[k].ndim - 1)), got[k], w["g64"][k]) for k in TENSORS}
        bad, _ = bc.judge(got, w["g32"], w["g64"], w["plan"], TENSORS, factor, rw.FLOOR)
        assert any(f"case {owner} " in b for b in bad), (mutant, owner, bad)
