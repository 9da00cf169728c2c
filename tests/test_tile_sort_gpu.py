"""-m gpu: the per-tile depth sort (csrc/radix_sort.hip) on the designed lists of tests/tile_lists.py — every list length at which the sort
changes its path (the early exits of 0, 1 and 2 instances; one wave up to 1024 with 1..16 elements per lane and partly empty last lanes; the
workgroup kernel in LDS up to 4096; global scratch beyond), every tie structure (none; 1, 8 and 9 isolated pairs; a run of 9 and of 10 at a
lane boundary, the head and the tail; one single run) and the key ranges that end the nibble passes early, need all eight, or make the long
body skip uniform byte passes.  Each scene goes through both binning paths (radix: rows in row order, no second key; atomic: rows in arrival
order, second key) and through both again as a PERMUTED map with tie_rank (the second key through a gather) — reversed, which turns every
tie into descending order of the second key, and randomly permuted.  The lists must be the reference's, which for these inputs is a plain
numpy statement: per tile, ascending (depth bits, original index).  The shipped build sorts in one pair buffer (GS_LSORT_SINGLE = 1), correct
only through the ordering of a wave's LDS accesses: there is one right list, and it is compared against here."""
import numpy as np
import pytest
import torch

import tile_lists as tl
from conftest import assert_close_flips

pytestmark = pytest.mark.gpu

# (binning mode, permutation of the map's rows)
MODES = [("radix", None), ("atomic", None), ("radix", "reversed"), ("atomic", "reversed"), ("radix", "random"), ("atomic", "random")]


@pytest.fixture
def binning_mode():
    from gaussian_lic_amd import _lib
    old = _lib.set_binning_mode("auto")
    yield _lib.set_binning_mode
    _lib.set_binning_mode(old)


_scenes = {}


def _scene(pattern, oracle):
    """(raw, camera, plan, the oracle's forward): built once per pattern, never modified"""
    if pattern not in _scenes:
        raw, sc, camd, cam, plan = tl.scene(pattern)
        _scenes[pattern] = (raw, cam, plan, oracle.forward(sc, camd))
    return _scenes[pattern]


def _forward(raw, cam, plan, mode, permutation, set_mode):
    """One HIP forward.  Returns (forward, lists in ORIGINAL rows, lists in storage rows, storage-order expectation)."""
    from gaussian_lic_amd import _lib
    from gaussian_lic_amd.synthetic import activate
    from gpu_helpers import hip_forward, npy
    P = plan["tile"].size
    act, perm, tie = activate(raw), None, None
    if permutation is not None:
        perm = np.arange(P)[::-1].copy() if permutation == "reversed" else np.random.default_rng(17).permutation(P)   # storage row s = original row perm[s]
        tperm = torch.from_numpy(perm)
        act = {k: (v[tperm].contiguous() if torch.is_tensor(v) else v) for k, v in act.items()}
        tie = tperm.to(torch.int32).to("cuda:0")
    set_mode(mode)
    f = hip_forward(raw, cam, export=("sorted_keys", "point_list", "ranges"), tie_rank=tie, act=act)
    assert _lib.binning_path()[0] == mode, (_lib.binning_path(), mode, permutation)
    d = f["dbg"]
    stored = dict(R=int(f["R"]), ranges=npy(d["ranges"]).astype(np.uint32).reshape(-1, 2), keys=npy(d["sorted_keys"]).view(np.uint64).reshape(-1),
                  point_list=npy(d["point_list"]).astype(np.uint32).reshape(-1))
    original = dict(stored, point_list=stored["point_list"] if perm is None else perm[stored["point_list"]].astype(np.uint32))
    exp = tl.expected_lists(plan["tile"] if perm is None else plan["tile"][perm], plan["key"] if perm is None else plan["key"][perm], plan["T"],
                            tie_rank=perm)
    return f, original, stored, exp


def _first_bad_tile(plan, got, want):
    """the designed case of the first tile whose list differs (for the failure message)"""
    bad = np.nonzero(got != want)[0]
    if bad.size == 0:
        return None
    t = int(plan["tile"][want[bad[0]]])
    c = next(c for c in plan["cases"] if c["tile"] == t)
    return f"first wrong list: tile {t}, n = {c['n']}, {c['pattern']} {c['where']} ({c['pairs']} equal neighbours), {bad.size} entries differ in all"


@pytest.mark.parametrize("pattern", tl.PATTERNS)
def test_designed_lists_on_every_path(oracle32, binning_mode, pattern):
    from gpu_helpers import npy
    raw, cam, plan, ref = _scene(pattern, oracle32)
    bins = ref["bins"]
    base = tl.expected_lists(plan["tile"], plan["key"], plan["T"])
    np.testing.assert_array_equal(bins["point_list"], base["point_list"])       # (the two references agree: tests/test_tile_lists_cpu.py)
    images = {}
    for mode, permutation in MODES:
        what = f"{pattern} {mode} {permutation}"
        f, original, stored, exp = _forward(raw, cam, plan, mode, permutation, binning_mode)
        assert original["R"] == ref["num_rendered"] == exp["R"], what
        for got, want in ((original, dict(ranges=bins["ranges"], keys=bins["keys"], point_list=bins["point_list"])), (stored, exp)):
            np.testing.assert_array_equal(got["ranges"], want["ranges"], err_msg=what)
            np.testing.assert_array_equal(got["keys"], want["keys"], err_msg=what)
        assert np.array_equal(original["point_list"], bins["point_list"]), (what, _first_bad_tile(plan, original["point_list"], bins["point_list"]))
        assert np.array_equal(stored["point_list"], exp["point_list"]), what
        images[(mode, permutation)] = (npy(f["color"]), npy(f["final_T"]))
    first = images[MODES[0]]
    for k, v in images.items():
        assert np.array_equal(v[0], first[0]) and np.array_equal(v[1], first[1]), (pattern, k)
    assert_close_flips(first[0], ref["color"], what=pattern + " color")
    assert_close_flips(first[1], ref["final_T"], what=pattern + " final_T")


def test_backward_is_the_same_on_both_paths(oracle32, binning_mode):
    """eight tied pairs per tile (the insertion path at its pair limit): every gradient bit-identical between the two groupings"""
    from gaussian_lic_amd.synthetic import pixel_grad
    from gpu_helpers import hip_backward
    raw, cam, plan, ref = _scene("pairs-8", oracle32)
    dL = pixel_grad(cam.image_height, cam.image_width, seed=2)
    g = {}
    for mode in ("radix", "atomic"):
        f, original, _, _ = _forward(raw, cam, plan, mode, None, binning_mode)
        assert np.array_equal(original["point_list"], ref["bins"]["point_list"]), mode
        g[mode] = hip_backward(f, dL)
    assert any(np.abs(v).max() > 0 for v in g["radix"].values())
    for k in g["radix"]:
        assert np.array_equal(g["radix"][k], g["atomic"][k]), k
