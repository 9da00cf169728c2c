"""-m gpu: the forward's front end (csrc/preprocess.hip: preprocess_kernel, keybuild_kernel, finalize_ranges_kernel; the tile grouping by radix
sort or by csrc/tile_bin.hip; the scans) on the designed scenes of tests/footprint_cases.py — rectangles of exactly 16 | 17, 80 | 81 and
144 | 145 tiles at lanes 0, 31, 32 and 63, waves of exactly 1024 | 1025 instances, SH row blocks with one visible row at every alignment of the
float4 staging, the culls on their exact values, the border clamps and the get_rect tie (tests/test_footprint_cases_cpu.py proves on the CPU
that the scenes reach these edges and that the wrong rule would show at each).  The bars are tests/test_parity_gpu.py's: radii,
tiles_touched, R, sorted keys, point list and ranges exact against the CPU oracle, means2D / depths / conic_opacity exact on visible rows,
rgb within 1e-6, the image within TOL up to threshold flips.  Everything else is bit-equality between two runs that must agree by
construction: both binning modes, a row alone in its block against the same row among visible neighbours, M = 15 at a lower active degree
against the truncated coefficients, the raw-parameter path, the capacity forward, a repeat."""
import numpy as np
import pytest
import torch

import footprint_cases as fc
from conftest import assert_close_flips, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4
EXPORT = ("tiles_touched", "means2D", "depths", "conic_opacity", "rgb", "sorted_keys", "point_list", "ranges")


@pytest.fixture
def binning_mode():
    from gaussian_lic_amd import _lib
    old = _lib.set_binning_mode("auto")
    yield _lib.set_binning_mode
    _lib.set_binning_mode(old)


_refs = {}
COUNT = dict(forwards=0, visible=0, rgb=0.0)     # what _check has seen so far (printed, never asserted)


def _report(what, ref=None):
    r = "" if ref is None else " P = %d, R = %d, longest list = %d;" % (
        ref["pre"]["radii"].size, ref["num_rendered"], int(np.diff(ref["bins"]["ranges"].astype(np.int64), axis=1).max()))
    print(f"{what}:{r} so far {COUNT['forwards']} forwards checked, {COUNT['visible']} visible rows, largest rgb rel err {COUNT['rgb']:.2e}")


def _ref(key, build, oracle):
    """(scene, the oracle's forward): computed once per scene, never modified"""
    if key not in _refs:
        s = build()
        _refs[key] = (s, oracle.forward(s["sc"], s["camd"]))
    return _refs[key]


def _forward(s):
    from gpu_helpers import hip_forward
    return hip_forward(s["raw"], s["cam"], export=EXPORT, act=s["act"])


def _check(f, ref, what, image=True):
    """test_parity_gpu.py's bars on one forward"""
    from gpu_helpers import npy
    d, pre, bins = f["dbg"], ref["pre"], ref["bins"]
    np.testing.assert_array_equal(npy(f["radii"]), pre["radii"], err_msg=what)
    np.testing.assert_array_equal(npy(d["tiles_touched"]).astype(np.uint32), pre["tiles_touched"], err_msg=what)
    assert f["R"] == ref["num_rendered"], what
    np.testing.assert_array_equal(npy(d["sorted_keys"]).view(np.uint64).reshape(-1), bins["keys"], err_msg=what)
    np.testing.assert_array_equal(npy(d["point_list"]).astype(np.uint32).reshape(-1), bins["point_list"], err_msg=what)
    np.testing.assert_array_equal(npy(d["ranges"]).astype(np.uint32).reshape(-1, 2), bins["ranges"], err_msg=what)
    vis = pre["radii"] > 0
    np.testing.assert_array_equal(npy(d["means2D"])[vis], pre["means2D"][vis], err_msg=what)
    np.testing.assert_array_equal(npy(d["depths"])[vis], pre["depths"][vis], err_msg=what)
    np.testing.assert_array_equal(npy(d["conic_opacity"])[vis], pre["conic_opacity"][vis], err_msg=what)
    e_rgb = rel_err(npy(d["rgb"])[vis], pre["rgb"][vis])
    COUNT["forwards"] += 1; COUNT["visible"] += int(vis.sum()); COUNT["rgb"] = max(COUNT["rgb"], e_rgb)
    assert e_rgb < 1e-6, what
    r = bins["ranges"].astype(np.int64)
    assert f["B"] == int(((r[:, 1] - r[:, 0] + 63) // 64).sum()), what
    if image:
        assert_close_flips(npy(f["color"]), ref["color"], tol=TOL, what=what + " color")
        assert_close_flips(npy(f["final_T"]), ref["final_T"], tol=TOL, what=what + " final_T")


def _same_forward(a, b, what):
    """two forwards that must agree on bits: the image and every exported array"""
    assert a["R"] == b["R"] and a["B"] == b["B"], what
    for k in ("color", "final_T", "radii"):
        assert torch.equal(a[k], b[k]), (what, k)
    for k in a["dbg"]:
        x, y = a["dbg"][k], b["dbg"][k]
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), (what, k)


SCENES = [("strip", None), ("waves", None), ("border", None), ("culls", None)] + [("row_counts", P) for P in fc.ROW_COUNTS]


@pytest.mark.parametrize("name,P", SCENES)
def test_oracle_parity_in_both_binning_modes(oracle32, binning_mode, name, P):
    """every designed scene against the oracle under both groupings; the two give the same image on bits, and so does a repeat"""
    from gaussian_lic_amd import _lib
    s, ref = _ref((name, P), (lambda: fc.scene(name)) if P is None else (lambda: fc.row_counts(P)), oracle32)
    got = {}
    for mode in ("radix", "atomic"):
        binning_mode(mode)
        got[mode] = _forward(s)
        assert _lib.binning_path()[0] == mode, (_lib.binning_path(), mode)
        _check(got[mode], ref, f"{name} {P} {mode}")
        _same_forward(got[mode], _forward(s), f"{name} {P} {mode} repeated")
    _same_forward(got["radix"], got["atomic"], f"{name} {P} radix against atomic")
    _report(f"{name} {P}", ref)


def _sh_grid(oracle, combos):
    """D x M x P x pattern: the oracle's bars on every scene (under the binning mode in force), and a row that is alone in its block
    (single-r) has the rgb of the same row among visible neighbours (all) on bits — same kernel, same arithmetic, another staging."""
    from gpu_helpers import npy
    for D, M in combos:
        for P in fc.SH_P:
            rgb_all = None
            for pattern in fc.SH_PATTERNS:
                s, ref = _ref(("sh", D, M, P, pattern), lambda: fc.sh_blocks(D, M, P, pattern), oracle)
                what = f"sh_blocks D={D} M={M} P={P} {pattern}"
                f = _forward(s)
                _check(f, ref, what)
                _same_forward(f, _forward(s), what + " repeated")
                rgb = npy(f["dbg"]["rgb"]).view(np.uint32)
                vis = ref["pre"]["radii"] > 0
                if pattern == "all":
                    rgb_all = rgb
                    assert vis.all(), what
                else:
                    np.testing.assert_array_equal(rgb[vis], rgb_all[vis], err_msg=what + ": rgb against the all-visible run")
        _report(f"sh_blocks D={D} M={M}")


@pytest.mark.parametrize("D,M", fc.SH_LDS)
def test_sh_blocks_through_lds(oracle32, D, M):
    _sh_grid(oracle32, [(D, M)])


@pytest.mark.parametrize("mode", ["radix", "atomic"])
def test_sh_blocks_other_binning_and_plain_kernel(oracle32, binning_mode, mode):
    """the 256-thread kernel's (D, M), and one LDS degree once more, under a forced grouping"""
    binning_mode(mode)
    _sh_grid(oracle32, fc.SH_PLAIN + (fc.SH_LDS[-1 if mode == "radix" else 0],))


@pytest.mark.parametrize("pattern", ["all", "alternate", "single-33"])
def test_active_degree_below_the_stored_one(oracle32, pattern):
    """M = 15 with D = 0, 1, 2 (every training run while the degree ramps): image and rgb of the truncated coefficient rows, on bits.
    D = 0 leaves the LDS kernel for the 256-thread one with a row stride of 45 floats."""
    P = 173
    for D in (0, 1, 2):
        M = (D + 1) ** 2 - 1
        full, ref = _ref(("sh", D, 15, P, pattern), lambda: fc.sh_blocks(D, 15, P, pattern), oracle32)
        cut, ref_cut = _ref(("sh", D, M, P, pattern), lambda: fc.sh_blocks(D, M, P, pattern), oracle32)
        assert full["act"]["shs"].shape[1] == 15 and cut["act"]["shs"].shape[1] == M
        np.testing.assert_array_equal(ref["pre"]["rgb"], ref_cut["pre"]["rgb"])           # (the oracle agrees that nothing else is read)
        a, b = _forward(full), _forward(cut)
        _check(a, ref, f"D={D} M=15 {pattern}")
        _same_forward(a, b, f"D={D}: M=15 against M={M}, {pattern}")


def test_clamped_channels_get_no_colour_gradient(oracle32):
    """the clamp bits travel in the record's spare word beside the seqmask: dL_ddc and dL_dsh are exactly zero on every channel the oracle
    marks as clamped, and non-zero on an unmarked channel of the same row wherever the oracle's own gradient is"""
    from gaussian_lic_amd.synthetic import pixel_grad
    from gpu_helpers import hip_backward
    for D, M, pattern in ((3, 15, "all"), (2, 15, "alternate"), (1, 3, "all")):
        s, ref = _ref(("sh", D, M, 173, pattern), lambda: fc.sh_blocks(D, M, 173, pattern), oracle32)
        f = _forward(s)
        _check(f, ref, f"clamp D={D} M={M}")
        dL = pixel_grad(fc.SH_H, fc.SH_W, seed=3)
        g = hip_backward(f, dL)
        gref = oracle32.backward(s["sc"], s["camd"], ref, dL.numpy())
        c = ref["pre"]["clamped"].astype(bool)                       # [P, 3]
        vis = ref["pre"]["radii"] > 0
        assert c[vis].any() and (~c[vis]).any()
        ddc, dsh = g["dL_ddc"].reshape(-1, 3), g["dL_dsh"].reshape(-1, M, 3)
        assert (ddc[c] == 0).all() and (np.abs(dsh).max(1)[c] == 0).all()
        nterms = (D + 1) ** 2 - 1
        live = ~c & (gref["dL_ddc"].reshape(-1, 3) != 0)
        assert live[c.any(1)].any(), "no row has both a clamped channel and a live one"
        assert (ddc[live] != 0).all() and (np.abs(dsh[:, :nterms]).max(1)[live] != 0).all()
        assert rel_err(ddc, gref["dL_ddc"].reshape(-1, 3)) < TOL and rel_err(dsh, gref["dL_dsh"].reshape(-1, M, 3)) < TOL
        assert (ddc[~vis] == 0).all() and (dsh[~vis] == 0).all()


@pytest.mark.parametrize("name", ["strip", "border"])
def test_raw_parameter_path(oracle32, name):
    """activations inside the kernel (a.raw): the lists of the activated path.  The kernel's expf / sigmoid may differ from the host's by an
    ulp; a row whose tiles change through that is COUNTED, against the oracle run on the values the raw path itself exported — none may."""
    from gaussian_lic_amd import trainer
    from gpu_helpers import export_lists, gpu, npy, raw_forward
    s, ref = _ref((name, None), lambda: fc.scene(name), oracle32)
    m = trainer.GaussianModel({k: (v.clone() if torch.is_tensor(v) else v) for k, v in s["raw"].items()}, gpu())
    cam = s["cam"].to_device(gpu())
    fwd = raw_forward(m, cam)
    d = export_lists(m, cam, fwd, ("tiles_touched", "conic_opacity", "point_list", "ranges"))
    R, B, radii = fwd.state[0], fwd.state[1], fwd.state[2]
    tt = npy(d["tiles_touched"]).astype(np.uint32)
    flipped = np.nonzero((tt != ref["pre"]["tiles_touched"]) | (npy(radii) != ref["pre"]["radii"]))[0]
    if flipped.size:
        # the oracle on the raw path's own opacity (exported) and the host's scales: which rows does it move?
        sc = dict(s["sc"])
        vis = npy(radii) > 0
        sc["opac"] = np.where(vis[:, None], npy(d["conic_opacity"])[:, 3:4], s["sc"]["opac"])
        own = oracle32.preprocess(sc, s["camd"])
        explained = np.nonzero(own["tiles_touched"] != ref["pre"]["tiles_touched"])[0]
        print(f"{name}: raw path differs on rows {flipped.tolist()}; the oracle on its exported opacity moves rows {explained.tolist()}")
    assert flipped.size == 0, f"{flipped.size} rows of {name} change their tiles on the raw-parameter path: {flipped.tolist()}"
    assert R == ref["num_rendered"]
    np.testing.assert_array_equal(npy(d["ranges"]).astype(np.uint32).reshape(-1, 2), ref["bins"]["ranges"])
    np.testing.assert_array_equal(npy(d["point_list"]).astype(np.uint32).reshape(-1), ref["bins"]["point_list"])
    act = _forward(s)
    assert (R, B) == (act["R"], act["B"])
    np.testing.assert_array_equal(npy(d["point_list"]), npy(act["dbg"]["point_list"]))
    np.testing.assert_array_equal(npy(d["ranges"]), npy(act["dbg"]["ranges"]))


@pytest.mark.parametrize("name", ["waves", "strip"])
def test_capacity_forward_sized_exactly(oracle32, name):
    """caller-owned buffers of exactly (R, B): status (R, B, 0, 1); image and radii of the callback path on bits"""
    from gaussian_lic_amd import rasterizer as rz
    s, ref = _ref((name, None), lambda: fc.scene(name), oracle32)
    dev = torch.device("cuda:0")
    base = _forward(s)
    _check(base, ref, name)
    act, cam = base["act"], s["cam"]
    vm, pm, cp = (torch.from_numpy(a).to(dev) for a in (cam.world_view_transform, cam.full_proj_transform, cam.camera_center))
    scal = (float(cam.tanfovx), float(cam.tanfovy), float(cam.limx_neg), float(cam.limx_pos), float(cam.limy_neg), float(cam.limy_pos))
    bufs = rz.CapacityBuffers(act["means"].shape[0], cam.image_width, cam.image_height, base["R"], base["B"], dev)
    out = rz.rasterize_gaussians_capacity(bufs, torch.zeros(3, device=dev), act["means"].contiguous(), act["opac"].contiguous(), act["scales"].contiguous(),
                                          act["rots"].contiguous(), 1.0, vm, pm, *scal, act["dc"].contiguous(), act["shs"].contiguous(), act["D"], cp)
    cR, cB, color, final_T, radii = out[:5]
    assert bufs.read_status() == (ref["num_rendered"], base["B"], 0, 1)
    assert (cR, cB) == (base["R"], base["B"])
    assert torch.equal(color, base["color"]) and torch.equal(final_T, base["final_T"]) and torch.equal(radii, base["radii"])
