"""-m gpu: depth rendering (gslic_rasterize_forward_depth / gslic_rasterize_backward_depth, render(return_depth=True)).

depth = sum T alpha z over the colour's contributors.  The oracle renders it as a colour: its render_forward / render_backward take the
per-Gaussian colour as an argument, so rgb := [z, 0, 0] makes channel 0 the expected depth image and, in the backward, dL := [g_D, 0, 0]
gives the depth's share of the 2D gradients and dL/dz = dL_dcolor[:, 0]."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import assert_close_flips, make_scene, rel_err
from gpu_helpers import gpu

pytestmark = pytest.mark.gpu

TOL = 1e-4
DEPTH_CASES = [
    ("random", 3000, 70, 50, 2, 5),        # ragged image (not a multiple of 16), deg 2
    ("random", 125000, 480, 270, 3, 7),    # 1/16 of config 3 (dense tiles, long lists)
    ("lidar", 30000, 640, 480, 3, 0),
]
# a general SE(3) pose (scene moved rigidly into its frame): the view matrix's row 2 (V[2], V[6], V[10]) differs from its column 2
# (V[8], V[9], V[10]) and V[2], V[6] are non-zero, so a transposed or mis-indexed view-row chain cannot pass
POSE = dict(ypr=(25.0, -12.0, 8.0), t=(0.4, -0.3, 0.6), place=True)
GRADS = ("dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmean3D", "dL_dcov3D", "dL_ddc", "dL_dsh", "dL_dscale", "dL_drot")


class _mode:
    """gslic_set_math_mode for the duration of a block (strict = the default)."""

    def __init__(self, strict):
        self.strict = strict

    def __enter__(self):
        from gaussian_lic_amd import _lib
        self.prev = _lib.set_math_mode(self.strict)

    def __exit__(self, *a):
        from gaussian_lic_amd import _lib
        _lib.set_math_mode(self.prev)


def _inputs(raw, cam, raw_params=False):
    from gpu_helpers import settings_from
    from gaussian_lic_amd.synthetic import activate
    dev = gpu()
    act = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in activate(raw).items()}
    rs = settings_from(cam, act["D"], dev)
    if raw_params:
        src = dict(means=raw["xyz"].to(dev), opac=raw["opacity"].to(dev), scales=raw["scaling"].to(dev), rots=raw["rotation"].to(dev),
                   dc=act["dc"], shs=act["shs"], D=act["D"])
    else:
        src = act
    return src, rs


def fwd_depth(raw, cam, raw_params=False):
    from gaussian_lic_amd import rasterizer as rz
    t, rs = _inputs(raw, cam, raw_params)
    out = rz.rasterize_gaussians_depth(rs.bg, t["means"], t["opac"], t["scales"], t["rots"], rs.scale_modifier, rs.viewmatrix, rs.projmatrix,
                                      rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, rs.limx_neg, rs.limx_pos, rs.limy_neg, rs.limy_pos,
                                      t["dc"], t["shs"], t["D"], rs.campos, raw_params=raw_params)
    R, B, color, final_T, depth, radii, geom, binning, img, sample = out
    torch.cuda.synchronize()
    return dict(R=R, B=B, color=color, final_T=final_T, depth=depth, radii=radii, bufs=(geom, binning, img, sample), t=t, rs=rs, raw=raw_params)


def fwd_plain(raw, cam, raw_params=False):
    from gaussian_lic_amd import rasterizer as rz
    t, rs = _inputs(raw, cam, raw_params)
    e = torch.empty(0, device=gpu())
    out = rz.rasterize_gaussians(rs.bg, t["means"], e, t["opac"], t["scales"], t["rots"], rs.scale_modifier, e, rs.viewmatrix, rs.projmatrix,
                                 rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, rs.limx_neg, rs.limx_pos, rs.limy_neg, rs.limy_pos,
                                 t["dc"], t["shs"], t["D"], rs.campos, False, False, False, raw_params=raw_params)
    R, B, color, final_T, radii, geom, binning, img, sample = out
    torch.cuda.synchronize()
    return dict(R=R, B=B, color=color, final_T=final_T, radii=radii, bufs=(geom, binning, img, sample), t=t, rs=rs, raw=raw_params)


def bwd(f, dL_dpix, dL_ddepth=None):
    """dL_ddepth None: the colour-only gslic_rasterize_backward on f's buffers; else gslic_rasterize_backward_depth."""
    from gaussian_lic_amd import rasterizer as rz
    t, rs = f["t"], f["rs"]
    dev = gpu()
    geom, binning, img, sample = f["bufs"]
    if dL_ddepth is None:
        e = torch.empty(0, device=dev)
        g = rz.rasterize_gaussians_backward(rs.bg, t["means"], f["radii"], e, t["scales"], t["rots"], rs.scale_modifier, e, rs.viewmatrix,
                                            rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.limx_neg, rs.limx_pos, rs.limy_neg, rs.limy_pos,
                                            dL_dpix.to(dev), t["dc"], t["shs"], t["D"], rs.campos, geom, f["R"], binning, img, f["B"], sample,
                                            0.0, False, raw_params=f["raw"])
    else:
        g = rz.rasterize_gaussians_backward_depth(rs.bg, t["means"], f["radii"], t["scales"], t["rots"], rs.scale_modifier, rs.viewmatrix,
                                                  rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.limx_neg, rs.limx_pos, rs.limy_neg, rs.limy_pos,
                                                  dL_dpix.to(dev), dL_ddepth.to(dev), t["dc"], t["shs"], t["D"], rs.campos, geom, f["R"], binning,
                                                  img, f["B"], sample, raw_params=f["raw"])
    torch.cuda.synchronize()
    return {n: x.cpu().numpy() for n, x in zip(GRADS, g)}


def n_contrib(f):
    from gaussian_lic_amd import rasterizer as rz
    P = f["t"]["means"].shape[0]
    M = f["t"]["shs"].shape[1] if f["t"]["shs"].numel() else 0
    return rz.debug_export(f["rs"], P, M, f["R"], f["B"], *f["bufs"], what=("n_contrib",))["n_contrib"].cpu().numpy()


def oracle_depth(orc, ref, W, H):
    """The oracle's depth image: its blend with rgb := [z, 0, 0] (same alphas, cut-offs and early stop as the colour)."""
    pre = dict(ref["pre"])
    rgb = np.zeros_like(pre["rgb"])
    rgb[:, 0] = pre["depths"]
    pre["rgb"] = rgb
    return orc.render_forward(pre, ref["bins"], W, H)["color"][0], pre


def oracle_backward_depth(orc, sc, camd, ref, dL_dpix, dL_ddepth):
    """Expected nine gradients of gslic_rasterize_backward_depth, composed from the oracle's library functions: the colour pass as
    Oracle.backward runs it, a depth pass (rgb := [z,0,0], final colour := the depth image, dL := [g_D,0,0]), orc_preprocess_backward on the
    summed 2D gradients with the colour pass's dL_dcolor only, then dL/dz * (V[2], V[6], V[10]) on dL_dmean3D and both opacity shares."""
    from oracle.oracle import _ptr
    W, H = camd["W"], camd["H"]
    P = sc["means"].shape[0]
    M = 0 if sc["shs"] is None or sc["shs"].size == 0 else sc["shs"].shape[1]
    pre, bins = ref["pre"], ref["bins"]
    z = lambda *s: np.zeros(s, orc.dtype)

    def render_bwd(pre_, final, dL):
        g = dict(m2=z(P, 3), con=z(P, 4), op=z(P, 1), col=z(P, 3))
        fin, dl = orc.a(final, (3, H, W)), orc.a(dL, (3, H, W))   # (named: the arrays must outlive the call)
        orc.lib.orc_render_backward(ctypes.c_int(W), ctypes.c_int(H), ctypes.c_int(P), _ptr(bins["ranges"]), _ptr(bins["point_list"]),
                                    _ptr(pre_["means2D"]), _ptr(pre_["conic_opacity"]), _ptr(pre_["rgb"]), _ptr(fin),
                                    _ptr(ref["n_contrib"]), _ptr(dl), _ptr(g["m2"]), _ptr(g["con"]), _ptr(g["op"]),
                                    _ptr(g["col"]))
        return g

    gc = render_bwd(pre, ref["color"], dL_dpix)
    depth_img, pre_d = oracle_depth(orc, ref, W, H)
    fin_d = np.zeros((3, H, W), np.float64)
    fin_d[0] = depth_img
    dL_d = np.zeros((3, H, W), np.float64)
    dL_d[0] = dL_ddepth
    gd = render_bwd(pre_d, fin_d, dL_d)
    m2 = orc.a(gc["m2"] + gd["m2"])
    con = orc.a(gc["con"] + gd["con"])
    g = dict(dL_dmean3D=z(P, 3), dL_dcov3D=z(P, 6), dL_ddc=z(P, 1, 3), dL_dsh=z(P, M, 3), dL_dscale=z(P, 3), dL_drot=z(P, 4))
    r = orc.real
    means, scales, rots, dc = orc.a(sc["means"]), orc.a(sc["scales"]), orc.a(sc["rots"]), orc.a(sc["dc"])
    shs = orc.a(sc["shs"]) if M > 0 else None
    view, proj, campos = orc.a(camd["view"]), orc.a(camd["proj"]), orc.a(camd["campos"])
    orc.lib.orc_preprocess_backward(
        ctypes.c_int(P), ctypes.c_int(int(sc["D"])), ctypes.c_int(M), _ptr(means), _ptr(pre["radii"]), _ptr(dc), _ptr(shs), _ptr(pre["clamped"]),
        _ptr(scales), _ptr(rots), r(1.0), _ptr(pre["cov3D"]), _ptr(view), _ptr(proj), ctypes.c_int(W), ctypes.c_int(H), r(camd["tanfovx"]),
        r(camd["tanfovy"]), r(camd["limx_neg"]), r(camd["limx_pos"]), r(camd["limy_neg"]), r(camd["limy_pos"]), _ptr(campos), _ptr(m2),
        _ptr(con), _ptr(gc["col"]), _ptr(g["dL_dmean3D"]), _ptr(g["dL_dcov3D"]), _ptr(g["dL_ddc"]), _ptr(g["dL_dsh"]) if M > 0 else None,
        _ptr(g["dL_dscale"]), _ptr(g["dL_drot"]), r(0.0))
    V = np.asarray(camd["view"], np.float64).reshape(-1)
    dz = gd["col"][:, 0].astype(np.float64)
    g["dL_dmean3D"] = g["dL_dmean3D"] + dz[:, None] * np.array([V[2], V[6], V[10]])[None, :]
    g["dL_dopacity"] = gc["op"].astype(np.float64) + gd["op"]
    g["dL_dmean2D"], g["dL_dconic"], g["dL_dcolor"] = m2, con.reshape(P, 2, 2), gc["col"]
    return g


# ------------------------------------------------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("kind,P,W,H,deg,seed", DEPTH_CASES)
def test_depth_forward_matches_oracle(oracle32, oracle64, strict, kind, P, W, H, deg, seed):
    from gpu_helpers import npy
    raw, sc, camd, cam = make_scene(kind, P, W, H, deg, seed)
    with _mode(strict):
        f = fwd_depth(raw, cam)
    got = npy(f["depth"])
    assert float(np.abs(got).max()) > 0
    for orc in (oracle32, oracle64):
        ref = orc.forward(sc, camd)
        exp, _ = oracle_depth(orc, ref, W, H)
        if strict and orc is oracle32:
            assert rel_err(got, exp) < TOL, (orc.dtype, rel_err(got, exp))
        else:
            # the fast arithmetic, and the double-precision oracle against any fp32 blend, decide a few alpha / transmittance cuts per million
            # pairs the other way (125k case: one pixel 2e-4 from oracle64 in the strict mode): the parity bar of the
            # blend's outputs with its threshold flips
            # A flipped pair moves its pixel by up to alpha T (z_i - depth behind it) ~ z_max / 255, and a dense scene can stack two flips in a pixel
            # (lidar case vs oracle64: 1.2e-2 of max-abs in one pixel, its colour moves with it): the bound is four contributions
            assert_close_flips(got, exp, TOL, what=f"depth {'strict' if strict else 'fast'} vs oracle {np.dtype(orc.dtype).name}",
                               flip_bound=4.0 / 255)
        if orc is oracle32 and strict:
            print(f"\n[{kind} P={P} {W}x{H}] strict depth bit-equal to oracle32 in {int((got == exp).sum())} of {got.size} pixels")


# ----------------------------------------------------------------------------------------------------------------- 2. nothing else moves
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("raw_params", [False, True])
def test_depth_forward_leaves_colour_untouched(strict, raw_params):
    from gpu_helpers import npy
    raw, sc, camd, cam = make_scene("random", 20000, 330, 250, 3, 1)
    with _mode(strict):
        a = fwd_plain(raw, cam, raw_params)
        b = fwd_depth(raw, cam, raw_params)
        na, nb = n_contrib(a), n_contrib(b)
    assert a["R"] == b["R"] and a["B"] == b["B"]
    for k in ("color", "final_T", "radii"):
        np.testing.assert_array_equal(npy(a[k]), npy(b[k]), err_msg=k)
    np.testing.assert_array_equal(na, nb)


# --------------------------------------------------------------------------------------------------------- 3. dL_ddepth = 0 changes nothing
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("raw_params", [False, True])
def test_zero_depth_gradient_and_layout_prefix(strict, raw_params):
    from gaussian_lic_amd.synthetic import pixel_grad
    raw, sc, camd, cam = make_scene("random", 20000, 330, 250, 3, 3)
    W, H = 330, 250
    dL = pixel_grad(H, W, seed=4)
    with _mode(strict):
        a = fwd_plain(raw, cam, raw_params)
        b = fwd_depth(raw, cam, raw_params)
        g_plain = bwd(a, dL)
        g_zero = bwd(b, dL, torch.zeros(H, W))
        g_prefix = bwd(b, dL)   # the colour-only backward on a depth forward's buffers
    for k in GRADS:
        np.testing.assert_array_equal(g_zero[k], g_plain[k], err_msg=f"dL_ddepth = 0: {k}")
        np.testing.assert_array_equal(g_prefix[k], g_plain[k], err_msg=f"plain backward on depth buffers: {k}")


def test_depth_backward_refuses_buffers_of_a_plain_forward():
    from gaussian_lic_amd import _lib
    raw, sc, camd, cam = make_scene("random", 2000, 96, 64, 3, 2)
    a = fwd_plain(raw, cam)
    with pytest.raises(_lib.GslicError, match="rendered no depth"):
        bwd(a, torch.zeros(3, 64, 96), torch.ones(64, 96))


def _view_row_is_not_symmetric(camd):
    V = np.asarray(camd["view"], np.float64).reshape(-1)
    return abs(V[2]) > 0.05 and abs(V[6]) > 0.05 and abs(V[2] - V[8]) > 0.05 and abs(V[6] - V[9]) > 0.05


# ------------------------------------------------------------------------------------------------------------------- 4. backward vs oracle
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("kind,P,W,H,deg,seed,view", [c + (None,) for c in DEPTH_CASES[:2]] + [("random", 10000, 640, 480, 0, 0, None),
                                                                                              ("random", 20000, 320, 240, 3, 8, POSE)])
def test_depth_backward_matches_oracle(oracle32, strict, kind, P, W, H, deg, seed, view):
    """strict: the row-scan kernel (render_bwd_scan_kernel<true>); fast: the pipeline kernel (render_bwd_kernel<false, true>), held with the
    flip allowance of the colour's fast-mode tests (tests/test_vs_reference_kernels_gpu.py)."""
    from gaussian_lic_amd.synthetic import pixel_grad
    raw, sc, camd, cam = make_scene(kind, P, W, H, deg, seed, view=view)
    if view is not None:
        assert _view_row_is_not_symmetric(camd)
    dL = pixel_grad(H, W, seed=1)
    gD = torch.randn(H, W, generator=torch.Generator().manual_seed(11)).float()
    with _mode(strict):
        f = fwd_depth(raw, cam)
        got = bwd(f, dL, gD)
        g_col = bwd(f, dL)
    ref = oracle32.forward(sc, camd)
    exp = oracle_backward_depth(oracle32, sc, camd, ref, dL.numpy(), gD.numpy())
    vis = ref["pre"]["radii"] > 0
    for k in GRADS:
        assert np.all(got[k].reshape(P, -1)[~vis] == 0), f"{k}: invisible rows must be exact zeros"
        if not strict:
            assert_close_flips(got[k], exp[k], TOL, k, flip_bound=2e-2)
            continue
        a_, b_ = got[k].reshape(-1).astype(np.float64), exp[k].reshape(-1).astype(np.float64)
        scale = np.abs(b_).max() if b_.size else 0.0
        if k == "dL_drot":  # exactly 0 for isotropic Gaussians: measure against the magnitude of the cancelling terms
            scale = max(scale, float(np.abs(exp["dL_dscale"]).max() * sc["scales"].max()))
        err_ = np.abs(a_ - b_) / max(scale, 1e-30) if b_.size else np.zeros(1)
        assert err_.max() < TOL, f"{k}: {int((err_ > TOL).sum())} elements > {TOL}, max rel err {err_.max():.3e}"
    # the depth term has teeth: without it dL_dmean3D is the colour-only gradient, far from the expected one
    assert rel_err(g_col["dL_dmean3D"], exp["dL_dmean3D"]) > 100 * TOL


def test_depth_strict_backward_on_a_fast_forward(oracle32):
    """A fast forward records no decision bits: the strict depth backward then runs the pipeline kernel's fallback (render_bwd_kernel<true, true>
    re-deriving the decisions), which must give the fast depth backward's gradients bit for bit, with a non-zero dL_ddepth — and those are
    the oracle's up to the fast mode's flipped cuts."""
    from gaussian_lic_amd.synthetic import pixel_grad
    W, H = 320, 240
    raw, sc, camd, cam = make_scene("random", 20000, W, H, 3, 8, view=POSE)
    dL = pixel_grad(H, W, seed=1)
    gD = torch.randn(H, W, generator=torch.Generator().manual_seed(12)).float()
    with _mode(False):
        f = fwd_depth(raw, cam)
        g_ff = bwd(f, dL, gD)
    with _mode(True):
        g_fs = bwd(f, dL, gD)
    ref = oracle32.forward(sc, camd)
    exp = oracle_backward_depth(oracle32, sc, camd, ref, dL.numpy(), gD.numpy())
    for k in GRADS:
        np.testing.assert_array_equal(g_fs[k], g_ff[k], err_msg=k)
        assert_close_flips(g_fs[k], exp[k], TOL, k, flip_bound=2e-2)


# ------------------------------------------------------------------------------------------------------------- 5. finite differences
def test_depth_gradient_matches_finite_differences(oracle64):
    """Central differences of the double-precision oracle's depth image under L = sum w depth, on ~20 visible Gaussians, against the HIP
    gradients of gslic_rasterize_backward_depth (dL_dpix = 0): pins the sign and the index of the view-row chain on its own — under a general
    pose, where row 2 and column 2 of the view matrix differ."""
    W, H = 64, 48
    raw, sc, camd, cam = make_scene("random", 40, W, H, 3, 4, view=POSE)
    assert _view_row_is_not_symmetric(camd)
    sc = {k: (np.asarray(v, np.float64) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v) for k, v in sc.items()}
    rng = np.random.default_rng(0)
    w = rng.standard_normal((H, W))

    def loss(s):
        f = oracle64.forward(s, camd)
        return float((oracle_depth(oracle64, f, W, H)[0] * w).sum()), f

    l0, f0 = loss(sc)
    vis = np.flatnonzero(f0["pre"]["radii"] > 0)
    assert len(vis) >= 15
    f = fwd_depth(raw, cam)
    g = bwd(f, torch.zeros(3, H, W), torch.from_numpy(w).float())
    checked = 0
    for key, gname in (("means", "dL_dmean3D"), ("opac", "dL_dopacity"), ("scales", "dL_dscale")):
        G = g[gname].reshape(sc[key].shape[0], -1)
        scale = max(float(np.abs(G[vis]).max()), 1e-12)
        for i in vis:
            for c in range(G.shape[1]):
                base = sc[key].reshape(sc[key].shape[0], -1)
                h = 1e-6 * max(1.0, abs(float(base[i, c])))
                sp, sm = dict(sc), dict(sc)
                sp[key] = sc[key].copy(); sp[key].reshape(sp[key].shape[0], -1)[i, c] += h
                sm[key] = sc[key].copy(); sm[key].reshape(sm[key].shape[0], -1)[i, c] -= h
                lp, fp = loss(sp)
                lm, fm = loss(sm)
                if (fp["num_rendered"] != f0["num_rendered"] or fm["num_rendered"] != f0["num_rendered"]
                        or not np.array_equal(fp["n_contrib"], f0["n_contrib"]) or not np.array_equal(fm["n_contrib"], f0["n_contrib"])):
                    continue  # a discrete decision moved inside the step: the difference straddles a discontinuity
                fd = (lp - lm) / (2 * h)
                assert abs(fd - float(G[i, c])) <= 2e-3 * scale + 1e-6, (gname, i, c, fd, float(G[i, c]))
                checked += 1
    assert checked >= 100, checked


# ----------------------------------------------------------------------------------------------------------------- 6. autograd, trainer
class _ActModel:
    """A model that offers only the activated accessors (render() then takes the operator path, raw=False)."""

    def __init__(self, act):
        self.t = {k: (v.clone().requires_grad_(True) if torch.is_tensor(v) and k != "D" else v) for k, v in act.items()}
        self.sh_degree, self.lambda_erank = act["D"], 0.0

    def get_xyz(self): return self.t["means"]
    def get_opacity(self): return self.t["opac"]
    def get_scaling(self): return self.t["scales"]
    def get_rotation(self): return self.t["rots"]
    def get_features_dc(self): return self.t["dc"]
    def get_features_rest(self): return self.t["shs"]


@pytest.mark.parametrize("raw_path", [True, False])
def test_render_return_depth_autograd_matches_the_c_abi(raw_path):
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.rasterizer import render
    from gaussian_lic_amd.synthetic import activate, pixel_grad
    dev = gpu()
    W, H = 200, 150
    raw, sc, camd, cam = make_scene("random", 8000, W, H, 3, 6)
    cam.to_device(dev)
    bg = torch.zeros(3, device=dev)
    wc = pixel_grad(H, W, seed=7).to(dev)
    wd = torch.randn(H, W, generator=torch.Generator().manual_seed(8)).float().to(dev)
    if raw_path:
        model = trainer.GaussianModel({k: (v.clone() if torch.is_tensor(v) else v) for k, v in raw.items()}, dev)
        leaves = [model.xyz, model.features_dc, model.features_rest, model.opacity, model.scaling, model.rotation]
    else:
        model = _ActModel({k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in activate(raw).items()})
        leaves = [model.t[k] for k in ("means", "dc", "shs", "opac", "scales", "rots")]
    image, final_T, _pts, vis, radii, depth = render(cam, model, bg, return_depth=True)
    assert depth.shape == (H, W) and depth.requires_grad
    ((image * wc).sum() + (depth * wd).sum()).backward()
    # the same through the C-ABI directly
    f = fwd_depth(raw, cam, raw_params=raw_path)
    torch.testing.assert_close(depth.detach(), f["depth"], rtol=0, atol=0)
    g = bwd(f, wc, wd)
    for leaf, k in zip(leaves, ("dL_dmean3D", "dL_ddc", "dL_dsh", "dL_dopacity", "dL_dscale", "dL_drot")):
        np.testing.assert_array_equal(leaf.grad.detach().cpu().numpy().reshape(-1), g[k].reshape(-1), err_msg=k)
    # and the five other results of render() are those of return_depth=False
    with torch.no_grad():
        i2, T2, _, v2, r2 = render(cam, model, bg)
    assert torch.equal(i2, image.detach()) and torch.equal(T2, final_T) and torch.equal(r2, radii) and torch.equal(v2, vis)


def test_morton_model_depth_is_bit_identical():
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.rasterizer import render
    from gaussian_lic_amd.synthetic import random_scene
    dev = gpu()
    W, H = 320, 192
    raw = random_scene(30000, W, H, sh_degree=3, seed=5)
    z = raw["xyz"][:, 2]
    zq = torch.where(z > 0.3, (z / 0.5).round().clamp_min(1.0) * 0.5, z)   # many exact depth ties: the tie rule matters
    raw["xyz"] = torch.stack([raw["xyz"][:, 0] * zq / z, raw["xyz"][:, 1] * zq / z, zq], 1).contiguous()
    a = trainer.GaussianModel({k: (v.clone() if torch.is_tensor(v) else v) for k, v in raw.items()}, dev)
    b = trainer.GaussianModel({k: (v.clone() if torch.is_tensor(v) else v) for k, v in raw.items()}, dev, order="morton")
    cam = synthetic_camera(W, H).to_device(dev)
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        ia, Ta, _, _, _, da = render(cam, a, bg, return_depth=True)
        ib, Tb, _, _, _, db = render(cam, b, bg, return_depth=True)
    assert torch.equal(da, db) and torch.equal(ia, ib) and torch.equal(Ta, Tb)
    assert float(da.abs().max()) > 0


def _params(m):
    return [getattr(m, n).detach().clone() for n in m.NAMES]


def test_training_step_lambda_depth_zero_is_the_colour_step():
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.synthetic import gt_image
    dev = gpu()
    W, H = 160, 120
    raw, sc, camd, cam = make_scene("random", 5000, W, H, 3, 9)
    cam.to_device(dev)
    a = trainer.GaussianModel({k: (v.clone() if torch.is_tensor(v) else v) for k, v in raw.items()}, dev); a.training_setup()
    b = trainer.GaussianModel({k: (v.clone() if torch.is_tensor(v) else v) for k, v in raw.items()}, dev); b.training_setup()
    gt, bg = gt_image(H, W).to(dev), torch.zeros(3, device=dev)
    gtd = torch.rand(H, W, device=dev) * 3.0
    for _ in range(3):
        la, _ = trainer.training_step(a, cam, gt, bg)
        lb, _ = trainer.training_step(b, cam, gt, bg, gt_depth=gtd, lambda_depth=0.0)
        assert float(la) == float(lb)
    for x, y in zip(_params(a), _params(b)):
        assert torch.equal(x, y)


def test_depth_supervision_pulls_the_map_toward_the_target_depth():
    """50 steps toward a target that renders the same image at 1.2x the depth (positions and extents scaled about the camera centre):
    with lambda_depth > 0 the depth L1 falls below its start and below the same run without depth supervision."""
    import math
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.loss import depth_l1
    from gaussian_lic_amd.rasterizer import render
    dev = gpu()
    W, H = 160, 120
    raw, sc, camd, cam = make_scene("random", 3000, W, H, 3, 10)
    cam.to_device(dev)
    bg = torch.zeros(3, device=dev)
    tgt = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in raw.items()}
    tgt["xyz"] = (raw["xyz"] * 1.2).contiguous()
    tgt["scaling"] = (raw["scaling"] + math.log(1.2)).contiguous()
    with torch.no_grad():
        gt, _, _, _, _, gtd = render(cam, trainer.GaussianModel(tgt, dev), bg, return_depth=True)

    def run(lam):
        m = trainer.GaussianModel({k: (v.clone() if torch.is_tensor(v) else v) for k, v in raw.items()}, dev); m.training_setup()
        with torch.no_grad():
            d0 = float(depth_l1(render(cam, m, bg, return_depth=True)[5], gtd))
        for _ in range(50):
            trainer.training_step(m, cam, gt, bg, gt_depth=gtd, lambda_depth=lam)
        with torch.no_grad():
            d1 = float(depth_l1(render(cam, m, bg, return_depth=True)[5], gtd))
        return d0, d1

    s_on, e_on = run(1.0)
    s_off, e_off = run(0.0)
    assert s_on == s_off and s_on > 0
    assert e_on < s_on and e_on < e_off, (s_on, e_on, e_off)


# ---------------------------------------------------------------------------------------------------- 7. determinism and edge cases
def test_depth_forward_backward_is_deterministic():
    from gaussian_lic_amd.synthetic import pixel_grad
    from gpu_helpers import npy
    raw, sc, camd, cam = make_scene("random", 60000, 480, 270, 3, 12)
    dL = pixel_grad(270, 480, seed=2)
    gD = torch.randn(270, 480, generator=torch.Generator().manual_seed(3)).float()
    runs = []
    for strict in (True, False):
        with _mode(strict):
            for _ in range(2):
                f = fwd_depth(raw, cam)
                runs.append((npy(f["depth"]), npy(f["color"]), bwd(f, dL, gD)))
    for i in (0, 2):
        a, b = runs[i], runs[i + 1]
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        for k in GRADS:
            np.testing.assert_array_equal(a[2][k], b[2][k], err_msg=k)


def test_depth_edge_cases(oracle32):
    from gaussian_lic_amd import rasterizer as rz
    from gaussian_lic_amd.synthetic import pixel_grad
    from gpu_helpers import npy
    dev = gpu()
    # P = 0
    e3 = torch.empty(0, 3, device=dev)
    out = rz.rasterize_gaussians_depth(torch.zeros(3, device=dev), e3, torch.empty(0, 1, device=dev), e3, torch.empty(0, 4, device=dev), 1.0,
                                      torch.eye(4, device=dev), torch.eye(4, device=dev), 0.5, 0.5, 50, 70, -1, 1, -1, 1,
                                      torch.empty(0, 1, 3, device=dev), torch.empty(0, 0, 3, device=dev), 0, torch.zeros(3, device=dev))
    assert out[0] == 0 and out[1] == 0 and float(out[4].abs().sum()) == 0 and out[4].shape == (50, 70)
    # a scene entirely behind the camera: nothing visible, depth 0, gradients exact zeros
    raw, sc, camd, cam = make_scene("random", 500, 70, 50, 3, 13)
    raw["xyz"] = torch.stack([raw["xyz"][:, 0], raw["xyz"][:, 1], -raw["xyz"][:, 2].abs() - 1.0], 1).contiguous()
    f = fwd_depth(raw, cam)
    assert f["R"] == 0 and int((f["radii"] > 0).sum()) == 0 and float(f["depth"].abs().sum()) == 0
    g = bwd(f, pixel_grad(50, 70), torch.ones(50, 70))
    for k in GRADS:
        assert np.all(g[k] == 0), k
    # SH degree 0 with M = 0 on a ragged 70x50 image
    raw, sc, camd, cam = make_scene("random", 3000, 70, 50, 0, 14)
    f = fwd_depth(raw, cam)
    ref = oracle32.forward(sc, camd)
    assert rel_err(npy(f["depth"]), oracle_depth(oracle32, ref, 70, 50)[0]) < TOL
    gD = torch.randn(50, 70, generator=torch.Generator().manual_seed(5)).float()
    got = bwd(f, pixel_grad(50, 70), gD)
    exp = oracle_backward_depth(oracle32, sc, camd, ref, pixel_grad(50, 70).numpy(), gD.numpy())
    for k in ("dL_dmean3D", "dL_dopacity", "dL_dscale", "dL_ddc"):
        assert rel_err(got[k], exp[k]) < TOL, k
