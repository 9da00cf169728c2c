"""Expected results of gslic_rasterize_backward_depth_camera, composed from the oracle's library functions (no oracle change): the depth is
rendered as a colour (rgb := [z, 0, 0], as tests/test_depth_gpu.py does for the nine ordinary gradients), the per-Gaussian chain is
orc_preprocess_backward_cam on the summed 2D gradients with the colour pass's dL_dcolor, and the direct term through
z = V[2] x + V[6] y + V[10] z + V[14] is added in numpy:  dV[2, 6, 10] += sum_i dz_i p_i,  dV[14] += sum_i dz_i,  dz = the depth pass's
dL_dcolor[:, 0]."""
import ctypes

import numpy as np

GRADS = ("dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmean3D", "dL_dcov3D", "dL_ddc", "dL_dsh", "dL_dscale", "dL_drot")
CAM = ("dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos")
VIEW_IDX = [4 * c + r for c in range(4) for r in range(3)]
PROJ_IDX = [4 * c + r for c in range(4) for r in (0, 1, 3)]


def oracle_depth(orc, ref, W, H):
    """The oracle's depth image: its blend with rgb := [z, 0, 0] (same alphas, cut-offs and early stop as the colour)."""
    pre = dict(ref["pre"])
    rgb = np.zeros_like(pre["rgb"])
    rgb[:, 0] = pre["depths"]
    pre["rgb"] = rgb
    return orc.render_forward(pre, ref["bins"], W, H)["color"][0], pre


def oracle_backward_depth_camera(orc, sc, camd, ref, dL_dpix, dL_ddepth):
    """The twelve expected outputs (GRADS + CAM) for loss = <dL_dpix, colour> + <dL_ddepth, depth>, plus "direct": the four numbers added to
    dL_dviewmatrix[2, 6, 10, 14], and "dL_dconic"."""
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
                                    _ptr(ref["n_contrib"]), _ptr(dl), _ptr(g["m2"]), _ptr(g["con"]), _ptr(g["op"]), _ptr(g["col"]))
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
    camg = np.zeros(35, np.float64)
    orc.lib.orc_preprocess_backward_cam(
        ctypes.c_int(P), ctypes.c_int(int(sc["D"])), ctypes.c_int(M), _ptr(means), _ptr(pre["radii"]), _ptr(dc), _ptr(shs), _ptr(pre["clamped"]),
        _ptr(scales), _ptr(rots), r(1.0), _ptr(pre["cov3D"]), _ptr(view), _ptr(proj), ctypes.c_int(W), ctypes.c_int(H), r(camd["tanfovx"]),
        r(camd["tanfovy"]), r(camd["limx_neg"]), r(camd["limx_pos"]), r(camd["limy_neg"]), r(camd["limy_pos"]), _ptr(campos), _ptr(m2),
        _ptr(con), _ptr(gc["col"]), _ptr(g["dL_dmean3D"]), _ptr(g["dL_dcov3D"]), _ptr(g["dL_ddc"]), _ptr(g["dL_dsh"]) if M > 0 else None,
        _ptr(g["dL_dscale"]), _ptr(g["dL_drot"]), r(0.0), _ptr(camg))
    V = np.asarray(camd["view"], np.float64).reshape(-1)
    dz = gd["col"][:, 0].astype(np.float64)
    p = np.asarray(sc["means"], np.float64)
    direct = np.concatenate([(dz[:, None] * p).sum(0), [dz.sum()]])
    dV = camg[:16].copy()
    dV[[2, 6, 10, 14]] += direct
    g["dL_dmean3D"] = g["dL_dmean3D"] + dz[:, None] * np.array([V[2], V[6], V[10]])[None, :]
    g["dL_dopacity"] = gc["op"].astype(np.float64) + gd["op"]
    g["dL_dmean2D"], g["dL_dconic"], g["dL_dcolor"] = m2, con.reshape(P, 2, 2), gc["col"]
    g["dL_dviewmatrix"], g["dL_dprojmatrix"], g["dL_dcampos"] = dV, camg[16:32].copy(), camg[32:].copy()
    g["direct"] = direct
    return g
