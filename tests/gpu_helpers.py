"""Helpers shared by the -m gpu tests: run the HIP path through the C-ABI front-end on seeded scenes, build the small models the statistics
tests share, and compare tensors, model states, maps and guard words.  Importable without a GPU: whatever touches the device or loads
libgslic_hip.so happens inside the functions."""
import types

import numpy as np
import torch

from gaussian_lic_amd import rasterizer as rz
from gaussian_lic_amd.synthetic import activate

SENTINEL = 0x5A5A5A5A   # the guard word of guarded(), and what the tests fill rows with that no kernel may write
GUARD = 64              # guard words on either side of a guarded() buffer


def gpu():
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32)


def same_tensors(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def guarded(n, dtype=torch.int32, fill=None, device=None, sentinel=SENTINEL):
    """A buffer of n words of `dtype` between two runs of GUARD guard words: (whole buffer, the n words as a view, set to `fill` if given)."""
    buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=gpu() if device is None else device)
    words = buf[GUARD:GUARD + n]
    if fill is not None:
        words.fill_(fill)
    return buf, words


def guards_intact(buf, n, sentinel=SENTINEL):
    return bool((buf[:GUARD] == sentinel).all()) and bool((buf[GUARD + n:] == sentinel).all())


def scene_model(name, order="insertion", **kw):
    """(GaussianModel of contribution_ref.scene(name), its synthetic camera on the device)."""
    import contribution_ref as cr
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    raw, W, H = cr.scene(name)
    m = trainer.GaussianModel(cr._clone(raw), gpu(), order=order, **kw)
    return m, synthetic_camera(W, H).to_device(gpu())


def training_model(raw):
    """A GaussianModel of a copy of the raw parameters on the device, with its optimizer set up."""
    from gaussian_lic_amd import trainer
    m = trainer.GaussianModel({k: (v.clone() if torch.is_tensor(v) else v) for k, v in raw.items()}, gpu())
    m.training_setup()
    return m


def raw_forward(m, cam, depth=False, bufs=None):
    """A trainer._RawRaster of the model after its forward (black background, no autograd)."""
    from gaussian_lic_amd import trainer
    fwd = trainer._RawRaster(m, cam, torch.zeros(3, device=gpu()), depth=depth)
    with torch.no_grad():
        fwd.forward(bufs)
    return fwd


def export_lists(m, cam, fwd, what):
    """rasterizer.debug_export of the lists a raw_forward left behind: the dict of the arrays named in `what`."""
    H, W = fwd.hw
    rs = types.SimpleNamespace(image_height=H, image_width=W, sh_degree=m.sh_degree, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, limx_neg=cam.limx_neg,
                               limx_pos=cam.limx_pos, limy_neg=cam.limy_neg, limy_pos=cam.limy_pos, scale_modifier=1.0, no_color=False)
    R, B, _radii, geom, binning, img, sample = fwd.state
    return rz.debug_export(rs, m.P, 0, R, B, geom, binning, img, sample, what=tuple(what))


def model_state(m):
    """Parameters and both Adam moments of every group, as host copies."""
    out = {}
    for i, n in enumerate(m.NAMES):
        out[n] = getattr(m, n).detach().cpu().clone()
        st = m.optimizer.state[i]
        if st is not None:
            out[n + ".m"] = st["exp_avg"].cpu().clone()
            out[n + ".v"] = st["exp_avg_sq"].cpu().clone()
    return out


def assert_same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def map_snapshot(m, order=None, tie=False):
    """Copies of the map's rows [0, P): parameters and both moments per group (rows listed by `order` when given), with tie=True also the
    tie rank as int64 (None for an insertion-order map)."""
    P = m.P
    pick = (lambda t: t[:P].clone()) if order is None else (lambda t: t[:P][order].clone())
    out = {}
    for n in m.NAMES:
        out[n] = pick(m._buf[n]); out[n + ".m"] = pick(m._m[n]); out[n + ".v"] = pick(m._v[n])
    if tie:
        out["tie"] = None if m._tie is None else m._tie[:P].clone().long()
    return out


def same_map(a, b, view=bits):
    """Asserts that the Morton-ordered model b holds the insertion-order model a's map: parameters and both moments, b's rows taken in their
    original order.  `view` is what torch.equal sees: the bits, or (view=None) the floats themselves."""
    view = view or (lambda t: t)
    order = b.original_order()
    for n in a.NAMES:
        assert torch.equal(view(getattr(a, n).detach()), view(getattr(b, n).detach()[order])), n
    for n in a.NAMES:
        assert torch.equal(view(a._m[n][:a.P]), view(b._m[n][:b.P][order])) and torch.equal(view(a._v[n][:a.P]), view(b._v[n][:b.P][order])), n


def settings_from(cam, deg, dev, no_color=False, lambda_erank=0.0, debug=False, scale_modifier=1.0):
    return rz.GaussianRasterizationSettings(
        cam.image_height, cam.image_width, float(cam.tanfovx), float(cam.tanfovy), float(cam.limx_neg), float(cam.limx_pos),
        float(cam.limy_neg), float(cam.limy_pos), torch.zeros(3, device=dev), float(scale_modifier),
        torch.from_numpy(cam.world_view_transform).to(dev), torch.from_numpy(cam.full_proj_transform).to(dev), deg,
        torch.from_numpy(cam.camera_center).to(dev), False, debug, no_color, lambda_erank)


def hip_forward(raw, cam, no_color=False, export=(), debug=False, scale_modifier=1.0, tie_rank=None, act=None):
    """tie_rank: int32 device tensor [P] — the rows' original indices when the map's rows are given in a permuted order
    (gslic_raster_params.tie_rank: what trainer.GaussianModel(order="morton") passes).
    act: the ACTIVATED scene (synthetic.activate's dict) instead of `raw` — a caller that permutes rows activates first and permutes the activated
    tensors, so that both sides of a comparison see the same bits whatever the host's LibTorch does at its chunk boundaries."""
    dev = torch.device("cuda:0")
    act = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in (activate(raw) if act is None else act).items()}
    rs = settings_from(cam, act["D"], dev, no_color, debug=debug, scale_modifier=scale_modifier)
    empty = torch.empty(0, device=dev)
    out = rz.rasterize_gaussians(rs.bg, act["means"], empty, act["opac"], act["scales"], act["rots"], rs.scale_modifier, empty, rs.viewmatrix,
                                 rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, rs.limx_neg, rs.limx_pos,
                                 rs.limy_neg, rs.limy_pos, act["dc"], act["shs"], act["D"], rs.campos, False, debug, no_color, tie_rank=tie_rank)
    R, B, color, final_T, radii, geom, binning, img, sample = out
    res = dict(R=R, B=B, color=color, final_T=final_T, radii=radii, bufs=(geom, binning, img, sample), act=act, rs=rs)
    if export:
        P = act["means"].shape[0]
        M = act["shs"].shape[1] if act["shs"].numel() else 0
        res["dbg"] = rz.debug_export(rs, P, M, R, B, geom, binning, img, sample, what=tuple(export))
    torch.cuda.synchronize()
    return res


def hip_backward(fwd, dL_dpix, lambda_erank=0.0):
    act, rs = fwd["act"], fwd["rs"]
    dev = act["means"].device
    empty = torch.empty(0, device=dev)
    geom, binning, img, sample = fwd["bufs"]
    g = rz.rasterize_gaussians_backward(rs.bg, act["means"], fwd["radii"], empty, act["scales"], act["rots"], rs.scale_modifier, empty,
                                        rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.limx_neg, rs.limx_pos,
                                        rs.limy_neg, rs.limy_pos, dL_dpix.to(dev), act["dc"], act["shs"], act["D"], rs.campos,
                                        geom, fwd["R"], binning, img, fwd["B"], sample, lambda_erank, False)
    torch.cuda.synchronize()
    names = ["dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmean3D", "dL_dcov3D", "dL_ddc", "dL_dsh", "dL_dscale", "dL_drot"]
    return {n: t.cpu().numpy() for n, t in zip(names, g)}


def npy(t):
    return t.detach().cpu().numpy()


def hip_extend_rows(points, colors, depths_rsp, R_cw, t_cw, intr, W, H, final_T, M=15, scaling_scale=1.0):
    """gslic_extend_select + gslic_extend_emit on a given transmittance image (what trainer.GaussianModel.extend runs after its no_color
    render): returns (k, dict of the six new-Gaussian row tensors as numpy, ascending point index)."""
    import ctypes
    from gaussian_lic_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    pts, col, rsp, Rc, tc, fT = t(points), t(colors), t(depths_rsp), t(R_cw), t(t_cw), t(final_T)
    n = int(pts.shape[0])
    fx, fy, cx, cy = (float(v) for v in intr)
    scratch = _lib.TensorAllocator(dev)
    flags, pos, count = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int32(0)
    p = _lib.ptr
    _lib.check(L.gslic_extend_select(n, p(pts), p(rsp), p(Rc), p(tc), fx, fy, cx, cy, int(W), int(H), p(fT), scratch.cb, None, ctypes.byref(flags),
                                     ctypes.byref(pos), ctypes.byref(count), _lib.current_stream_ptr()))
    k = count.value
    rows = dict(xyz=torch.empty(k, 3, device=dev), dc=torch.empty(k, 1, 3, device=dev), rest=torch.empty(k, M, 3, device=dev),
                opacity=torch.empty(k, 1, device=dev), scaling=torch.empty(k, 3, device=dev), rotation=torch.empty(k, 4, device=dev))
    if k:
        q = lambda x: ctypes.c_void_p(x.data_ptr()) if x.numel() else None
        _lib.check(L.gslic_extend_emit(n, flags, pos, p(pts), p(col), p(rsp), float(scaling_scale), (fx + fy) / 2.0, int(M), q(rows["xyz"]), q(rows["dc"]),
                                       q(rows["rest"]), q(rows["opacity"]), q(rows["scaling"]), q(rows["rotation"]), _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    return k, {key: v.cpu().numpy() for key, v in rows.items()}
