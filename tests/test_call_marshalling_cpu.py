"""CPU-only: what rasterizer.py hands to the library.  _lib.lib is replaced by a recorder that returns 0 for every symbol, so nothing runs;
every input is a CPU tensor of its own and each pointer argument is recorded as the NAME of the tensor it points at (NULL as "NULL", a
tensor the function returned as "ret[i]", one it allocated and kept to itself as "internal#k").

The expected records (test_call_marshalling_cpu.json) were produced by running this file against rasterizer.py of the commit BEFORE its
four forwards / two backwards were folded into one private forward and one private backward:
    GSLIC_MARSHALLING_WRITE=1 python -m pytest tests/test_call_marshalling_cpu.py
The argtypes table below is a literal copy of what _lib.py of that commit declared."""
import ctypes
import json
import os
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
JSON_PATH = os.path.join(HERE, "test_call_marshalling_cpu.json")
P, W, H, M, DEG = 8, 32, 16, 3, 1
STREAM = 0x5eadbeef


def _mods():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib, rasterizer
    return _lib, rasterizer


class Recorder:
    """Stands in for the loaded library: every attribute is a function that records its arguments and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, sym):
        def fn(*args):
            self.calls.append((sym, args))
            return 0
        return fn


class Names:
    def __init__(self):
        self.t = {}

    def new(self, name, *shape, dtype=torch.float32):
        self.t[name] = torch.zeros(*shape, dtype=dtype)
        return self.t[name]

    def lookup(self, addr, extra, internal):
        if addr is None or addr == 0:
            return "NULL"
        if addr == STREAM:
            return "stream"
        for table in (extra, self.t):
            for n, t in table.items():
                if t is not None and t.numel() and t.data_ptr() <= addr < t.data_ptr() + t.numel() * t.element_size():
                    off = addr - t.data_ptr()
                    return n if off == 0 else f"{n}+{off}"
        return internal.setdefault(addr, f"internal#{len(internal)}")


def _describe(a, lookup, _lib):
    if a is None:
        return "NULL"
    if isinstance(a, (bool, int, float)):
        return a
    if isinstance(a, ctypes.c_void_p):
        return lookup(a.value)
    if isinstance(a, _lib.ALLOC_FN):
        return "alloc_cb"
    obj = getattr(a, "_obj", a)   # ctypes.byref(x)
    if isinstance(obj, _lib.RasterParams):
        return {"RasterParams": {n: (lookup(getattr(obj, n)) if n == "tie_rank" else getattr(obj, n)) for n, _t in obj._fields_}}
    if isinstance(obj, _lib.AdamFused):
        d = {k: [lookup(v) for v in getattr(obj, k)] for k in ("param", "exp_avg", "exp_avg_sq")}
        d.update(lr=list(obj.lr), b1=obj.b1, b2=obj.b2, eps=obj.eps, visible_out=lookup(obj.visible_out))
        return {"AdamFused": d}
    if isinstance(obj, ctypes.c_int32):
        return "int32*"
    raise TypeError(f"unexpected argument {a!r}")


def _flatten(ret, prefix="ret"):
    out = {}
    if torch.is_tensor(ret):
        out[prefix] = ret
    elif isinstance(ret, (tuple, list)):
        for i, r in enumerate(ret):
            out.update(_flatten(r, f"{prefix}[{i}]"))
    elif isinstance(ret, dict):
        for k, r in ret.items():
            out.update(_flatten(r, f"{prefix}[{k}]"))
    return out


def _shape_of(ret):
    if torch.is_tensor(ret):
        return [str(ret.dtype).replace("torch.", "")] + list(ret.shape)
    if isinstance(ret, (tuple, list)):
        return [_shape_of(r) for r in ret]
    if isinstance(ret, dict):
        return {k: _shape_of(r) for k, r in ret.items()}
    return ret


def _record_all(monkeypatch):
    _lib, rz = _mods()
    rec = Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "current_stream_ptr", lambda: ctypes.c_void_p(STREAM))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)   # (debug_export synchronises; nothing ran)
    nm = Names()
    f = nm.new
    bg, xyz, dc, sh = f("background", 3), f("means3D", P, 3), f("dc", P, 1, 3), f("sh", P, M, 3)
    op, sc, rot = f("opacity", P, 1), f("scales", P, 3), f("rotations", P, 4)
    view, proj, campos = f("viewmatrix", 4, 4), f("projmatrix", 4, 4), f("campos", 3)
    tie = f("tie_rank", P, dtype=torch.int32)
    radii = f("radii", P, dtype=torch.int32)
    geom, binning, img, sample = (f(n, 64, dtype=torch.uint8) for n in ("geom", "binning", "img", "sample"))
    dL, dLd = f("dL_dcolor", 3, H, W), f("dL_ddepth", H, W)
    e = torch.empty(0)
    out = {k: f("out_" + k, *s) for k, s in dict(xyz=(P, 3), features_dc=(P, 1, 3), features_rest=(P, M, 3), opacity=(P, 1), scaling=(P, 3),
                                                 rotation=(P, 4)).items()}
    rgb_out, pay_vis, pay_campos, xyz_grad = f("rgb_out", P, 3), f("pay_vis", P, dtype=torch.uint8), f("pay_campos", 3), f("xyz_grad", P, 3)
    vis_out = f("visible_out", P, dtype=torch.uint8)
    adam = _lib.AdamFused()
    for g, (prm_t, shape) in enumerate(((xyz, (P, 3)), (dc, (P, 1, 3)), (sh, (P, M, 3)), (op, (P, 1)), (sc, (P, 3)), (rot, (P, 4)))):
        adam.param[g] = prm_t.data_ptr()
        adam.exp_avg[g], adam.exp_avg_sq[g] = f(f"exp_avg{g}", *shape).data_ptr(), f(f"exp_avg_sq{g}", *shape).data_ptr()
        adam.lr[g] = 0.5 ** g
    adam.b1, adam.b2, adam.eps, adam.visible_out = 0.5, 0.75, 0.125, vis_out.data_ptr()

    def bufs(depth, no_color=False):
        b = types.SimpleNamespace(P=P, W=W, H=H, no_color=no_color, with_depth=depth, cap_R=0, cap_B=0)
        tag = "capd_" if depth else "cap_"
        for n in ("geom", "binning", "img", "sample"):
            setattr(b, n, f(tag + n, 48 if n == "geom" else 80, dtype=torch.uint8))
        b.status, b.color, b.final_T = f(tag + "status", 8, dtype=torch.int32), f(tag + "color", 3, H, W), f(tag + "final_T", H, W)
        b.depth = f(tag + "depth", H, W) if depth else None
        b.radii = f(tag + "radii", P, dtype=torch.int32)
        return b

    cam = (1.25, 0.75, -1.5, 1.625, -0.875, 0.9375)   # tanfovx, tanfovy, limx_neg, limx_pos, limy_neg, limy_pos
    records = {}

    def drive(label, fn, *args, **kw):
        rec.calls.clear()
        ret = fn(*args, **kw)
        extra, internal = _flatten(ret), {}
        lookup = lambda addr: nm.lookup(addr, extra, internal)
        records[label] = dict(calls=[[sym, [_describe(a, lookup, _lib) for a in cargs]] for sym, cargs in rec.calls], ret=_shape_of(ret))

    for raw in (False, True):
        for tr in (None, tie):
            tag = f"raw={int(raw)},tie={int(tr is not None)}"
            drive(f"forward[{tag}]", rz.rasterize_gaussians, bg, xyz, e, op, sc, rot, 1.5, e, view, proj, cam[0], cam[1], H, W, *cam[2:], dc, sh, DEG, campos,
                  False, False, False, raw_params=raw, tie_rank=tr)
            drive(f"forward_depth[{tag}]", rz.rasterize_gaussians_depth, bg, xyz, op, sc, rot, 1.5, view, proj, cam[0], cam[1], H, W, *cam[2:], dc, sh, DEG,
                  campos, raw_params=raw, tie_rank=tr)
            drive(f"forward_capacity[{tag}]", rz.rasterize_gaussians_capacity, bufs(False), bg, xyz, op, sc, rot, 1.5, view, proj, *cam, dc, sh, DEG, campos,
                  raw_params=raw, tie_rank=tr)
            drive(f"forward_depth_capacity[{tag}]", rz.rasterize_gaussians_depth_capacity, bufs(True), bg, xyz, op, sc, rot, 1.5, view, proj, *cam, dc, sh,
                  DEG, campos, raw_params=raw, tie_rank=tr)
    drive("forward[no_color,prefiltered,debug]", rz.rasterize_gaussians, bg, xyz, e, op, sc, rot, 1.0, e, view, proj, cam[0], cam[1], H, W, *cam[2:], dc, sh,
          DEG, campos, True, True, True)
    drive("forward[P=0]", rz.rasterize_gaussians, bg, torch.zeros(0, 3), e, e, e, e, 1.0, e, view, proj, cam[0], cam[1], H, W, *cam[2:], e, e, DEG, campos,
          False, False)
    drive("forward_depth[P=0]", rz.rasterize_gaussians_depth, bg, torch.zeros(0, 3), e, e, e, 1.0, view, proj, cam[0], cam[1], H, W, *cam[2:], e, e, DEG,
          campos)
    drive("forward_capacity[no_color]", rz.rasterize_gaussians_capacity, bufs(False, True), bg, xyz, op, sc, rot, 1.0, view, proj, *cam, dc, sh, DEG, campos)
    drive("forward[M=0]", rz.rasterize_gaussians, bg, xyz, e, op, sc, rot, 1.0, e, view, proj, cam[0], cam[1], H, W, *cam[2:], dc, torch.zeros(P, 0, 3), 0,
          campos, False, False)

    def bwd(**kw):
        return (rz.rasterize_gaussians_backward, bg, xyz, radii, e, sc, rot, 1.5, e, view, proj, *cam, dL, dc, sh, DEG, campos, geom, 11, binning, img, 5,
                sample, 0.25, False), kw

    def bwd_depth(**kw):
        return (rz.rasterize_gaussians_backward_depth, bg, xyz, radii, sc, rot, 1.5, view, proj, *cam, dL, dLd, dc, sh, DEG, campos, geom, 11, binning, img,
                5, sample, 0.25, False), kw

    for label, (args, kw) in {
        "backward[plain]": bwd(), "backward[plain,raw]": bwd(raw_params=True), "backward[out]": bwd(raw_params=True, out=out),
        "backward[adam]": bwd(raw_params=True, adam=adam), "backward[camera_grads]": bwd(raw_params=True, camera_grads=True),
        "backward[camera_grads,out]": bwd(raw_params=True, camera_grads=True, out=out),
        "backward[rgb_out,payload]": bwd(raw_params=True, out=out, rgb_out=rgb_out, payload=(pay_vis, pay_campos)),
        "backward[rgb_out]": bwd(raw_params=True, out=out, rgb_out=rgb_out),
        "backward[rgb_out,rows]": bwd(raw_params=True, out=out, rgb_out=rgb_out, rows=(0, 8), skip_blend=False),
        "backward[rgb_out,rows,out_addr,skip_blend]": bwd(
            raw_params=True, out=out, rgb_out=rgb_out, rows=(64, 128), skip_blend=True,
            out_addr=dict(xyz=out["xyz"].data_ptr() + 12, opacity=out["opacity"].data_ptr() + 4, scaling=out["scaling"].data_ptr() + 24,
                          rotation=out["rotation"].data_ptr() + 16, rgb=rgb_out.data_ptr() + 36)),
        "backward_depth[plain]": bwd_depth(), "backward_depth[out]": bwd_depth(raw_params=True, out=out),
        "backward_depth[adam,xyz_grad]": bwd_depth(raw_params=True, adam=adam, xyz_grad=xyz_grad), "backward_depth[adam]": bwd_depth(adam=adam),
        "backward_depth[camera_grads]": bwd_depth(raw_params=True, camera_grads=True),
        "backward_depth[camera_grads,out]": bwd_depth(raw_params=True, camera_grads=True, out=out),
    }.items():
        drive(label, *args, **kw)
    z3 = torch.zeros(0, 3)
    drive("backward[P=0,camera_grads]", rz.rasterize_gaussians_backward, bg, z3, torch.zeros(0, dtype=torch.int32), e, e, e, 1.0, e, view, proj, *cam, dL, e,
          e, DEG, campos, geom, 0, binning, img, 0, sample, 0.0, False, camera_grads=True)
    drive("backward_depth[P=0,camera_grads]", rz.rasterize_gaussians_backward_depth, bg, z3, torch.zeros(0, dtype=torch.int32), e, e, 1.0, view, proj, *cam,
          dL, dLd, e, e, DEG, campos, geom, 0, binning, img, 0, sample, camera_grads=True)
    drive("backward_depth[P=0,adam]", rz.rasterize_gaussians_backward_depth, bg, z3, torch.zeros(0, dtype=torch.int32), e, e, 1.0, view, proj, *cam, dL, dLd,
          e, e, DEG, campos, geom, 0, binning, img, 0, sample, adam=adam)
    rgb_all, campos_all = f("rgb_all", 2, P, 3), f("campos_all", 2, 3)
    drive("sh_grad_from_rgb", rz.sh_grad_from_rgb, xyz, campos_all, rgb_all, DEG, out["features_dc"], out["features_rest"])
    drive("sh_grad_from_rgb[input_is_ddc,M=0]", rz.sh_grad_from_rgb, xyz, campos_all, rgb_all, 0, out["features_dc"], torch.zeros(P, 0, 3), input_is_ddc=True)
    drive("sh_grad_from_rgb[view_stride]", rz.sh_grad_from_rgb, xyz, campos_all, rgb_all, DEG, out["features_dc"], out["features_rest"], n_views=2,
          view_stride=40)
    rs = rz.GaussianRasterizationSettings(H, W, cam[0], cam[1], *cam[2:], bg, 1.5, view, proj, DEG, campos)
    drive("debug_export", rz.debug_export, rs, P, M, 11, 5, geom, binning, img, sample)
    drive("debug_export[all]", rz.debug_export, rs, P, M, 11, 5, geom, binning, img, sample,
          what=("tiles_touched", "means2D", "depths", "conic_opacity", "rgb", "sorted_keys", "point_list", "ranges", "n_contrib", "max_contrib"))
    return json.loads(json.dumps(records))


def test_every_call_reaches_the_library_with_the_same_arguments(monkeypatch):
    got = _record_all(monkeypatch)
    if os.environ.get("GSLIC_MARSHALLING_WRITE") == "1":
        with open(JSON_PATH, "w") as fh:
            json.dump(got, fh, indent=1, sort_keys=True)
            fh.write("\n")
    with open(JSON_PATH) as fh:
        want = json.load(fh)
    assert sorted(got) == sorted(want)
    for label in want:
        assert got[label] == want[label], label
    symbols = {c[0] for r in want.values() for c in r["calls"]}
    # (gslic_rasterize_backward_rgb is the C hosts' spelling: rasterizer.py always takes the payload or the rows variant)
    assert {s for s in symbols if s.startswith("gslic_rasterize_")} | {"gslic_rasterize_backward_rgb"} == \
        {s for s in ARGTYPES if s.startswith("gslic_rasterize_")}, "an entry point is never driven"


# one letter per argument: P params*, A allocator callback, v void*, z size_t, i int32, f float, q int64, I int32*, D gslic_adam_fused*
ARGTYPES = {
    'gslic_debug_export': 'Piivvvvvvvvvvvvvvv',
    'gslic_rasterize_backward': 'Piivvvvvvvvvvvvvvvvvvvvvvvvvvvfv',
    'gslic_rasterize_backward_adam': 'PiivvvvvvvvvvvvvvvvvvvvvvvfDv',
    'gslic_rasterize_backward_camera': 'Piivvvvvvvvvvvvvvvvvvvvvvvvvvvfvvvv',
    'gslic_rasterize_backward_depth': 'Piivvvvvvvvvvvvvvvvvvvvvvvvvvvvfv',
    'gslic_rasterize_backward_depth_adam': 'PiivvvvvvvvvvvvvvvvvvvvvvvvfDv',
    'gslic_rasterize_backward_depth_camera': 'Piivvvvvvvvvvvvvvvvvvvvvvvvvvvvfvvvv',
    'gslic_rasterize_backward_rgb': 'Piivvvvvvvvvvvvvvvvvvvvvvfv',
    'gslic_rasterize_backward_rgb_payload': 'Piivvvvvvvvvvvvvvvvvvvvvvfvvv',
    'gslic_rasterize_backward_rgb_rows': 'Piivvvvvvvvvvvvvvvvvvvvvvfiiiv',
    'gslic_rasterize_forward': 'PAvAvAvAvvvvvvvvvvvvvvvvIIv',
    'gslic_rasterize_forward_capacity': 'PvzvzvzvzvvvvvvvvvvvvvvvIIvv',
    'gslic_rasterize_forward_depth': 'PAvAvAvAvvvvvvvvvvvvvvvvvIIv',
    'gslic_rasterize_forward_depth_capacity': 'PvzvzvzvzvvvvvvvvvvvvvvvvIIvv',
    'gslic_sh_grad_from_rgb': 'iiiivvvivvqv',
    'gslic_sh_grad_from_rgb_adam': 'iiiivvvivDvvqv',
    'gslic_sh_grad_from_rgb_adam_all': 'iiiivvvivqvDvvvvqv',
}


def _letters(argtypes, _lib):
    code = {ctypes.POINTER(_lib.RasterParams): "P", _lib.ALLOC_FN: "A", ctypes.c_void_p: "v", ctypes.c_size_t: "z", ctypes.c_int32: "i",
            ctypes.c_float: "f", ctypes.c_int64: "q", ctypes.POINTER(ctypes.c_int32): "I", ctypes.POINTER(_lib.AdamFused): "D"}
    return "".join(code[t] for t in argtypes)


def test_argtypes_are_what_they_were():
    _lib, _rz = _mods()
    L = _lib.lib()
    assert len(ARGTYPES) == 17
    for sym, want in ARGTYPES.items():
        assert _letters(getattr(L, sym).argtypes, _lib) == want, sym
