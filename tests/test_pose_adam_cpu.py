"""CPU-only: the two fused-Adam camera backwards (gslic_rasterize_backward_camera_adam / _depth_camera_adam) as rasterizer._backward hands them to
the library — _lib.lib replaced by a recorder, in the style of tests/test_call_marshalling_cpu.py — and every argument check of theirs and of the
Python layers above them that needs no device.  refusal_cases() is shared with tests/test_pose_adam_gpu.py."""
import ctypes

import pytest
import torch

ERR_INVALID_ARG = -1
P, W, H, M, DEG = 8, 32, 16, 3, 1
STREAM = 0x5eadbeef


def _mods():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib, rasterizer, trainer
    return _lib, rasterizer, trainer


class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, sym):
        def fn(*args):
            self.calls.append((sym, args))
            return 0
        return fn


def _addr(a):
    if a is None:
        return 0
    if isinstance(a, ctypes.c_void_p):
        return a.value or 0
    return a


def _inputs():
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype)
    t = dict(bg=z(3), xyz=z(P, 3), dc=z(P, 1, 3), sh=z(P, M, 3), sc=z(P, 3), rot=z(P, 4), view=z(4, 4), proj=z(4, 4), campos=z(3),
             radii=z(P, dtype=torch.int32), dL=z(3, H, W), dLd=z(H, W), xyz_grad=z(P, 3), m2d=z(P, 3), cam_out=z(35))
    for n in ("geom", "binning", "img", "sample"):
        t[n] = z(64, dtype=torch.uint8)
    return t


def _call(rz, t, depth, adam, **modes):
    view = (H, W, 0.5, 0.5, -1.0, 1.0, -1.0, 1.0, 1.0)
    e = torch.empty(0)
    return rz._backward(view, DEG, False, True, t["bg"], t["xyz"], t["radii"], e, t["sc"], t["rot"], e, t["view"], t["proj"], t["campos"], t["dL"],
                        t["dLd"] if depth else None, t["dc"], t["sh"], t["geom"], 5, t["binning"], t["img"], 7, t["sample"], 0.25, adam=adam, **modes)


@pytest.mark.parametrize("depth", [False, True])
def test_marshalling_of_the_two_calls(monkeypatch, depth):
    _lib, rz, _tr = _mods()
    real = _lib.lib()
    sym = "gslic_rasterize_backward_depth_camera_adam" if depth else "gslic_rasterize_backward_camera_adam"
    parent = "gslic_rasterize_backward_depth_adam" if depth else "gslic_rasterize_backward_adam"
    n_args = len(getattr(real, sym).argtypes)
    assert n_args == len(getattr(real, parent).argtypes) + 4                          # three camera outputs and dL_dmean2D
    rec = Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "current_stream_ptr", lambda: ctypes.c_void_p(STREAM))
    t = _inputs()
    adam = _lib.AdamFused()
    got = _call(rz, t, depth, adam, camera_grads=True, xyz_grad=t["xyz_grad"], mean2d_out=t["m2d"], cam_out=t["cam_out"])
    _call(rz, t, depth, adam, xyz_grad=t["xyz_grad"])
    (s_new, a_new), (s_old, a_old) = rec.calls
    assert (s_new, s_old) == (sym, parent) and len(a_new) == n_args
    n_head = len(a_old) - 2                                                           # everything up to and including lambda_erank
    assert [_addr(x) if not hasattr(x, "_obj") else "prm" for x in a_new[:n_head]] == \
           [_addr(x) if not hasattr(x, "_obj") else "prm" for x in a_old[:n_head]]   # the parent's arguments, unchanged and in its order
    prm = a_new[0]._obj
    assert (prm.P, prm.D, prm.M, prm.width, prm.height, prm.raw_params) == (P, DEG, M, W, H, 1)
    assert a_new[n_head]._obj is adam
    base = t["cam_out"].data_ptr()
    assert [_addr(x) for x in a_new[n_head + 1:]] == [base, base + 64, base + 128, t["m2d"].data_ptr(), STREAM]
    # dL_dmean3D: the xyz gradient buffer under depth, NULL without; the five other gradient pointers NULL
    six = [_addr(x) for x in a_new[n_head - 7:n_head - 1]]
    assert six == [0, t["xyz_grad"].data_ptr() if depth else 0, 0, 0, 0, 0]
    assert a_new[n_head - 1] == 0.25
    # the return value: the three camera outputs as views of cam_out
    assert [g.data_ptr() for g in got] == [base, base + 64, base + 128] and [g.numel() for g in got] == [16, 16, 3]
    # without cam_out / mean2d_out: a new 35-float tensor, a NULL dL_dmean2D
    rec.calls.clear()
    got = _call(rz, t, depth, adam, camera_grads=True, xyz_grad=t["xyz_grad"])
    a = rec.calls[0][1]
    assert _addr(a[-2]) == 0 and _addr(a[-5]) == got[0].data_ptr() and got[1].data_ptr() == got[0].data_ptr() + 64


def test_python_argument_checks(monkeypatch):
    _lib, rz, trainer = _mods()
    rec = Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "current_stream_ptr", lambda: ctypes.c_void_p(STREAM))
    t = _inputs()
    adam = _lib.AdamFused()
    with pytest.raises(ValueError, match="no grad_stats"):
        _call(rz, t, False, adam, camera_grads=True, grad_stats=_lib.GradStats())
    with pytest.raises(ValueError, match="cam_out goes with"):
        _call(rz, t, False, adam, cam_out=t["cam_out"])
    with pytest.raises(ValueError, match="cam_out goes with"):
        _call(rz, t, False, None, camera_grads=True, cam_out=t["cam_out"])
    for bad in (torch.zeros(34), torch.zeros(35, dtype=torch.float64), torch.zeros(70)[::2]):
        with pytest.raises(ValueError, match="35 contiguous float32"):
            _call(rz, t, False, adam, camera_grads=True, cam_out=bad)
    assert rec.calls == []
    # the joint step with the Adam in the backward is single-GPU only
    monkeypatch.setattr(trainer, "_dist_on", lambda: True)
    with pytest.raises(NotImplementedError, match="single-GPU only"):
        trainer.training_step_with_pose(None, None, None, None, fused_loss=object(), adam_in_backward=True)


def refusal_cases():
    """[(label, symbol, argument tuple)]: every call is refused with GSLIC_ERR_INVALID_ARG before any device work, so the made-up addresses are
    never followed (the descriptor and the parameter block are host structures)."""
    _lib, _rz, _tr = _mods()
    A = lambda k: ctypes.c_void_p(0x10000 + 0x1000 * k)   # distinct non-NULL addresses

    def args(depth, prm_kw=None, adam="ok", null=(), alias_ok=True):
        prm = _lib.RasterParams(P=P, D=DEG, M=M, width=W, height=H, tan_fovx=0.5, tan_fovy=0.5, limx_neg=-1.0, limx_pos=1.0, limy_neg=-1.0,
                                limy_pos=1.0, scale_modifier=1.0, prefiltered=0, debug=0, no_color=0, raw_params=1, tie_rank=None)
        for k, v in (prm_kw or {}).items():
            setattr(prm, k, v)
        names = ["background", "means3D", "dc", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp", "viewmatrix", "projmatrix", "cam_pos",
                 "radii", "geom", "binning", "img", "sample", "dL_dpix"] + (["dL_ddepth"] if depth else []) + \
                ["dL_dopacity", "dL_dmean3D", "dL_ddc", "dL_dsh", "dL_dscale", "dL_drot"]
        val = {n: A(i) for i, n in enumerate(names)}
        val["colors_precomp"] = val["cov3D_precomp"] = None
        for n in ("dL_dopacity", "dL_ddc", "dL_dsh", "dL_dscale", "dL_drot"):
            val[n] = None
        if not depth:
            val["dL_dmean3D"] = None
        cam = {n: A(40 + i) for i, n in enumerate(("dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos"))}
        for n in null:
            (cam if n in cam else val)[n] = None
        d = _lib.AdamFused()
        for g, n in enumerate(("means3D", "dc", "shs", None, "scales", "rotations")):
            d.param[g] = (A(60).value if n is None or not alias_ok else A(names.index(n)).value)
            d.exp_avg[g], d.exp_avg_sq[g] = A(70 + g).value, A(80 + g).value
        if adam == "null_moment":
            d.exp_avg[3] = None
        a = None if adam is None else ctypes.byref(d)
        keep = (prm, d)   # (kept alive by the tuple)
        return (ctypes.byref(prm), 5, 7) + tuple(val[n] for n in names) + (ctypes.c_float(0.0), a, cam["dL_dviewmatrix"], cam["dL_dprojmatrix"],
                                                                              cam["dL_dcampos"], None, None), keep

    cases = []
    for depth in (False, True):
        sym = "gslic_rasterize_backward_depth_camera_adam" if depth else "gslic_rasterize_backward_camera_adam"
        tag = "depth " if depth else "colour "
        for n in ("dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos"):
            cases.append((tag + "NULL " + n, sym, args(depth, null=(n,))))
        cases.append((tag + "adam NULL", sym, args(depth, adam=None)))
        cases.append((tag + "raw_params 0", sym, args(depth, prm_kw=dict(raw_params=0))))
        # what the parents refuse
        cases.append((tag + "a NULL moment", sym, args(depth, adam="null_moment")))
        cases.append((tag + "param[] not the inputs", sym, args(depth, alias_ok=False)))
        cases.append((tag + "NULL means3D", sym, args(depth, null=("means3D",))))
        cases.append((tag + "NULL dL_dpix", sym, args(depth, null=("dL_dpix",))))
        cases.append((tag + "no_color", sym, args(depth, prm_kw=dict(no_color=1))))
        cases.append((tag + "SH degree 4", sym, args(depth, prm_kw=dict(D=4))))
        cases.append((tag + "negative P", sym, args(depth, prm_kw=dict(P=-1))))
        if depth:
            cases.append((tag + "NULL dL_ddepth", sym, args(depth, null=("dL_ddepth",))))
            cases.append((tag + "NULL dL_dmean3D", sym, args(depth, null=("dL_dmean3D",))))
    return cases


def run_refusal_cases():
    _lib, _rz, _tr = _mods()
    L = _lib.lib()
    cases = refusal_cases()
    for label, sym, (a, _keep) in cases:
        rc = getattr(L, sym)(*a)
        assert rc == ERR_INVALID_ARG, (label, rc)
        assert L.gslic_last_error(), label
    return len(cases)


def test_refusals_before_any_device_work():
    assert run_refusal_cases() == 2 * 12 + 2
