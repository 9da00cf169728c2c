"""CPU-only: the argument checks of the rasterize entry points (four forwards, nine backwards) and of the three gslic_sh_grad_from_rgb*
functions — return code AND the complete gslic_last_error() text, including which check fires first when several would.

Every case returns before any device work (no case may reach a HIP call: without a GPU it would fail, not pass).  Pointers that are never
dereferenced are dummies; the params, the Adam descriptor and the two count outputs are real objects.

EXPECTED was produced by running this table against the library built from the commit BEFORE the host call path was rewritten around
ForwardCall / BackwardCall (api.hip), and is written out literally: the rewrite must not change a code, a message or the order of the checks.
A call that returns 0 leaves the error text alone; each case first provokes a known message (SENTINEL), so an untouched text is checked too."""
import ctypes

import pytest

vp = ctypes.c_void_p
SENTINEL = "bad kernel id -1"

INPUTS = ["background", "means3D", "dc", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp", "viewmatrix", "projmatrix", "cam_pos", "radii"]
FWD_INPUTS = ["background", "means3D", "dc", "shs", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp", "viewmatrix", "projmatrix",
              "cam_pos"]
BUFFERS = ["geom", "binning", "img", "sample"]
BWD_HEAD = ["prm", "R", "B"] + INPUTS + BUFFERS + ["dL_dpix"]
TEN = ["dL_dmean2D", "dL_dconic", "dL_dopacity", "dL_dcolor", "dL_dmean3D", "dL_dcov3D", "dL_ddc", "dL_dsh", "dL_dscale", "dL_drot"]
FIVE = ["dL_dopacity", "dL_dmean3D", "dL_drgb", "dL_dscale", "dL_drot"]
SIX = ["dL_dopacity", "dL_dmean3D", "dL_ddc", "dL_dsh", "dL_dscale", "dL_drot"]
CAM = ["dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos"]
ALLOCS = ["geom_alloc", "geom_ctx", "binning_alloc", "binning_ctx", "img_alloc", "img_ctx", "sample_alloc", "sample_ctx"]
CAPS = ["geom", "geom_bytes", "binning", "binning_bytes", "img", "img_bytes", "sample", "sample_bytes"]
SH_HEAD = ["P", "D", "M", "n_views", "means3D", "campos_all", "rgb_all", "input_is_ddc"]

SIGNATURES = {
    "gslic_rasterize_forward": ["prm"] + ALLOCS + FWD_INPUTS + ["out_color", "out_final_T", "radii", "num_rendered", "num_buckets", "stream"],
    "gslic_rasterize_forward_depth": ["prm"] + ALLOCS + FWD_INPUTS + ["out_color", "out_final_T", "out_depth", "radii", "num_rendered", "num_buckets",
                                                                     "stream"],
    "gslic_rasterize_forward_capacity": ["prm"] + CAPS + FWD_INPUTS + ["out_color", "out_final_T", "radii", "num_rendered", "num_buckets", "status",
                                                                      "stream"],
    "gslic_rasterize_forward_depth_capacity": ["prm"] + CAPS + FWD_INPUTS + ["out_color", "out_final_T", "out_depth", "radii", "num_rendered",
                                                                            "num_buckets", "status", "stream"],
    "gslic_rasterize_backward": BWD_HEAD + TEN + ["lambda_erank", "stream"],
    "gslic_rasterize_backward_depth": BWD_HEAD + ["dL_ddepth"] + TEN + ["lambda_erank", "stream"],
    "gslic_rasterize_backward_rgb": BWD_HEAD + FIVE + ["lambda_erank", "stream"],
    "gslic_rasterize_backward_rgb_payload": BWD_HEAD + FIVE + ["lambda_erank", "vis_out", "campos_out", "stream"],
    "gslic_rasterize_backward_rgb_rows": BWD_HEAD + FIVE + ["lambda_erank", "row_begin", "row_end", "skip_blend", "stream"],
    "gslic_rasterize_backward_adam": BWD_HEAD + SIX + ["lambda_erank", "adam", "stream"],
    "gslic_rasterize_backward_depth_adam": BWD_HEAD + ["dL_ddepth"] + SIX + ["lambda_erank", "adam", "stream"],
    "gslic_rasterize_backward_camera": BWD_HEAD + TEN + ["lambda_erank"] + CAM + ["stream"],
    "gslic_rasterize_backward_depth_camera": BWD_HEAD + ["dL_ddepth"] + TEN + ["lambda_erank"] + CAM + ["stream"],
    "gslic_sh_grad_from_rgb": SH_HEAD + ["dL_ddc", "dL_dsh", "view_stride", "stream"],
    "gslic_sh_grad_from_rgb_adam": SH_HEAD + ["visible", "adam", "dL_ddc", "dL_dsh", "view_stride", "stream"],
    "gslic_sh_grad_from_rgb_adam_all": SH_HEAD + ["vis_all", "vis_stride", "vis_out", "adam", "dL_dmean3D", "dL_dopacity", "dL_dscale", "dL_drot",
                                                  "view_stride", "stream"],
}
FORWARDS = [e for e in SIGNATURES if "forward" in e]
BACKWARDS = [e for e in SIGNATURES if "backward" in e]
SH = [e for e in SIGNATURES if "sh_grad" in e]
SCALARS = dict(R=10, B=2, lambda_erank=0.0, row_begin=0, row_end=-1, skip_blend=0, geom_bytes=1 << 30, binning_bytes=1 << 30, img_bytes=1 << 30,
               sample_bytes=1 << 30, P=128, D=1, M=3, n_views=2, input_is_ddc=0, view_stride=0, vis_stride=0, stream=None, colors_precomp=None,
               cov3D_precomp=None, geom_ctx=None, binning_ctx=None, img_ctx=None, sample_ctx=None)


def _libs():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    return _lib, _lib.lib()


_DUMMIES = {}


def _dummy(name):
    return vp(_DUMMIES.setdefault(name, 0x100000 + 4096 * len(_DUMMIES)))   # (distinct per name, never dereferenced)


def _call(entry, mutations):
    """Build the entry's complete, valid argument list (P = 128, degree 1, M = 3, 32 x 16; it would reach the device), apply the case's
    mutations ({argument or 'prm.field' or 'adam.field[i]': value}), call, return (code, error text)."""
    _l, L = _libs()
    prm = _l.RasterParams(128, 1, 3, 32, 16, 1.0, 1.0, -1.3, 1.3, -1.3, 1.3, 1.0, 0, 0, 0, 1 if "adam" in entry else 0, None)
    adam = _l.AdamFused()
    null_alloc = _l.ALLOC_FN(lambda _ctx, _n: None)
    vals = {}
    for n in SIGNATURES[entry]:
        if n in SCALARS:
            vals[n] = SCALARS[n]
        elif n == "prm":
            vals[n] = ctypes.byref(prm)
        elif n == "adam":
            vals[n] = ctypes.byref(adam)
        elif n in ("num_rendered", "num_buckets"):
            vals[n] = ctypes.byref(ctypes.c_int32(77))
        elif n.endswith("_alloc"):
            vals[n] = null_alloc
        else:
            vals[n] = _dummy(n)
    for g, n in enumerate(("means3D", "dc", "shs", "opacities", "scales", "rotations")):   # param[] aliases the inputs; moments are dummies
        adam.param[g] = _dummy(n).value
        adam.exp_avg[g], adam.exp_avg_sq[g] = _dummy(f"m{g}").value, _dummy(f"v{g}").value
    for key, v in mutations.items():
        if key.startswith("prm."):
            setattr(prm, key[4:], v)
        elif key.startswith("adam."):
            field, g = key[5:].split("[")
            getattr(adam, field)[int(g[:-1])] = v
        else:
            assert key in vals, (entry, key)
            vals[key] = _l.ALLOC_FN() if (v is None and key.endswith("_alloc")) else v   # (a NULL function pointer)
    assert L.gslic_profile_get(-1, None, None) == -1 and L.gslic_last_error().decode() == SENTINEL
    rc = getattr(L, entry)(*[vals[n] for n in SIGNATURES[entry]])
    return rc, L.gslic_last_error().decode()


def _own_required(entry):
    """The pointers this entry itself requires (beyond the shared implementation's), in the order its checks test them."""
    own = []
    if "camera" in entry:
        own.append("dL_dprojmatrix")
    if "rgb" in entry:
        own.append("dL_drgb")
    if "adam" in entry:
        own.append("adam")
    if "depth" in entry:
        own.append("dL_ddepth")
    if entry in ("gslic_rasterize_backward_depth_adam", "gslic_rasterize_backward_depth_camera"):
        own.append("dL_dmean3D")
    return own


def _cases():
    c = []
    add = lambda entry, name, **m: c.append((entry, name, {k.replace("__", "."): v for k, v in m.items()}))
    for e in FORWARDS + BACKWARDS:
        cam, depth = "camera" in e, "depth" in e
        add(e, "null_params", prm=None)
        add(e, "degree4", prm__D=4)
        add(e, "M_too_small", prm__D=2)
        add(e, "bad_width", prm__width=0)
        if not cam:   # (the camera backwards zero-fill their outputs on P == 0: device work)
            add(e, "P0", prm__P=0)
            add(e, "P0_no_color", prm__P=0, prm__no_color=1)
            add(e, "P0_precomp", prm__P=0, colors_precomp=_dummy("cp"))
        add(e, "P0_degree4", prm__P=0, prm__D=4) if e != "gslic_rasterize_backward_camera" else None
        add(e, "no_color", **({"prm__no_color": 1} if (depth or e in BACKWARDS) else {"prm__no_color": 1, "means3D": None}))
        add(e, "precomp", cov3D_precomp=_dummy("cov"))
        add(e, "precomp_no_color", colors_precomp=_dummy("cp"), prm__no_color=1, means3D=None)
        add(e, "means3D_null", means3D=None)
        add(e, "shs_null_M3", shs=None)
    for e in FORWARDS:
        add(e, "num_rendered_null", num_rendered=None)
        add(e, "num_rendered_null_degree4", num_rendered=None, prm__D=4)
        add(e, "num_buckets_null_P0", num_buckets=None, prm__P=0)
        add(e, "out_color_null", out_color=None)
        add(e, "radii_null", radii=None)
        if "depth" in e:
            add(e, "out_depth_null", out_depth=None)
            add(e, "out_depth_null_no_color", out_depth=None, prm__no_color=1)
            add(e, "out_depth_null_precomp", out_depth=None, colors_precomp=_dummy("cp"))
            add(e, "out_depth_null_P0", out_depth=None, prm__P=0)
        if "capacity" in e:
            add(e, "geom_too_small", geom_bytes=16)
            add(e, "img_too_small", img_bytes=16)
            add(e, "binning_null", binning=None)
            add(e, "status_null", status=None)
            add(e, "geom_too_small_means3D_null", geom_bytes=16, means3D=None)
        else:
            add(e, "allocator_null", img_alloc=None)
            add(e, "allocator_null_means3D_null", geom_alloc=None, means3D=None)
            add(e, "allocator_returns_null")
    for e in BACKWARDS:
        own = _own_required(e)
        add(e, "negative_R", R=-1)
        add(e, "negative_B", B=-1)
        add(e, "negative_R_no_color", R=-1, prm__no_color=1)
        add(e, "negative_B_geom_null", B=-1, geom=None)
        add(e, "dL_dpix_null", dL_dpix=None)
        add(e, "sample_null_grad_null", sample=None, dL_dopacity=None)
        if "adam" not in e:   # (with the update inside the backward no gradient output is required)
            add(e, "dL_dopacity_null", dL_dopacity=None)
            add(e, "dL_dopacity_null_bad_rows_or_precomp", dL_dopacity=None, **({"row_begin": 32} if "rows" in e else {"cov3D_precomp": _dummy("cov")}))
        add(e, "dL_drot_null_means3D_null", dL_drot=None, means3D=None)
        for o in own:
            add(e, f"{o}_null", **{o: None})
            add(e, f"{o}_null_null_params", **{o: None, "prm": None})
            add(e, f"{o}_null_degree4", **{o: None, "prm__D": 4})
            add(e, f"{o}_null_no_color", **{o: None, "prm__no_color": 1})
            add(e, f"{o}_null_negative_R", **{o: None, "R": -1})
            if "camera" not in e or o == "dL_dprojmatrix":
                add(e, f"{o}_null_P0", **{o: None, "prm__P": 0})
        for a, b in zip(own, own[1:]):
            add(e, f"{a}_null_{b}_null", **{a: None, b: None})
        if "camera" in e:
            add(e, "dL_dviewmatrix_null", dL_dviewmatrix=None)
            add(e, "dL_dcampos_null_null_params", dL_dcampos=None, prm=None)
        if "rows" in e:
            add(e, "row_begin_not_multiple_of_64", row_begin=32)
            add(e, "row_end_past_P", row_end=129)
            add(e, "row_begin_past_row_end", row_begin=128, row_end=64)
            add(e, "row_begin_negative", row_begin=-64)
            add(e, "row_begin_past_P_default_end", row_begin=192)
            add(e, "rows_negative_R", row_begin=32, R=-1)
            add(e, "rows_dL_drgb_null", row_begin=32, dL_drgb=None)
            add(e, "rows_dL_dscale_null", row_end=200, dL_dscale=None)
        if "adam" in e:
            add(e, "adam_without_raw_params", prm__raw_params=0)
            add(e, "adam_without_raw_params_group_null", prm__raw_params=0, **{"adam__param[3]": None})
            add(e, "adam_group3_param_null", **{"adam__param[3]": None})
            add(e, "adam_group0_exp_avg_null", **{"adam__exp_avg[0]": None})
            add(e, "adam_group5_exp_avg_sq_null", **{"adam__exp_avg_sq[5]": None})
            add(e, "adam_group2_null_M0", prm__D=0, prm__M=0, shs=None, **{"adam__param[2]": None, "adam__param[4]": 4096})
            add(e, "adam_param0_not_aliasing", **{"adam__param[0]": 4096})
            add(e, "adam_param2_not_aliasing", **{"adam__param[2]": 4096})
            add(e, "adam_param5_not_aliasing_group1_null", **{"adam__param[5]": 4096, "adam__exp_avg[1]": None})
            add(e, "adam_not_aliasing_negative_R", R=-1, **{"adam__param[4]": 4096})
            add(e, "adam_not_aliasing_means3D_null", means3D=None, **{"adam__param[0]": 4096})
    for e in SH:
        add(e, "view_stride_negative", view_stride=-1)
        add(e, "view_stride_too_small", view_stride=383)
        add(e, "view_stride_negative_degree4", view_stride=-1, D=4)
        add(e, "degree4", D=4)
        add(e, "P_negative", P=-1)
        add(e, "M_negative", M=-1)
        add(e, "n_views_0", n_views=0)
        add(e, "n_views_0_means3D_null", n_views=0, means3D=None)
        add(e, "P0", P=0)
        add(e, "P0_means3D_null", P=0, means3D=None)
        add(e, "P0_degree4", P=0, D=4)
        add(e, "means3D_null", means3D=None)
        add(e, "rgb_all_null", rgb_all=None)
        if e == "gslic_sh_grad_from_rgb":
            add(e, "dL_ddc_null", dL_ddc=None)
            add(e, "dL_dsh_null", dL_dsh=None)
            add(e, "dL_dsh_null_M0_view_stride_negative", dL_dsh=None, M=0, view_stride=-5)
        else:
            add(e, "adam_null", adam=None)
            add(e, "adam_null_P0", adam=None, P=0)
            add(e, "adam_group1_param_null", **{"adam__param[1]": None})
            add(e, "adam_group2_exp_avg_null", **{"adam__exp_avg[2]": None})
            add(e, "adam_group1_null_means3D_null", means3D=None, **{"adam__param[1]": None})
        if e == "gslic_sh_grad_from_rgb_adam":
            add(e, "visible_null", visible=None)
        if e == "gslic_sh_grad_from_rgb_adam_all":
            add(e, "vis_all_null", vis_all=None)
            add(e, "vis_stride_negative", vis_stride=-1)
            add(e, "vis_stride_too_small", vis_stride=127)
            add(e, "vis_stride_too_small_view_stride_negative", vis_stride=127, view_stride=-1)
            add(e, "small_gradients_partial", dL_dscale=None)
            add(e, "small_gradients_partial_group_null", dL_drot=None, **{"adam__param[1]": None})
            add(e, "adam_group0_null_with_small", **{"adam__param[0]": None})
            add(e, "adam_group5_null_with_small", **{"adam__exp_avg_sq[5]": None})
            add(e, "adam_group1_null_without_small", dL_dmean3D=None, dL_dopacity=None, dL_dscale=None, dL_drot=None, **{"adam__param[1]": None})
    return [x for x in c if x is not None]


CASES = _cases()

# (code, gslic_last_error()) of every case on the library of the parent commit; see the module docstring
EXPECTED = {
    'gslic_rasterize_forward/null_params': (-1, 'params is NULL'),
    'gslic_rasterize_forward/degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_forward/M_too_small': (-1, 'M=3 rest coefficients cannot hold SH degree 2'),
    'gslic_rasterize_forward/bad_width': (-1, 'bad sizes P=128 W=0 H=16'),
    'gslic_rasterize_forward/P0': (0, 'bad kernel id -1'),
    'gslic_rasterize_forward/P0_no_color': (0, 'bad kernel id -1'),
    'gslic_rasterize_forward/P0_precomp': (0, 'bad kernel id -1'),
    'gslic_rasterize_forward/P0_degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_forward/no_color': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_forward/precomp': (-2, 'colors_precomp / cov3D_precomp are not supported (the reference host always passes empty tensors)'),
    'gslic_rasterize_forward/precomp_no_color': (-2, 'colors_precomp / cov3D_precomp are not supported (the reference host always passes empty tensors)'),
    'gslic_rasterize_forward/means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_forward/shs_null_M3': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_forward_depth/null_params': (-1, 'params is NULL'),
    'gslic_rasterize_forward_depth/degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_forward_depth/M_too_small': (-1, 'M=3 rest coefficients cannot hold SH degree 2'),
    'gslic_rasterize_forward_depth/bad_width': (-1, 'bad sizes P=128 W=0 H=16'),
    'gslic_rasterize_forward_depth/P0': (0, 'bad kernel id -1'),
    'gslic_rasterize_forward_depth/P0_no_color': (0, 'bad kernel id -1'),
    'gslic_rasterize_forward_depth/P0_precomp': (0, 'bad kernel id -1'),
    'gslic_rasterize_forward_depth/P0_degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_forward_depth/no_color': (-1, 'depth forward: no_color = 1 (the depth is blended with the colour and needs its checkpoints)'),
    'gslic_rasterize_forward_depth/precomp': (-2, 'colors_precomp / cov3D_precomp are not supported (the reference host always passes empty tensors)'),
    'gslic_rasterize_forward_depth/precomp_no_color': (-1, 'depth forward: no_color = 1 (the depth is blended with the colour and needs its checkpoints)'),
    'gslic_rasterize_forward_depth/means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_forward_depth/shs_null_M3': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_forward_capacity/null_params': (-1, 'params is NULL'),
    'gslic_rasterize_forward_capacity/degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_forward_capacity/M_too_small': (-1, 'M=3 rest coefficients cannot hold SH degree 2'),
    'gslic_rasterize_forward_capacity/bad_width': (-1, 'bad sizes P=128 W=0 H=16'),
    'gslic_rasterize_forward_capacity/P0': (0, 'bad kernel id -1'),
    'gslic_rasterize_forward_capacity/P0_no_color': (0, 'bad kernel id -1'),
    'gslic_rasterize_forward_capacity/P0_precomp': (0, 'bad kernel id -1'),
    'gslic_rasterize_forward_capacity/P0_degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_forward_capacity/no_color': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_forward_capacity/precomp': (-2, 'colors_precomp / cov3D_precomp are not supported (the reference host always passes empty tensors)'),
    'gslic_rasterize_forward_capacity/precomp_no_color': (-2, 'colors_precomp / cov3D_precomp are not supported (the reference host always passes empty tensors)'),
    'gslic_rasterize_forward_capacity/means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_forward_capacity/shs_null_M3': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_forward_depth_capacity/null_params': (-1, 'params is NULL'),
    'gslic_rasterize_forward_depth_capacity/degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_forward_depth_capacity/M_too_small': (-1, 'M=3 rest coefficients cannot hold SH degree 2'),
    'gslic_rasterize_forward_depth_capacity/bad_width': (-1, 'bad sizes P=128 W=0 H=16'),
    'gslic_rasterize_forward_depth_capacity/P0': (0, 'bad kernel id -1'),
    'gslic_rasterize_forward_depth_capacity/P0_no_color': (0, 'bad kernel id -1'),
    'gslic_rasterize_forward_depth_capacity/P0_precomp': (0, 'bad kernel id -1'),
    'gslic_rasterize_forward_depth_capacity/P0_degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_forward_depth_capacity/no_color': (-1, 'depth forward: no_color = 1 (the depth is blended with the colour and needs its checkpoints)'),
    'gslic_rasterize_forward_depth_capacity/precomp': (-2, 'colors_precomp / cov3D_precomp are not supported (the reference host always passes empty tensors)'),
    'gslic_rasterize_forward_depth_capacity/precomp_no_color': (-1, 'depth forward: no_color = 1 (the depth is blended with the colour and needs its checkpoints)'),
    'gslic_rasterize_forward_depth_capacity/means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_forward_depth_capacity/shs_null_M3': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward/null_params': (-1, 'params is NULL'),
    'gslic_rasterize_backward/degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_backward/M_too_small': (-1, 'M=3 rest coefficients cannot hold SH degree 2'),
    'gslic_rasterize_backward/bad_width': (-1, 'bad sizes P=128 W=0 H=16'),
    'gslic_rasterize_backward/P0': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward/P0_no_color': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward/P0_precomp': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward/P0_degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_backward/no_color': (-1, 'backward of a no_color forward is undefined (no checkpoints were stored)'),
    'gslic_rasterize_backward/precomp': (-2, 'colors_precomp / cov3D_precomp are not supported'),
    'gslic_rasterize_backward/precomp_no_color': (-2, 'colors_precomp / cov3D_precomp are not supported'),
    'gslic_rasterize_backward/means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward/shs_null_M3': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_depth/null_params': (-1, 'params is NULL'),
    'gslic_rasterize_backward_depth/degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_backward_depth/M_too_small': (-1, 'M=3 rest coefficients cannot hold SH degree 2'),
    'gslic_rasterize_backward_depth/bad_width': (-1, 'bad sizes P=128 W=0 H=16'),
    'gslic_rasterize_backward_depth/P0': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward_depth/P0_no_color': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward_depth/P0_precomp': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward_depth/P0_degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_backward_depth/no_color': (-1, 'depth backward: no_color = 1 (no depth forward renders without colour)'),
    'gslic_rasterize_backward_depth/precomp': (-2, 'colors_precomp / cov3D_precomp are not supported'),
    'gslic_rasterize_backward_depth/precomp_no_color': (-1, 'depth backward: no_color = 1 (no depth forward renders without colour)'),
    'gslic_rasterize_backward_depth/means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_depth/shs_null_M3': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_rgb/null_params': (-1, 'params is NULL'),
    'gslic_rasterize_backward_rgb/degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_backward_rgb/M_too_small': (-1, 'M=3 rest coefficients cannot hold SH degree 2'),
    'gslic_rasterize_backward_rgb/bad_width': (-1, 'bad sizes P=128 W=0 H=16'),
    'gslic_rasterize_backward_rgb/P0': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward_rgb/P0_no_color': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward_rgb/P0_precomp': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward_rgb/P0_degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_backward_rgb/no_color': (-1, 'backward of a no_color forward is undefined (no checkpoints were stored)'),
    'gslic_rasterize_backward_rgb/precomp': (-2, 'colors_precomp / cov3D_precomp are not supported'),
    'gslic_rasterize_backward_rgb/precomp_no_color': (-2, 'colors_precomp / cov3D_precomp are not supported'),
    'gslic_rasterize_backward_rgb/means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_rgb/shs_null_M3': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_rgb_payload/null_params': (-1, 'params is NULL'),
    'gslic_rasterize_backward_rgb_payload/degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_backward_rgb_payload/M_too_small': (-1, 'M=3 rest coefficients cannot hold SH degree 2'),
    'gslic_rasterize_backward_rgb_payload/bad_width': (-1, 'bad sizes P=128 W=0 H=16'),
    'gslic_rasterize_backward_rgb_payload/P0': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward_rgb_payload/P0_no_color': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward_rgb_payload/P0_precomp': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward_rgb_payload/P0_degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_backward_rgb_payload/no_color': (-1, 'backward of a no_color forward is undefined (no checkpoints were stored)'),
    'gslic_rasterize_backward_rgb_payload/precomp': (-2, 'colors_precomp / cov3D_precomp are not supported'),
    'gslic_rasterize_backward_rgb_payload/precomp_no_color': (-2, 'colors_precomp / cov3D_precomp are not supported'),
    'gslic_rasterize_backward_rgb_payload/means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_rgb_payload/shs_null_M3': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_rgb_rows/null_params': (-1, 'params is NULL'),
    'gslic_rasterize_backward_rgb_rows/degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_backward_rgb_rows/M_too_small': (-1, 'M=3 rest coefficients cannot hold SH degree 2'),
    'gslic_rasterize_backward_rgb_rows/bad_width': (-1, 'bad sizes P=128 W=0 H=16'),
    'gslic_rasterize_backward_rgb_rows/P0': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward_rgb_rows/P0_no_color': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward_rgb_rows/P0_precomp': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward_rgb_rows/P0_degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_backward_rgb_rows/no_color': (-1, 'backward of a no_color forward is undefined (no checkpoints were stored)'),
    'gslic_rasterize_backward_rgb_rows/precomp': (-2, 'colors_precomp / cov3D_precomp are not supported'),
    'gslic_rasterize_backward_rgb_rows/precomp_no_color': (-2, 'colors_precomp / cov3D_precomp are not supported'),
    'gslic_rasterize_backward_rgb_rows/means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_rgb_rows/shs_null_M3': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_adam/null_params': (-1, 'params is NULL'),
    'gslic_rasterize_backward_adam/degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_backward_adam/M_too_small': (-1, 'M=3 rest coefficients cannot hold SH degree 2'),
    'gslic_rasterize_backward_adam/bad_width': (-1, 'bad sizes P=128 W=0 H=16'),
    'gslic_rasterize_backward_adam/P0': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward_adam/P0_no_color': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward_adam/P0_precomp': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward_adam/P0_degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_backward_adam/no_color': (-1, 'backward of a no_color forward is undefined (no checkpoints were stored)'),
    'gslic_rasterize_backward_adam/precomp': (-2, 'colors_precomp / cov3D_precomp are not supported'),
    'gslic_rasterize_backward_adam/precomp_no_color': (-2, 'colors_precomp / cov3D_precomp are not supported'),
    'gslic_rasterize_backward_adam/means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_adam/shs_null_M3': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_depth_adam/null_params': (-1, 'params is NULL'),
    'gslic_rasterize_backward_depth_adam/degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_backward_depth_adam/M_too_small': (-1, 'M=3 rest coefficients cannot hold SH degree 2'),
    'gslic_rasterize_backward_depth_adam/bad_width': (-1, 'bad sizes P=128 W=0 H=16'),
    'gslic_rasterize_backward_depth_adam/P0': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward_depth_adam/P0_no_color': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward_depth_adam/P0_precomp': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward_depth_adam/P0_degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_backward_depth_adam/no_color': (-1, 'depth backward: no_color = 1 (no depth forward renders without colour)'),
    'gslic_rasterize_backward_depth_adam/precomp': (-2, 'colors_precomp / cov3D_precomp are not supported'),
    'gslic_rasterize_backward_depth_adam/precomp_no_color': (-1, 'depth backward: no_color = 1 (no depth forward renders without colour)'),
    'gslic_rasterize_backward_depth_adam/means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_depth_adam/shs_null_M3': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_camera/null_params': (-1, 'params is NULL'),
    'gslic_rasterize_backward_camera/degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_backward_camera/M_too_small': (-1, 'M=3 rest coefficients cannot hold SH degree 2'),
    'gslic_rasterize_backward_camera/bad_width': (-1, 'bad sizes P=128 W=0 H=16'),
    'gslic_rasterize_backward_camera/no_color': (-1, 'backward of a no_color forward is undefined (no checkpoints were stored)'),
    'gslic_rasterize_backward_camera/precomp': (-2, 'colors_precomp / cov3D_precomp are not supported'),
    'gslic_rasterize_backward_camera/precomp_no_color': (-2, 'colors_precomp / cov3D_precomp are not supported'),
    'gslic_rasterize_backward_camera/means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_camera/shs_null_M3': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_depth_camera/null_params': (-1, 'params is NULL'),
    'gslic_rasterize_backward_depth_camera/degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_backward_depth_camera/M_too_small': (-1, 'M=3 rest coefficients cannot hold SH degree 2'),
    'gslic_rasterize_backward_depth_camera/bad_width': (-1, 'bad sizes P=128 W=0 H=16'),
    'gslic_rasterize_backward_depth_camera/P0_degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_backward_depth_camera/no_color': (-1, 'depth backward: no_color = 1 (no depth forward renders without colour)'),
    'gslic_rasterize_backward_depth_camera/precomp': (-2, 'colors_precomp / cov3D_precomp are not supported'),
    'gslic_rasterize_backward_depth_camera/precomp_no_color': (-1, 'depth backward: no_color = 1 (no depth forward renders without colour)'),
    'gslic_rasterize_backward_depth_camera/means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_depth_camera/shs_null_M3': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_forward/num_rendered_null': (-1, 'num_rendered / num_buckets is NULL'),
    'gslic_rasterize_forward/num_rendered_null_degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_forward/num_buckets_null_P0': (-1, 'num_rendered / num_buckets is NULL'),
    'gslic_rasterize_forward/out_color_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_forward/radii_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_forward/allocator_null': (-1, 'allocator callback is NULL'),
    'gslic_rasterize_forward/allocator_null_means3D_null': (-1, 'allocator callback is NULL'),
    'gslic_rasterize_forward/allocator_returns_null': (-3, 'geometry allocator returned NULL for 9472 bytes'),
    'gslic_rasterize_forward_depth/num_rendered_null': (-1, 'num_rendered / num_buckets is NULL'),
    'gslic_rasterize_forward_depth/num_rendered_null_degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_forward_depth/num_buckets_null_P0': (-1, 'num_rendered / num_buckets is NULL'),
    'gslic_rasterize_forward_depth/out_color_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_forward_depth/radii_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_forward_depth/out_depth_null': (-1, 'depth forward: out_depth is NULL'),
    'gslic_rasterize_forward_depth/out_depth_null_no_color': (-1, 'depth forward: no_color = 1 (the depth is blended with the colour and needs its checkpoints)'),
    'gslic_rasterize_forward_depth/out_depth_null_precomp': (-1, 'depth forward: out_depth is NULL'),
    'gslic_rasterize_forward_depth/out_depth_null_P0': (0, 'bad kernel id -1'),
    'gslic_rasterize_forward_depth/allocator_null': (-1, 'allocator callback is NULL'),
    'gslic_rasterize_forward_depth/allocator_null_means3D_null': (-1, 'allocator callback is NULL'),
    'gslic_rasterize_forward_depth/allocator_returns_null': (-3, 'geometry allocator returned NULL for 9472 bytes'),
    'gslic_rasterize_forward_capacity/num_rendered_null': (-1, 'num_rendered / num_buckets is NULL'),
    'gslic_rasterize_forward_capacity/num_rendered_null_degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_forward_capacity/num_buckets_null_P0': (-1, 'num_rendered / num_buckets is NULL'),
    'gslic_rasterize_forward_capacity/out_color_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_forward_capacity/radii_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_forward_capacity/geom_too_small': (-1, 'capacity mode: geometry / image buffer too small (need 9472 / 9216 bytes) or a NULL buffer'),
    'gslic_rasterize_forward_capacity/img_too_small': (-1, 'capacity mode: geometry / image buffer too small (need 9472 / 9216 bytes) or a NULL buffer'),
    'gslic_rasterize_forward_capacity/binning_null': (-1, 'capacity mode: geometry / image buffer too small (need 9472 / 9216 bytes) or a NULL buffer'),
    'gslic_rasterize_forward_capacity/status_null': (-1, 'capacity mode: geometry / image buffer too small (need 9472 / 9216 bytes) or a NULL buffer'),
    'gslic_rasterize_forward_capacity/geom_too_small_means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_forward_depth_capacity/num_rendered_null': (-1, 'num_rendered / num_buckets is NULL'),
    'gslic_rasterize_forward_depth_capacity/num_rendered_null_degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_forward_depth_capacity/num_buckets_null_P0': (-1, 'num_rendered / num_buckets is NULL'),
    'gslic_rasterize_forward_depth_capacity/out_color_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_forward_depth_capacity/radii_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_forward_depth_capacity/out_depth_null': (-1, 'depth forward: out_depth is NULL'),
    'gslic_rasterize_forward_depth_capacity/out_depth_null_no_color': (-1, 'depth forward: no_color = 1 (the depth is blended with the colour and needs its checkpoints)'),
    'gslic_rasterize_forward_depth_capacity/out_depth_null_precomp': (-1, 'depth forward: out_depth is NULL'),
    'gslic_rasterize_forward_depth_capacity/out_depth_null_P0': (0, 'bad kernel id -1'),
    'gslic_rasterize_forward_depth_capacity/geom_too_small': (-1, 'capacity mode: geometry / image buffer too small (need 9472 / 11264 bytes) or a NULL buffer'),
    'gslic_rasterize_forward_depth_capacity/img_too_small': (-1, 'capacity mode: geometry / image buffer too small (need 9472 / 11264 bytes) or a NULL buffer'),
    'gslic_rasterize_forward_depth_capacity/binning_null': (-1, 'capacity mode: geometry / image buffer too small (need 9472 / 11264 bytes) or a NULL buffer'),
    'gslic_rasterize_forward_depth_capacity/status_null': (-1, 'capacity mode: geometry / image buffer too small (need 9472 / 11264 bytes) or a NULL buffer'),
    'gslic_rasterize_forward_depth_capacity/geom_too_small_means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward/negative_R': (-1, 'negative R / B'),
    'gslic_rasterize_backward/negative_B': (-1, 'negative R / B'),
    'gslic_rasterize_backward/negative_R_no_color': (-1, 'backward of a no_color forward is undefined (no checkpoints were stored)'),
    'gslic_rasterize_backward/negative_B_geom_null': (-1, 'negative R / B'),
    'gslic_rasterize_backward/dL_dpix_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward/sample_null_grad_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward/dL_dopacity_null': (-1, 'required gradient output pointer is NULL'),
    'gslic_rasterize_backward/dL_dopacity_null_bad_rows_or_precomp': (-2, 'colors_precomp / cov3D_precomp are not supported'),
    'gslic_rasterize_backward/dL_drot_null_means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_depth/negative_R': (-1, 'negative R / B'),
    'gslic_rasterize_backward_depth/negative_B': (-1, 'negative R / B'),
    'gslic_rasterize_backward_depth/negative_R_no_color': (-1, 'depth backward: no_color = 1 (no depth forward renders without colour)'),
    'gslic_rasterize_backward_depth/negative_B_geom_null': (-1, 'negative R / B'),
    'gslic_rasterize_backward_depth/dL_dpix_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_depth/sample_null_grad_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_depth/dL_dopacity_null': (-1, 'required gradient output pointer is NULL'),
    'gslic_rasterize_backward_depth/dL_dopacity_null_bad_rows_or_precomp': (-2, 'colors_precomp / cov3D_precomp are not supported'),
    'gslic_rasterize_backward_depth/dL_drot_null_means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_depth/dL_ddepth_null': (-1, 'depth backward: dL_ddepth is NULL (gslic_rasterize_backward is the colour-only backward)'),
    'gslic_rasterize_backward_depth/dL_ddepth_null_null_params': (-1, 'params is NULL'),
    'gslic_rasterize_backward_depth/dL_ddepth_null_degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_backward_depth/dL_ddepth_null_no_color': (-1, 'depth backward: no_color = 1 (no depth forward renders without colour)'),
    'gslic_rasterize_backward_depth/dL_ddepth_null_negative_R': (-1, 'depth backward: dL_ddepth is NULL (gslic_rasterize_backward is the colour-only backward)'),
    'gslic_rasterize_backward_depth/dL_ddepth_null_P0': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward_rgb/negative_R': (-1, 'negative R / B'),
    'gslic_rasterize_backward_rgb/negative_B': (-1, 'negative R / B'),
    'gslic_rasterize_backward_rgb/negative_R_no_color': (-1, 'backward of a no_color forward is undefined (no checkpoints were stored)'),
    'gslic_rasterize_backward_rgb/negative_B_geom_null': (-1, 'negative R / B'),
    'gslic_rasterize_backward_rgb/dL_dpix_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_rgb/sample_null_grad_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_rgb/dL_dopacity_null': (-1, 'dL_drgb mode: dL_ddc / dL_dsh / adam must be NULL, the four other parameter gradients are required'),
    'gslic_rasterize_backward_rgb/dL_dopacity_null_bad_rows_or_precomp': (-2, 'colors_precomp / cov3D_precomp are not supported'),
    'gslic_rasterize_backward_rgb/dL_drot_null_means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_rgb/dL_drgb_null': (-1, 'gslic_rasterize_backward_rgb: dL_drgb is NULL'),
    'gslic_rasterize_backward_rgb/dL_drgb_null_null_params': (-1, 'gslic_rasterize_backward_rgb: dL_drgb is NULL'),
    'gslic_rasterize_backward_rgb/dL_drgb_null_degree4': (-1, 'gslic_rasterize_backward_rgb: dL_drgb is NULL'),
    'gslic_rasterize_backward_rgb/dL_drgb_null_no_color': (-1, 'gslic_rasterize_backward_rgb: dL_drgb is NULL'),
    'gslic_rasterize_backward_rgb/dL_drgb_null_negative_R': (-1, 'gslic_rasterize_backward_rgb: dL_drgb is NULL'),
    'gslic_rasterize_backward_rgb/dL_drgb_null_P0': (-1, 'gslic_rasterize_backward_rgb: dL_drgb is NULL'),
    'gslic_rasterize_backward_rgb_payload/negative_R': (-1, 'negative R / B'),
    'gslic_rasterize_backward_rgb_payload/negative_B': (-1, 'negative R / B'),
    'gslic_rasterize_backward_rgb_payload/negative_R_no_color': (-1, 'backward of a no_color forward is undefined (no checkpoints were stored)'),
    'gslic_rasterize_backward_rgb_payload/negative_B_geom_null': (-1, 'negative R / B'),
    'gslic_rasterize_backward_rgb_payload/dL_dpix_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_rgb_payload/sample_null_grad_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_rgb_payload/dL_dopacity_null': (-1, 'dL_drgb mode: dL_ddc / dL_dsh / adam must be NULL, the four other parameter gradients are required'),
    'gslic_rasterize_backward_rgb_payload/dL_dopacity_null_bad_rows_or_precomp': (-2, 'colors_precomp / cov3D_precomp are not supported'),
    'gslic_rasterize_backward_rgb_payload/dL_drot_null_means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_rgb_payload/dL_drgb_null': (-1, 'gslic_rasterize_backward_rgb_payload: dL_drgb is NULL'),
    'gslic_rasterize_backward_rgb_payload/dL_drgb_null_null_params': (-1, 'gslic_rasterize_backward_rgb_payload: dL_drgb is NULL'),
    'gslic_rasterize_backward_rgb_payload/dL_drgb_null_degree4': (-1, 'gslic_rasterize_backward_rgb_payload: dL_drgb is NULL'),
    'gslic_rasterize_backward_rgb_payload/dL_drgb_null_no_color': (-1, 'gslic_rasterize_backward_rgb_payload: dL_drgb is NULL'),
    'gslic_rasterize_backward_rgb_payload/dL_drgb_null_negative_R': (-1, 'gslic_rasterize_backward_rgb_payload: dL_drgb is NULL'),
    'gslic_rasterize_backward_rgb_payload/dL_drgb_null_P0': (-1, 'gslic_rasterize_backward_rgb_payload: dL_drgb is NULL'),
    'gslic_rasterize_backward_rgb_rows/negative_R': (-1, 'negative R / B'),
    'gslic_rasterize_backward_rgb_rows/negative_B': (-1, 'negative R / B'),
    'gslic_rasterize_backward_rgb_rows/negative_R_no_color': (-1, 'backward of a no_color forward is undefined (no checkpoints were stored)'),
    'gslic_rasterize_backward_rgb_rows/negative_B_geom_null': (-1, 'negative R / B'),
    'gslic_rasterize_backward_rgb_rows/dL_dpix_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_rgb_rows/sample_null_grad_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_rgb_rows/dL_dopacity_null': (-1, 'dL_drgb mode: dL_ddc / dL_dsh / adam must be NULL, the four other parameter gradients are required'),
    'gslic_rasterize_backward_rgb_rows/dL_dopacity_null_bad_rows_or_precomp': (-1, 'dL_drgb mode: dL_ddc / dL_dsh / adam must be NULL, the four other parameter gradients are required'),
    'gslic_rasterize_backward_rgb_rows/dL_drot_null_means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_rgb_rows/dL_drgb_null': (-1, 'gslic_rasterize_backward_rgb_rows: dL_drgb is NULL'),
    'gslic_rasterize_backward_rgb_rows/dL_drgb_null_null_params': (-1, 'gslic_rasterize_backward_rgb_rows: dL_drgb is NULL'),
    'gslic_rasterize_backward_rgb_rows/dL_drgb_null_degree4': (-1, 'gslic_rasterize_backward_rgb_rows: dL_drgb is NULL'),
    'gslic_rasterize_backward_rgb_rows/dL_drgb_null_no_color': (-1, 'gslic_rasterize_backward_rgb_rows: dL_drgb is NULL'),
    'gslic_rasterize_backward_rgb_rows/dL_drgb_null_negative_R': (-1, 'gslic_rasterize_backward_rgb_rows: dL_drgb is NULL'),
    'gslic_rasterize_backward_rgb_rows/dL_drgb_null_P0': (-1, 'gslic_rasterize_backward_rgb_rows: dL_drgb is NULL'),
    'gslic_rasterize_backward_rgb_rows/row_begin_not_multiple_of_64': (-1, 'row range [32, 128) of 128 Gaussians (row_begin must be a multiple of 64)'),
    'gslic_rasterize_backward_rgb_rows/row_end_past_P': (-1, 'row range [0, 129) of 128 Gaussians (row_begin must be a multiple of 64)'),
    'gslic_rasterize_backward_rgb_rows/row_begin_past_row_end': (-1, 'row range [128, 64) of 128 Gaussians (row_begin must be a multiple of 64)'),
    'gslic_rasterize_backward_rgb_rows/row_begin_negative': (-1, 'row range [-64, 128) of 128 Gaussians (row_begin must be a multiple of 64)'),
    'gslic_rasterize_backward_rgb_rows/row_begin_past_P_default_end': (-1, 'row range [192, 128) of 128 Gaussians (row_begin must be a multiple of 64)'),
    'gslic_rasterize_backward_rgb_rows/rows_negative_R': (-1, 'negative R / B'),
    'gslic_rasterize_backward_rgb_rows/rows_dL_drgb_null': (-1, 'gslic_rasterize_backward_rgb_rows: dL_drgb is NULL'),
    'gslic_rasterize_backward_rgb_rows/rows_dL_dscale_null': (-1, 'dL_drgb mode: dL_ddc / dL_dsh / adam must be NULL, the four other parameter gradients are required'),
    'gslic_rasterize_backward_adam/negative_R': (-1, 'negative R / B'),
    'gslic_rasterize_backward_adam/negative_B': (-1, 'negative R / B'),
    'gslic_rasterize_backward_adam/negative_R_no_color': (-1, 'backward of a no_color forward is undefined (no checkpoints were stored)'),
    'gslic_rasterize_backward_adam/negative_B_geom_null': (-1, 'negative R / B'),
    'gslic_rasterize_backward_adam/dL_dpix_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_adam/sample_null_grad_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_adam/dL_drot_null_means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_adam/adam_null': (-1, 'gslic_rasterize_backward_adam: adam descriptor is NULL'),
    'gslic_rasterize_backward_adam/adam_null_null_params': (-1, 'gslic_rasterize_backward_adam: adam descriptor is NULL'),
    'gslic_rasterize_backward_adam/adam_null_degree4': (-1, 'gslic_rasterize_backward_adam: adam descriptor is NULL'),
    'gslic_rasterize_backward_adam/adam_null_no_color': (-1, 'gslic_rasterize_backward_adam: adam descriptor is NULL'),
    'gslic_rasterize_backward_adam/adam_null_negative_R': (-1, 'gslic_rasterize_backward_adam: adam descriptor is NULL'),
    'gslic_rasterize_backward_adam/adam_null_P0': (-1, 'gslic_rasterize_backward_adam: adam descriptor is NULL'),
    'gslic_rasterize_backward_adam/adam_without_raw_params': (-1, 'fused Adam needs raw_params = 1 (it updates the raw parameters)'),
    'gslic_rasterize_backward_adam/adam_without_raw_params_group_null': (-1, 'fused Adam needs raw_params = 1 (it updates the raw parameters)'),
    'gslic_rasterize_backward_adam/adam_group3_param_null': (-1, 'fused Adam: group 3 has a NULL pointer'),
    'gslic_rasterize_backward_adam/adam_group0_exp_avg_null': (-1, 'fused Adam: group 0 has a NULL pointer'),
    'gslic_rasterize_backward_adam/adam_group5_exp_avg_sq_null': (-1, 'fused Adam: group 5 has a NULL pointer'),
    'gslic_rasterize_backward_adam/adam_group2_null_M0': (-1, 'fused Adam: param[] must alias the tensors passed as means3D / shs / scales / rotations'),
    'gslic_rasterize_backward_adam/adam_param0_not_aliasing': (-1, 'fused Adam: param[] must alias the tensors passed as means3D / shs / scales / rotations'),
    'gslic_rasterize_backward_adam/adam_param2_not_aliasing': (-1, 'fused Adam: param[] must alias the tensors passed as means3D / shs / scales / rotations'),
    'gslic_rasterize_backward_adam/adam_param5_not_aliasing_group1_null': (-1, 'fused Adam: group 1 has a NULL pointer'),
    'gslic_rasterize_backward_adam/adam_not_aliasing_negative_R': (-1, 'negative R / B'),
    'gslic_rasterize_backward_adam/adam_not_aliasing_means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_depth_adam/negative_R': (-1, 'negative R / B'),
    'gslic_rasterize_backward_depth_adam/negative_B': (-1, 'negative R / B'),
    'gslic_rasterize_backward_depth_adam/negative_R_no_color': (-1, 'depth backward: no_color = 1 (no depth forward renders without colour)'),
    'gslic_rasterize_backward_depth_adam/negative_B_geom_null': (-1, 'negative R / B'),
    'gslic_rasterize_backward_depth_adam/dL_dpix_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_depth_adam/sample_null_grad_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_depth_adam/dL_drot_null_means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_depth_adam/adam_null': (-1, 'gslic_rasterize_backward_depth_adam: adam descriptor is NULL'),
    'gslic_rasterize_backward_depth_adam/adam_null_null_params': (-1, 'params is NULL'),
    'gslic_rasterize_backward_depth_adam/adam_null_degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_backward_depth_adam/adam_null_no_color': (-1, 'gslic_rasterize_backward_depth_adam: adam descriptor is NULL'),
    'gslic_rasterize_backward_depth_adam/adam_null_negative_R': (-1, 'gslic_rasterize_backward_depth_adam: adam descriptor is NULL'),
    'gslic_rasterize_backward_depth_adam/adam_null_P0': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward_depth_adam/dL_ddepth_null': (-1, 'depth backward: dL_ddepth is NULL (gslic_rasterize_backward_adam is the colour-only backward)'),
    'gslic_rasterize_backward_depth_adam/dL_ddepth_null_null_params': (-1, 'params is NULL'),
    'gslic_rasterize_backward_depth_adam/dL_ddepth_null_degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_backward_depth_adam/dL_ddepth_null_no_color': (-1, 'depth backward: no_color = 1 (no depth forward renders without colour)'),
    'gslic_rasterize_backward_depth_adam/dL_ddepth_null_negative_R': (-1, 'depth backward: dL_ddepth is NULL (gslic_rasterize_backward_adam is the colour-only backward)'),
    'gslic_rasterize_backward_depth_adam/dL_ddepth_null_P0': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward_depth_adam/dL_dmean3D_null': (-1, 'gslic_rasterize_backward_depth_adam: dL_dmean3D is NULL (the xyz gradient is assembled there before its update)'),
    'gslic_rasterize_backward_depth_adam/dL_dmean3D_null_null_params': (-1, 'params is NULL'),
    'gslic_rasterize_backward_depth_adam/dL_dmean3D_null_degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_backward_depth_adam/dL_dmean3D_null_no_color': (-1, 'depth backward: no_color = 1 (no depth forward renders without colour)'),
    'gslic_rasterize_backward_depth_adam/dL_dmean3D_null_negative_R': (-1, 'gslic_rasterize_backward_depth_adam: dL_dmean3D is NULL (the xyz gradient is assembled there before its update)'),
    'gslic_rasterize_backward_depth_adam/dL_dmean3D_null_P0': (0, 'bad kernel id -1'),
    'gslic_rasterize_backward_depth_adam/adam_null_dL_ddepth_null': (-1, 'gslic_rasterize_backward_depth_adam: adam descriptor is NULL'),
    'gslic_rasterize_backward_depth_adam/dL_ddepth_null_dL_dmean3D_null': (-1, 'depth backward: dL_ddepth is NULL (gslic_rasterize_backward_adam is the colour-only backward)'),
    'gslic_rasterize_backward_depth_adam/adam_without_raw_params': (-1, 'fused Adam needs raw_params = 1 (it updates the raw parameters)'),
    'gslic_rasterize_backward_depth_adam/adam_without_raw_params_group_null': (-1, 'fused Adam needs raw_params = 1 (it updates the raw parameters)'),
    'gslic_rasterize_backward_depth_adam/adam_group3_param_null': (-1, 'fused Adam: group 3 has a NULL pointer'),
    'gslic_rasterize_backward_depth_adam/adam_group0_exp_avg_null': (-1, 'fused Adam: group 0 has a NULL pointer'),
    'gslic_rasterize_backward_depth_adam/adam_group5_exp_avg_sq_null': (-1, 'fused Adam: group 5 has a NULL pointer'),
    'gslic_rasterize_backward_depth_adam/adam_group2_null_M0': (-1, 'fused Adam: param[] must alias the tensors passed as means3D / shs / scales / rotations'),
    'gslic_rasterize_backward_depth_adam/adam_param0_not_aliasing': (-1, 'fused Adam: param[] must alias the tensors passed as means3D / shs / scales / rotations'),
    'gslic_rasterize_backward_depth_adam/adam_param2_not_aliasing': (-1, 'fused Adam: param[] must alias the tensors passed as means3D / shs / scales / rotations'),
    'gslic_rasterize_backward_depth_adam/adam_param5_not_aliasing_group1_null': (-1, 'fused Adam: group 1 has a NULL pointer'),
    'gslic_rasterize_backward_depth_adam/adam_not_aliasing_negative_R': (-1, 'negative R / B'),
    'gslic_rasterize_backward_depth_adam/adam_not_aliasing_means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_camera/negative_R': (-1, 'negative R / B'),
    'gslic_rasterize_backward_camera/negative_B': (-1, 'negative R / B'),
    'gslic_rasterize_backward_camera/negative_R_no_color': (-1, 'backward of a no_color forward is undefined (no checkpoints were stored)'),
    'gslic_rasterize_backward_camera/negative_B_geom_null': (-1, 'negative R / B'),
    'gslic_rasterize_backward_camera/dL_dpix_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_camera/sample_null_grad_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_camera/dL_dopacity_null': (-1, 'required gradient output pointer is NULL'),
    'gslic_rasterize_backward_camera/dL_dopacity_null_bad_rows_or_precomp': (-2, 'colors_precomp / cov3D_precomp are not supported'),
    'gslic_rasterize_backward_camera/dL_drot_null_means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_camera/dL_dprojmatrix_null': (-1, 'gslic_rasterize_backward_camera: a camera-gradient output pointer is NULL'),
    'gslic_rasterize_backward_camera/dL_dprojmatrix_null_null_params': (-1, 'gslic_rasterize_backward_camera: a camera-gradient output pointer is NULL'),
    'gslic_rasterize_backward_camera/dL_dprojmatrix_null_degree4': (-1, 'gslic_rasterize_backward_camera: a camera-gradient output pointer is NULL'),
    'gslic_rasterize_backward_camera/dL_dprojmatrix_null_no_color': (-1, 'gslic_rasterize_backward_camera: a camera-gradient output pointer is NULL'),
    'gslic_rasterize_backward_camera/dL_dprojmatrix_null_negative_R': (-1, 'gslic_rasterize_backward_camera: a camera-gradient output pointer is NULL'),
    'gslic_rasterize_backward_camera/dL_dprojmatrix_null_P0': (-1, 'gslic_rasterize_backward_camera: a camera-gradient output pointer is NULL'),
    'gslic_rasterize_backward_camera/dL_dviewmatrix_null': (-1, 'gslic_rasterize_backward_camera: a camera-gradient output pointer is NULL'),
    'gslic_rasterize_backward_camera/dL_dcampos_null_null_params': (-1, 'gslic_rasterize_backward_camera: a camera-gradient output pointer is NULL'),
    'gslic_rasterize_backward_depth_camera/negative_R': (-1, 'negative R / B'),
    'gslic_rasterize_backward_depth_camera/negative_B': (-1, 'negative R / B'),
    'gslic_rasterize_backward_depth_camera/negative_R_no_color': (-1, 'depth backward: no_color = 1 (no depth forward renders without colour)'),
    'gslic_rasterize_backward_depth_camera/negative_B_geom_null': (-1, 'negative R / B'),
    'gslic_rasterize_backward_depth_camera/dL_dpix_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_depth_camera/sample_null_grad_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_depth_camera/dL_dopacity_null': (-1, 'required gradient output pointer is NULL'),
    'gslic_rasterize_backward_depth_camera/dL_dopacity_null_bad_rows_or_precomp': (-2, 'colors_precomp / cov3D_precomp are not supported'),
    'gslic_rasterize_backward_depth_camera/dL_drot_null_means3D_null': (-1, 'required tensor pointer is NULL'),
    'gslic_rasterize_backward_depth_camera/dL_dprojmatrix_null': (-1, 'gslic_rasterize_backward_depth_camera: a camera-gradient output pointer is NULL'),
    'gslic_rasterize_backward_depth_camera/dL_dprojmatrix_null_null_params': (-1, 'gslic_rasterize_backward_depth_camera: a camera-gradient output pointer is NULL'),
    'gslic_rasterize_backward_depth_camera/dL_dprojmatrix_null_degree4': (-1, 'gslic_rasterize_backward_depth_camera: a camera-gradient output pointer is NULL'),
    'gslic_rasterize_backward_depth_camera/dL_dprojmatrix_null_no_color': (-1, 'gslic_rasterize_backward_depth_camera: a camera-gradient output pointer is NULL'),
    'gslic_rasterize_backward_depth_camera/dL_dprojmatrix_null_negative_R': (-1, 'gslic_rasterize_backward_depth_camera: a camera-gradient output pointer is NULL'),
    'gslic_rasterize_backward_depth_camera/dL_dprojmatrix_null_P0': (-1, 'gslic_rasterize_backward_depth_camera: a camera-gradient output pointer is NULL'),
    'gslic_rasterize_backward_depth_camera/dL_ddepth_null': (-1, 'depth backward: dL_ddepth is NULL (gslic_rasterize_backward_camera is the colour-only camera backward)'),
    'gslic_rasterize_backward_depth_camera/dL_ddepth_null_null_params': (-1, 'params is NULL'),
    'gslic_rasterize_backward_depth_camera/dL_ddepth_null_degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_backward_depth_camera/dL_ddepth_null_no_color': (-1, 'depth backward: no_color = 1 (no depth forward renders without colour)'),
    'gslic_rasterize_backward_depth_camera/dL_ddepth_null_negative_R': (-1, 'depth backward: dL_ddepth is NULL (gslic_rasterize_backward_camera is the colour-only camera backward)'),
    'gslic_rasterize_backward_depth_camera/dL_dmean3D_null': (-1, "gslic_rasterize_backward_depth_camera: dL_dmean3D is NULL (the depth's share is added to it)"),
    'gslic_rasterize_backward_depth_camera/dL_dmean3D_null_null_params': (-1, 'params is NULL'),
    'gslic_rasterize_backward_depth_camera/dL_dmean3D_null_degree4': (-1, 'SH degree 4 out of range 0..3'),
    'gslic_rasterize_backward_depth_camera/dL_dmean3D_null_no_color': (-1, 'depth backward: no_color = 1 (no depth forward renders without colour)'),
    'gslic_rasterize_backward_depth_camera/dL_dmean3D_null_negative_R': (-1, "gslic_rasterize_backward_depth_camera: dL_dmean3D is NULL (the depth's share is added to it)"),
    'gslic_rasterize_backward_depth_camera/dL_dprojmatrix_null_dL_ddepth_null': (-1, 'gslic_rasterize_backward_depth_camera: a camera-gradient output pointer is NULL'),
    'gslic_rasterize_backward_depth_camera/dL_ddepth_null_dL_dmean3D_null': (-1, 'depth backward: dL_ddepth is NULL (gslic_rasterize_backward_camera is the colour-only camera backward)'),
    'gslic_rasterize_backward_depth_camera/dL_dviewmatrix_null': (-1, 'gslic_rasterize_backward_depth_camera: a camera-gradient output pointer is NULL'),
    'gslic_rasterize_backward_depth_camera/dL_dcampos_null_null_params': (-1, 'gslic_rasterize_backward_depth_camera: a camera-gradient output pointer is NULL'),
    'gslic_sh_grad_from_rgb/view_stride_negative': (-1, 'gslic_sh_grad_from_rgb: bad view_stride'),
    'gslic_sh_grad_from_rgb/view_stride_too_small': (-1, 'gslic_sh_grad_from_rgb: bad view_stride'),
    'gslic_sh_grad_from_rgb/view_stride_negative_degree4': (-1, 'gslic_sh_grad_from_rgb: bad view_stride'),
    'gslic_sh_grad_from_rgb/degree4': (-1, 'gslic_sh_grad_from_rgb: bad P / D / M / n_views'),
    'gslic_sh_grad_from_rgb/P_negative': (-1, 'gslic_sh_grad_from_rgb: bad P / D / M / n_views'),
    'gslic_sh_grad_from_rgb/M_negative': (-1, 'gslic_sh_grad_from_rgb: bad P / D / M / n_views'),
    'gslic_sh_grad_from_rgb/n_views_0': (-1, 'gslic_sh_grad_from_rgb: bad P / D / M / n_views'),
    'gslic_sh_grad_from_rgb/n_views_0_means3D_null': (-1, 'gslic_sh_grad_from_rgb: bad P / D / M / n_views'),
    'gslic_sh_grad_from_rgb/P0': (0, 'bad kernel id -1'),
    'gslic_sh_grad_from_rgb/P0_means3D_null': (0, 'bad kernel id -1'),
    'gslic_sh_grad_from_rgb/P0_degree4': (-1, 'gslic_sh_grad_from_rgb: bad P / D / M / n_views'),
    'gslic_sh_grad_from_rgb/means3D_null': (-1, 'gslic_sh_grad_from_rgb: NULL pointer'),
    'gslic_sh_grad_from_rgb/rgb_all_null': (-1, 'gslic_sh_grad_from_rgb: NULL pointer'),
    'gslic_sh_grad_from_rgb/dL_ddc_null': (-1, 'gslic_sh_grad_from_rgb: NULL pointer'),
    'gslic_sh_grad_from_rgb/dL_dsh_null': (-1, 'gslic_sh_grad_from_rgb: NULL pointer'),
    'gslic_sh_grad_from_rgb/dL_dsh_null_M0_view_stride_negative': (-1, 'gslic_sh_grad_from_rgb: bad view_stride'),
    'gslic_sh_grad_from_rgb_adam/view_stride_negative': (-1, 'gslic_sh_grad_from_rgb_adam: bad view_stride'),
    'gslic_sh_grad_from_rgb_adam/view_stride_too_small': (-1, 'gslic_sh_grad_from_rgb_adam: bad view_stride'),
    'gslic_sh_grad_from_rgb_adam/view_stride_negative_degree4': (-1, 'gslic_sh_grad_from_rgb_adam: bad view_stride'),
    'gslic_sh_grad_from_rgb_adam/degree4': (-1, 'gslic_sh_grad_from_rgb_adam: bad P / D / M / n_views'),
    'gslic_sh_grad_from_rgb_adam/P_negative': (-1, 'gslic_sh_grad_from_rgb_adam: bad P / D / M / n_views'),
    'gslic_sh_grad_from_rgb_adam/M_negative': (-1, 'gslic_sh_grad_from_rgb_adam: bad P / D / M / n_views'),
    'gslic_sh_grad_from_rgb_adam/n_views_0': (-1, 'gslic_sh_grad_from_rgb_adam: bad P / D / M / n_views'),
    'gslic_sh_grad_from_rgb_adam/n_views_0_means3D_null': (-1, 'gslic_sh_grad_from_rgb_adam: bad P / D / M / n_views'),
    'gslic_sh_grad_from_rgb_adam/P0': (0, 'bad kernel id -1'),
    'gslic_sh_grad_from_rgb_adam/P0_means3D_null': (0, 'bad kernel id -1'),
    'gslic_sh_grad_from_rgb_adam/P0_degree4': (-1, 'gslic_sh_grad_from_rgb_adam: bad P / D / M / n_views'),
    'gslic_sh_grad_from_rgb_adam/means3D_null': (-1, 'gslic_sh_grad_from_rgb_adam: NULL pointer'),
    'gslic_sh_grad_from_rgb_adam/rgb_all_null': (-1, 'gslic_sh_grad_from_rgb_adam: NULL pointer'),
    'gslic_sh_grad_from_rgb_adam/adam_null': (-1, 'gslic_sh_grad_from_rgb_adam: NULL pointer'),
    'gslic_sh_grad_from_rgb_adam/adam_null_P0': (0, 'bad kernel id -1'),
    'gslic_sh_grad_from_rgb_adam/adam_group1_param_null': (-1, 'gslic_sh_grad_from_rgb_adam: group 1 has a NULL pointer'),
    'gslic_sh_grad_from_rgb_adam/adam_group2_exp_avg_null': (-1, 'gslic_sh_grad_from_rgb_adam: group 2 has a NULL pointer'),
    'gslic_sh_grad_from_rgb_adam/adam_group1_null_means3D_null': (-1, 'gslic_sh_grad_from_rgb_adam: NULL pointer'),
    'gslic_sh_grad_from_rgb_adam/visible_null': (-1, 'gslic_sh_grad_from_rgb_adam: NULL pointer'),
    'gslic_sh_grad_from_rgb_adam_all/view_stride_negative': (-1, 'gslic_sh_grad_from_rgb_adam_all: bad view_stride'),
    'gslic_sh_grad_from_rgb_adam_all/view_stride_too_small': (-1, 'gslic_sh_grad_from_rgb_adam_all: bad view_stride'),
    'gslic_sh_grad_from_rgb_adam_all/view_stride_negative_degree4': (-1, 'gslic_sh_grad_from_rgb_adam_all: bad view_stride'),
    'gslic_sh_grad_from_rgb_adam_all/degree4': (-1, 'gslic_sh_grad_from_rgb_adam_all: bad P / D / M / n_views / vis_stride'),
    'gslic_sh_grad_from_rgb_adam_all/P_negative': (-1, 'gslic_sh_grad_from_rgb_adam_all: bad P / D / M / n_views / vis_stride'),
    'gslic_sh_grad_from_rgb_adam_all/M_negative': (-1, 'gslic_sh_grad_from_rgb_adam_all: bad P / D / M / n_views / vis_stride'),
    'gslic_sh_grad_from_rgb_adam_all/n_views_0': (-1, 'gslic_sh_grad_from_rgb_adam_all: bad P / D / M / n_views / vis_stride'),
    'gslic_sh_grad_from_rgb_adam_all/n_views_0_means3D_null': (-1, 'gslic_sh_grad_from_rgb_adam_all: bad P / D / M / n_views / vis_stride'),
    'gslic_sh_grad_from_rgb_adam_all/P0': (0, 'bad kernel id -1'),
    'gslic_sh_grad_from_rgb_adam_all/P0_means3D_null': (0, 'bad kernel id -1'),
    'gslic_sh_grad_from_rgb_adam_all/P0_degree4': (-1, 'gslic_sh_grad_from_rgb_adam_all: bad P / D / M / n_views / vis_stride'),
    'gslic_sh_grad_from_rgb_adam_all/means3D_null': (-1, 'gslic_sh_grad_from_rgb_adam_all: NULL pointer'),
    'gslic_sh_grad_from_rgb_adam_all/rgb_all_null': (-1, 'gslic_sh_grad_from_rgb_adam_all: NULL pointer'),
    'gslic_sh_grad_from_rgb_adam_all/adam_null': (-1, 'gslic_sh_grad_from_rgb_adam_all: NULL pointer'),
    'gslic_sh_grad_from_rgb_adam_all/adam_null_P0': (0, 'bad kernel id -1'),
    'gslic_sh_grad_from_rgb_adam_all/adam_group1_param_null': (-1, 'gslic_sh_grad_from_rgb_adam_all: group 1 has a NULL pointer'),
    'gslic_sh_grad_from_rgb_adam_all/adam_group2_exp_avg_null': (-1, 'gslic_sh_grad_from_rgb_adam_all: group 2 has a NULL pointer'),
    'gslic_sh_grad_from_rgb_adam_all/adam_group1_null_means3D_null': (-1, 'gslic_sh_grad_from_rgb_adam_all: NULL pointer'),
    'gslic_sh_grad_from_rgb_adam_all/vis_all_null': (-1, 'gslic_sh_grad_from_rgb_adam_all: NULL pointer'),
    'gslic_sh_grad_from_rgb_adam_all/vis_stride_negative': (-1, 'gslic_sh_grad_from_rgb_adam_all: bad P / D / M / n_views / vis_stride'),
    'gslic_sh_grad_from_rgb_adam_all/vis_stride_too_small': (-1, 'gslic_sh_grad_from_rgb_adam_all: bad P / D / M / n_views / vis_stride'),
    'gslic_sh_grad_from_rgb_adam_all/vis_stride_too_small_view_stride_negative': (-1, 'gslic_sh_grad_from_rgb_adam_all: bad view_stride'),
    'gslic_sh_grad_from_rgb_adam_all/small_gradients_partial': (-1, 'gslic_sh_grad_from_rgb_adam_all: the four small gradients are given together or not at all'),
    'gslic_sh_grad_from_rgb_adam_all/small_gradients_partial_group_null': (-1, 'gslic_sh_grad_from_rgb_adam_all: the four small gradients are given together or not at all'),
    'gslic_sh_grad_from_rgb_adam_all/adam_group0_null_with_small': (-1, 'gslic_sh_grad_from_rgb_adam_all: group 0 has a NULL pointer'),
    'gslic_sh_grad_from_rgb_adam_all/adam_group5_null_with_small': (-1, 'gslic_sh_grad_from_rgb_adam_all: group 5 has a NULL pointer'),
    'gslic_sh_grad_from_rgb_adam_all/adam_group1_null_without_small': (-1, 'gslic_sh_grad_from_rgb_adam_all: group 1 has a NULL pointer'),
}


@pytest.mark.parametrize("entry,name,mutations", CASES, ids=[f"{e[6:]}-{n}" for e, n, _m in CASES])
def test_argument_checks_keep_their_code_text_and_order(entry, name, mutations):
    assert _call(entry, mutations) == EXPECTED[f"{entry}/{name}"]


def test_every_case_stays_off_the_device():
    """No expected result is a HIP error (code -4) or mentions a device call: each case ends in an argument check, or at P == 0."""
    assert len(EXPECTED) == len(CASES) == len({f"{e}/{n}" for e, n, _m in CASES})
    for key, (rc, msg) in EXPECTED.items():
        assert rc != -4 and "hip" not in msg.lower().replace("gslic_hip", ""), (key, rc, msg)
        assert (rc == 0) == (msg == SENTINEL), (key, rc, msg)
