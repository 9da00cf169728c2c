"""Host-side mirror of the reference's rasterizer operator interface on top of the C-ABI.

Same names and argument meaning as the reference's L2/L3 layers:
  rasterize_gaussians / rasterize_gaussians_backward  <- RasterizeGaussiansCUDA / ...BackwardCUDA
                                                         (src/rasterizer/rasterize_points.h:25-82)
  GaussianRasterizationSettings, GaussianRasterizerFunction, GaussianRasterizer
                                                      <- src/rasterizer/rasterizer.h:27-114, rasterizer.cpp:21-216
  render                                              <- src/rasterizer/renderer.cpp:21-88
torch is used for device memory, streams and autograd plumbing only; all arithmetic runs in libgslic_hip.so.
"""
import ctypes
from dataclasses import dataclass

import torch

from . import _lib


@dataclass
class GaussianRasterizationSettings:
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    limx_neg: float
    limx_pos: float
    limy_neg: float
    limy_pos: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor   # [4,4] world_view_transform_ (stored transposed, camera.h:86)
    projmatrix: torch.Tensor   # [4,4] full_proj_transform_
    sh_degree: int
    campos: torch.Tensor       # [3]
    prefiltered: bool = False
    debug: bool = False
    no_color: bool = False
    lambda_erank: float = 0.0
    tie_rank: torch.Tensor = None   # not in the reference: int32 [P], set by render() for a model that keeps its rows in a permuted order (_params)
    mean2d_grad_out: torch.Tensor = None   # not in the reference: float32 [P,3] the raw nodes' backward writes dL_dmeans2D into (render(mean2d_grad_out=))


def _params(P, D, M, H, W, tanfovx, tanfovy, lxn, lxp, lyn, lyp, scale_modifier, prefiltered, debug, no_color, raw=False, tie_rank=None):
    """tie_rank (forward only): device int32 [P], the rows' indices in the map's ORIGINAL order when the host stores them permuted
    (gslic_raster_params.tie_rank); the caller keeps the tensor alive for the duration of the call."""
    if tie_rank is not None:
        assert tie_rank.is_contiguous() and tie_rank.dtype == torch.int32 and tie_rank.numel() >= int(P)
    return _lib.RasterParams(int(P), int(D), int(M), int(W), int(H), float(tanfovx), float(tanfovy), float(lxn), float(lxp),
                             float(lyn), float(lyp), float(scale_modifier), int(bool(prefiltered)), int(bool(debug)),
                             int(bool(no_color)), int(bool(raw)), None if tie_rank is None else ctypes.c_void_p(tie_rank.data_ptr()))


def _f32c(t):
    return t.contiguous() if t.dtype == torch.float32 else t.float().contiguous()


def _sh_width(sh):
    return sh.size(1) if sh is not None and sh.size(0) != 0 else 0


def _forward(bufs, depth, view, degree, prefiltered, debug, no_color, raw_params, tie_rank, background, means3D, dc, sh, colors, opacity, scales,
             rotations, cov3D_precomp, viewmatrix, projmatrix, campos):
    """The one forward behind the four public ones.  bufs: None = the library's allocator callbacks size the scratch (two host round trips), a
    CapacityBuffers = caller-owned scratch and outputs (no copies are made: addresses have to be stable for graph capture); depth: also render
    the depth image.  view = (H, W, tan_fovx, tan_fovy, limx_neg, limx_pos, limy_neg, limy_pos, scale_modifier), _params' order.
    Returns (R, B, out_color, out_final_T, out_depth or None, radii, geom, binning, img, sample)."""
    L = _lib.lib()
    P, M = means3D.size(0), _sh_width(sh)
    p = _lib.ptr
    R, B = ctypes.c_int32(0), ctypes.c_int32(0)
    if bufs is None:
        dev, (H, W) = means3D.device, view[:2]
        mk = torch.zeros if P == 0 else torch.empty
        out_color = (torch.zeros if no_color else mk)(3, H, W, dtype=torch.float32, device=dev)
        out_final_T = mk(H, W, dtype=torch.float32, device=dev)
        out_depth = mk(H, W, dtype=torch.float32, device=dev) if depth else None
        radii = torch.empty(P, dtype=torch.int32, device=dev)
        allocs = [_lib.TensorAllocator(dev) for _ in range(4)]  # geom, binning, img, sample
        scratch = (allocs[0].cb, None, allocs[1].cb, None, allocs[2].cb, None, allocs[3].cb, None)
        status = ()
        if P != 0:
            means3D, dc, opacity, scales, rotations = map(_f32c, (means3D, dc, opacity, scales, rotations))
            sh = _f32c(sh) if M > 0 else None
            viewmatrix, projmatrix, campos, background = map(_f32c, (viewmatrix, projmatrix, campos, background))
        fn = L.gslic_rasterize_forward_depth if depth else L.gslic_rasterize_forward
    else:
        assert P == bufs.P and P > 0
        if depth and not bufs.with_depth:
            raise ValueError("rasterize_gaussians_depth_capacity needs CapacityBuffers(..., depth=True)")
        for t in (means3D, dc, opacity, scales, rotations, viewmatrix, projmatrix, campos):
            assert t.is_contiguous() and t.dtype == torch.float32
        out_color, out_final_T, out_depth, radii = bufs.color, bufs.final_T, bufs.depth if depth else None, bufs.radii
        bp = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None
        scratch = (bp(bufs.geom), bufs.geom.numel(), bp(bufs.binning), bufs.binning.numel(), bp(bufs.img), bufs.img.numel(), bp(bufs.sample),
                   bufs.sample.numel())
        status = (p(bufs.status),)
        sh = sh if M > 0 else None
        fn = L.gslic_rasterize_forward_depth_capacity if depth else L.gslic_rasterize_forward_capacity
    if P != 0:
        prm = _params(P, degree, M, *view, prefiltered, debug, no_color, raw_params, tie_rank)
        _lib.check(fn(ctypes.byref(prm), *scratch, p(background), p(means3D), p(dc), p(sh), p(colors), p(opacity), p(scales), p(rotations),
                      p(cov3D_precomp), p(viewmatrix), p(projmatrix), p(campos), p(out_color), p(out_final_T), *((p(out_depth),) if depth else ()),
                      p(radii), ctypes.byref(R), ctypes.byref(B), *status, _lib.current_stream_ptr()))
    if bufs is None:
        geom, binning, img, sample = (a.tensor for a in allocs)
    else:
        bufs.cap_R, bufs.cap_B = R.value, B.value
        geom, binning, img, sample = bufs.geom, bufs.binning, bufs.img, bufs.sample
    return (R.value, B.value, out_color, out_final_T, out_depth, radii, geom, binning, img, sample)


def rasterize_gaussians(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                        projmatrix, tan_fovx, tan_fovy, image_height, image_width, limx_neg, limx_pos, limy_neg, limy_pos,
                        dc, sh, degree, campos, prefiltered, debug, no_color=False, raw_params=False, tie_rank=None):
    """RasterizeGaussiansCUDA (rasterize_points.cu:50-149): returns
    (num_rendered, num_buckets, out_color, out_final_T, radii, geomBuffer, binningBuffer, imgBuffer, sampleBuffer).
    raw_params=True (not in the reference): opacity / scales / rotations are the RAW parameters, activated inside the kernels.
    tie_rank (not in the reference): see _params — a map stored in a permuted row order renders as the unpermuted one."""
    if means3D.dim() != 2 or means3D.size(1) != 3:
        raise ValueError("means3D must have dimensions (num_points, 3)")  # rasterize_points.cu:77-80
    view = (int(image_height), int(image_width), tan_fovx, tan_fovy, limx_neg, limx_pos, limy_neg, limy_pos, scale_modifier)
    r = _forward(None, False, view, degree, prefiltered, debug, no_color, raw_params, tie_rank, background, means3D, dc, sh, colors, opacity, scales,
                 rotations, cov3D_precomp, viewmatrix, projmatrix, campos)
    return r[:4] + r[5:]


def rasterize_gaussians_depth(background, means3D, opacity, scales, rotations, scale_modifier, viewmatrix, projmatrix, tan_fovx, tan_fovy,
                              image_height, image_width, limx_neg, limx_pos, limy_neg, limy_pos, dc, sh, degree, campos, prefiltered=False,
                              debug=False, raw_params=False, tie_rank=None):
    """gslic_rasterize_forward_depth (no reference counterpart): rasterize_gaussians plus the depth image.  Returns
    (num_rendered, num_buckets, out_color, out_final_T, out_depth, radii, geomBuffer, binningBuffer, imgBuffer, sampleBuffer).
    out_depth [H,W] = sum T alpha z over the colour's contributors (z = view-space depth), NOT normalised (divide by 1 - final_T for
    the expected depth of the covered part); colour, final_T and radii are bit-identical to rasterize_gaussians'."""
    if means3D.dim() != 2 or means3D.size(1) != 3:
        raise ValueError("means3D must have dimensions (num_points, 3)")
    view = (int(image_height), int(image_width), tan_fovx, tan_fovy, limx_neg, limx_pos, limy_neg, limy_pos, scale_modifier)
    return _forward(None, True, view, degree, prefiltered, debug, False, raw_params, tie_rank, background, means3D, dc, sh, None, opacity, scales,
                    rotations, None, viewmatrix, projmatrix, campos)


class CapacityBuffers:
    """Caller-owned scratch + outputs of gslic_rasterize_forward_capacity for one (P, W, H): nothing is allocated per step, every
    address is stable, so the step can be captured in a hipGraph.  cap_R / cap_B: how many instances / checkpoint buckets fit.
    depth=True: the buffers of gslic_rasterize_forward_depth_capacity (the depth carves, gslic_*_bytes_depth) and a `depth` [H,W] output."""

    def __init__(self, P, W, H, cap_R, cap_B, device, no_color=False, depth=False):
        L = _lib.lib()
        self.P, self.W, self.H, self.no_color, self.with_depth = int(P), int(W), int(H), bool(no_color), bool(depth)
        if depth and no_color:
            raise ValueError("CapacityBuffers(depth=True) needs the colour (no_color=False)")
        mk = lambda n: torch.empty(int(n), dtype=torch.uint8, device=device)
        self.geom = mk(L.gslic_geom_bytes(self.P))
        if depth:
            self.img = mk(L.gslic_img_bytes_depth(self.W, self.H))
            self.binning = mk(L.gslic_binning_bytes_depth(int(cap_R)))
            self.sample = mk(L.gslic_sample_bytes_depth(int(cap_B)))
        else:
            self.img = mk(L.gslic_img_bytes(self.W, self.H))
            self.binning = mk(L.gslic_binning_bytes(int(cap_R), int(no_color)))
            self.sample = mk(L.gslic_sample_bytes(int(cap_B)) if not no_color else 0)
        self.status = torch.zeros(8, dtype=torch.int32, device=device)
        self.color = torch.zeros(3, self.H, self.W, dtype=torch.float32, device=device)
        self.final_T = torch.empty(self.H, self.W, dtype=torch.float32, device=device)
        self.depth = torch.zeros(self.H, self.W, dtype=torch.float32, device=device) if depth else None
        self.radii = torch.empty(self.P, dtype=torch.int32, device=device)
        self.cap_R = self.cap_B = 0   # filled by the first forward (what the library derives from the buffer sizes)

    def read_status(self):
        """(R, B, bits, forwards that completed) of the status words — synchronises."""
        r, b, bits, good = (int(v) for v in self.status.cpu().tolist()[:4])
        return r & 0xffffffff, b & 0xffffffff, bits, good & 0xffffffff

    def read_window(self):
        """(forwards issued, bit mask of the issue indices mod 32 that did not complete, largest R, largest B) since the words were zeroed
        — synchronises."""
        w = [int(v) & 0xffffffff for v in self.status.cpu().tolist()]
        return w[4], w[5], w[6], w[7]


def rasterize_gaussians_capacity(bufs, background, means3D, opacity, scales, rotations, scale_modifier, viewmatrix, projmatrix, tan_fovx, tan_fovy,
                                 limx_neg, limx_pos, limy_neg, limy_pos, dc, sh, degree, campos, raw_params=False, tie_rank=None):
    """gslic_rasterize_forward_capacity: RasterizeGaussiansCUDA without a host round trip, into caller-owned buffers.  The tensors must
    already be contiguous fp32 (no copies are made: addresses have to be stable for graph capture).  Returns the same 9-tuple as
    rasterize_gaussians with (cap_R, cap_B) in place of (R, B) — pass them on to rasterize_gaussians_backward unchanged."""
    view = (bufs.H, bufs.W, tan_fovx, tan_fovy, limx_neg, limx_pos, limy_neg, limy_pos, scale_modifier)
    r = _forward(bufs, False, view, degree, False, False, bufs.no_color, raw_params, tie_rank, background, means3D, dc, sh, None, opacity, scales,
                 rotations, None, viewmatrix, projmatrix, campos)
    return r[:4] + r[5:]


def rasterize_gaussians_depth_capacity(bufs, background, means3D, opacity, scales, rotations, scale_modifier, viewmatrix, projmatrix, tan_fovx,
                                       tan_fovy, limx_neg, limx_pos, limy_neg, limy_pos, dc, sh, degree, campos, raw_params=False, tie_rank=None):
    """gslic_rasterize_forward_depth_capacity: rasterize_gaussians_capacity plus the depth image, into CapacityBuffers(depth=True).  Returns
    (cap_R, cap_B, out_color, out_final_T, out_depth, radii, geom, binning, img, sample); bit-identical to rasterize_gaussians_depth."""
    view = (bufs.H, bufs.W, tan_fovx, tan_fovy, limx_neg, limx_pos, limy_neg, limy_pos, scale_modifier)
    return _forward(bufs, True, view, degree, False, False, False, raw_params, tie_rank, background, means3D, dc, sh, None, opacity, scales,
                    rotations, None, viewmatrix, projmatrix, campos)


def _backward(view, degree, debug, raw_params, background, means3D, radii, colors, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, campos,
              dL_dout_color, dL_dout_depth, dc, sh, geomBuffer, R, binningBuffer, imageBuffer, B, sampleBuffer, lambda_erank, out=None, adam=None,
              camera_grads=False, rgb_out=None, rows=None, skip_blend=False, out_addr=None, payload=None, xyz_grad=None, grad_stats=None,
              mean2d_out=None, cam_out=None):
    """The one backward behind the two public ones (see there for the modes).  dL_dout_depth: None = the colour-only entry points, a tensor =
    their depth twins.  view as _forward's.  grad_stats (a _lib.GradStats, with adam only): the *_adam_stats entry points; mean2d_out
    (float32 [P,3], with out and no adam / rgb_out): dL_dmeans2D is written there instead of not being materialised.
    camera_grads with adam: gslic_rasterize_backward_camera_adam / _depth_camera_adam — the Adam update inside the backward AND the camera
    gradient; returns (dL_dviewmatrix [16], dL_dprojmatrix [16], dL_dcampos [3]) — views of cam_out (a float32 [35] the caller keeps, e.g. a
    captured step's static buffer) or of a new tensor.  mean2d_out is then written too; grad_stats / rows / rgb_out do not combine with it."""
    if grad_stats is not None and adam is None:
        raise ValueError("grad_stats goes with adam (the fused backward); the other backwards give dL_dmeans2D to gradient_stats_accumulate")
    cam_adam = camera_grads and adam is not None
    if cam_adam and (grad_stats is not None or rows is not None or rgb_out is not None):
        raise ValueError("camera_grads with adam: no grad_stats (pass mean2d_out and use gradient_stats_accumulate), no rows, no rgb_out")
    if cam_out is not None:
        if not cam_adam:
            raise ValueError("cam_out goes with camera_grads and adam")
        if cam_out.numel() != 35 or cam_out.dtype != torch.float32 or not cam_out.is_contiguous() or cam_out.device != means3D.device:
            raise ValueError("cam_out must be 35 contiguous float32 values on the model's device")
    L = _lib.lib()
    dev, P, M = means3D.device, means3D.size(0), _sh_width(sh)
    depth = dL_dout_depth is not None
    full = adam is None and rgb_out is None   # the nine gradient tensors are returned (else: None)
    if rgb_out is not None:
        assert out is not None   # the four other parameter gradients go into the caller's storage, nothing else is materialised
    if cam_adam:
        if mean2d_out is not None:
            assert mean2d_out.is_contiguous() and mean2d_out.dtype == torch.float32 and mean2d_out.numel() >= 3 * P
        if cam_out is None:
            cam_out = torch.empty(35, dtype=torch.float32, device=dev)
        cam = (cam_out[:16], cam_out[16:32], cam_out[32:35])
    if adam is not None and depth and P == 0:
        if cam_adam:
            cam_out.zero_()
            return cam
        return None   # (the colour-only fused backward leaves P == 0 to the library, which returns at once)
    if full and out is not None:
        # caller-provided gradient storage (e.g. views of one flat slab for a zero-copy all-reduce); the tensors the host
        # discards (means2D, conic, colors_precomp, cov3D: rasterizer.cpp:171-182) are not materialised at all
        dL_dmeans3D, dL_ddc, dL_dsh = out["xyz"], out["features_dc"], out["features_rest"]
        dL_dopacities, dL_dscales, dL_drotations = out["opacity"], out["scaling"], out["rotation"]
        dL_dmeans2D = dL_dcolors = dL_dconic = dL_dcov3D = None
        if mean2d_out is not None:
            assert mean2d_out.is_contiguous() and mean2d_out.dtype == torch.float32 and mean2d_out.numel() >= 3 * P
            dL_dmeans2D = mean2d_out
    elif full:
        mk = (lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)) if P != 0 else \
            (lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev))
        dL_dmeans3D, dL_dmeans2D, dL_dcolors = mk(P, 3), mk(P, 3), mk(P, 3)
        dL_dconic, dL_dopacities, dL_dcov3D = mk(P, 2, 2), mk(P, 1), mk(P, 6)
        dL_ddc, dL_dsh, dL_dscales, dL_drotations = mk(P, 1, 3), mk(P, M, 3), mk(P, 3), mk(P, 4)
    if P != 0 or adam is not None:
        means3D, dc, scales, rotations, dL = map(_f32c, (means3D, dc, scales, rotations, dL_dout_color))
        dLd = _f32c(dL_dout_depth) if depth else None
        sh_c = _f32c(sh) if M > 0 else None
        viewmatrix, projmatrix, campos, background = map(_f32c, (viewmatrix, projmatrix, campos, background))
        if adam is not None and depth:
            if xyz_grad is None:
                xyz_grad = torch.empty(P, 3, dtype=torch.float32, device=dev)
            assert xyz_grad.is_contiguous() and xyz_grad.numel() >= 3 * P
        prm = _params(P, degree, M, *view, False, debug, False, True if adam is not None else raw_params)
        p, vp, erank = _lib.ptr, ctypes.c_void_p, float(lambda_erank)
        # what every variant starts with: params, R, B, the twelve inputs, the four buffers, dL (and dL/d depth)
        head = (ctypes.byref(prm), int(R), int(B), p(background), p(means3D), p(dc), p(sh_c), p(colors), p(scales), p(rotations), p(cov3D_precomp),
                p(viewmatrix), p(projmatrix), p(campos), p(radii.contiguous()), vp(geomBuffer.data_ptr()), vp(binningBuffer.data_ptr()),
                vp(imageBuffer.data_ptr()), vp(sampleBuffer.data_ptr()), p(dL)) + ((p(dLd),) if depth else ())
        if adam is not None:
            # single-GPU fast path: Adam applied inside the backward kernel, no gradient tensors at all (but xyz's under depth supervision)
            fn = L.gslic_rasterize_backward_depth_adam if depth else L.gslic_rasterize_backward_adam
            tail = (None, p(xyz_grad) if depth else None, None, None, None, None, erank, ctypes.byref(adam))
            if grad_stats is not None:   # the same call plus the statistics descriptor
                fn = L.gslic_rasterize_backward_depth_adam_stats if depth else L.gslic_rasterize_backward_adam_stats
                tail += (ctypes.byref(grad_stats),)
            elif cam_adam:               # the same call plus the three camera outputs and the optional dL_dmean2D
                fn = L.gslic_rasterize_backward_depth_camera_adam if depth else L.gslic_rasterize_backward_camera_adam
                tail += (p(cam[0]), p(cam[1]), p(cam[2]), p(mean2d_out))
        elif rgb_out is not None and rows is not None:
            # chunked (gslic_rasterize_backward_rgb_rows): Gaussians [rows[0], rows[1]) only; the kernels index the gradient pointers by the
            # ABSOLUTE Gaussian index, so a caller that keeps its chunks in separate blocks passes `out_addr` = {name: address of row 0}
            addr = out_addr or {k: out[k].data_ptr() for k in ("opacity", "xyz", "scaling", "rotation")}
            rgb_addr = (out_addr or {}).get("rgb", rgb_out.data_ptr())
            fn = L.gslic_rasterize_backward_rgb_rows
            tail = (vp(addr["opacity"]), vp(addr["xyz"]), vp(rgb_addr), vp(addr["scaling"]), vp(addr["rotation"]), erank, int(rows[0]), int(rows[1]),
                    int(bool(skip_blend)))
        elif rgb_out is not None:
            # N > 1 exchange: the clamp-masked colour gradient [P,3] is written instead of dL_ddc / dL_dsh, and the rest of the rank's all-gather
            # payload (mask, camera centre) by the same kernel (no compare / copy launches)
            pay_vis, pay_campos = (payload or (None, None))
            fn = L.gslic_rasterize_backward_rgb_payload
            tail = (p(out["opacity"]), p(out["xyz"]), p(rgb_out), p(out["scaling"]), p(out["rotation"]), erank, p(pay_vis), p(pay_campos))
        else:
            tail = (p(dL_dmeans2D), p(dL_dconic), p(dL_dopacities), p(dL_dcolors), p(dL_dmeans3D), p(dL_dcov3D), p(dL_ddc), p(dL_dsh), p(dL_dscales),
                    p(dL_drotations), erank)
            if camera_grads:
                cam = (torch.empty(16, device=dev), torch.empty(16, device=dev), torch.empty(3, device=dev))
                fn = L.gslic_rasterize_backward_depth_camera if depth else L.gslic_rasterize_backward_camera
                tail += (p(cam[0]), p(cam[1]), p(cam[2]))
            else:
                fn = L.gslic_rasterize_backward_depth if depth else L.gslic_rasterize_backward
        _lib.check(fn(*head, *tail, _lib.current_stream_ptr()))
    elif full and camera_grads:
        cam = (torch.zeros(16, device=dev), torch.zeros(16, device=dev), torch.zeros(3, device=dev))
    if not full:
        return cam if cam_adam else None
    res = (dL_dmeans2D, dL_dcolors, dL_dopacities, dL_dmeans3D, dL_dcov3D, dL_ddc, dL_dsh, dL_dscales, dL_drotations)
    return res + cam if camera_grads else res


def rasterize_gaussians_backward(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                                 projmatrix, tan_fovx, tan_fovy, limx_neg, limx_pos, limy_neg, limy_pos, dL_dout_color, dc, sh,
                                 degree, campos, geomBuffer, R, binningBuffer, imageBuffer, B, sampleBuffer, lambda_erank, debug,
                                 raw_params=False, out=None, adam=None, camera_grads=False, rgb_out=None, rows=None, skip_blend=False,
                                 out_addr=None, payload=None, grad_stats=None, mean2d_out=None, cam_out=None):
    """RasterizeGaussiansBackwardCUDA (rasterize_points.cu:151-246): returns (dL_dmeans2D, dL_dcolors_precomp,
    dL_dopacities, dL_dmeans3D, dL_dcov3Ds_precomp, dL_ddc, dL_dsh, dL_dscales, dL_drotations).
    raw_params=True: scales / rotations are raw and dL_dopacities / dL_dscales / dL_drotations are w.r.t. the raw parameters.
    out: caller-provided storage for the six parameter gradients (dict xyz / features_dc / features_rest / opacity / scaling / rotation); the
    four the host discards are then not materialised.
    adam (a gslic_adam_fused descriptor, raw_params implied): gslic_rasterize_backward_adam, the Adam update inside the backward; returns None.
    rgb_out [P,3] (with out; returns None): gslic_rasterize_backward_rgb_payload, or with rows=(p0, p1) gslic_rasterize_backward_rgb_rows.
    camera_grads=True (gslic_rasterize_backward_camera; no reference counterpart): three more tensors are appended —
    dL_dviewmatrix [16], dL_dprojmatrix [16], dL_dcampos [3], element order of the inputs.  With adam as well
    (gslic_rasterize_backward_camera_adam): the Adam update inside the backward, the three returned alone (views of cam_out [35] when given).
    grad_stats (a _lib.GradStats, with adam): gslic_rasterize_backward_adam_stats.  mean2d_out [P,3] (with out): dL_dmeans2D is written there."""
    view = (dL_dout_color.size(1), dL_dout_color.size(2), tan_fovx, tan_fovy, limx_neg, limx_pos, limy_neg, limy_pos, scale_modifier)
    return _backward(view, degree, debug, raw_params, background, means3D, radii, colors, scales, rotations, cov3D_precomp, viewmatrix, projmatrix,
                     campos, dL_dout_color, None, dc, sh, geomBuffer, R, binningBuffer, imageBuffer, B, sampleBuffer, lambda_erank, out=out, adam=adam,
                     camera_grads=camera_grads, rgb_out=rgb_out, rows=rows, skip_blend=skip_blend, out_addr=out_addr, payload=payload,
                     grad_stats=grad_stats, mean2d_out=mean2d_out, cam_out=cam_out)


def rasterize_gaussians_backward_depth(background, means3D, radii, scales, rotations, scale_modifier, viewmatrix, projmatrix, tan_fovx,
                                       tan_fovy, limx_neg, limx_pos, limy_neg, limy_pos, dL_dout_color, dL_dout_depth, dc, sh, degree, campos,
                                       geomBuffer, R, binningBuffer, imageBuffer, B, sampleBuffer, lambda_erank=0.0, debug=False, raw_params=False,
                                       out=None, adam=None, xyz_grad=None, camera_grads=False, grad_stats=None, mean2d_out=None, cam_out=None):
    """gslic_rasterize_backward_depth: rasterize_gaussians_backward with dL/d(out_depth) [H,W] as a second input, on the buffers of
    rasterize_gaussians_depth (or rasterize_gaussians_depth_capacity: pass its cap_R / cap_B as R / B).  Returns the same nine tensors
    (dL_dmeans2D, dL_dcolors, dL_dopacities, dL_dmeans3D, dL_dcov3D, dL_ddc, dL_dsh, dL_dscales, dL_drotations); dL_dout_depth = 0 gives
    rasterize_gaussians_backward's results bit for bit.
    out: caller-provided storage for the six parameter gradients (dict xyz / features_dc / features_rest / opacity / scaling / rotation, as
    rasterize_gaussians_backward's `out`); the four the host discards are then not materialised.
    adam (a gslic_adam_fused descriptor, raw_params implied): gslic_rasterize_backward_depth_adam — the Adam update inside the backward,
    bit-identical to this backward followed by the masked Adam step; returns None.  xyz_grad [P,3]: where the xyz gradient is assembled before
    its update (allocated when None; a graph-captured step passes a buffer of its own).
    camera_grads=True (gslic_rasterize_backward_depth_camera): three more tensors are appended — dL_dviewmatrix [16], dL_dprojmatrix [16],
    dL_dcampos [3] of the colour AND depth loss, as rasterize_gaussians_backward(camera_grads=True) does.  With adam as well
    (gslic_rasterize_backward_depth_camera_adam): returns the three alone, views of cam_out [35] when given; mean2d_out is written too.
    grad_stats (with adam): gslic_rasterize_backward_depth_adam_stats.  mean2d_out [P,3] (with out): dL_dmeans2D is written there."""
    view = (dL_dout_color.size(1), dL_dout_color.size(2), tan_fovx, tan_fovy, limx_neg, limx_pos, limy_neg, limy_pos, scale_modifier)
    return _backward(view, degree, debug, raw_params, background, means3D, radii, None, scales, rotations, None, viewmatrix, projmatrix, campos,
                     dL_dout_color, dL_dout_depth, dc, sh, geomBuffer, R, binningBuffer, imageBuffer, B, sampleBuffer, lambda_erank, out=out, adam=adam,
                     camera_grads=camera_grads, xyz_grad=xyz_grad, grad_stats=grad_stats, mean2d_out=mean2d_out, cam_out=cam_out)


def _depth_grads(ctx, dL_dcolor, dL_ddepth, xyz, dc, sh, opacity, scaling, rotation, radii, geom, binning, img, sample, raw):
    rs = ctx.rs
    if dL_dcolor is None:
        dL_dcolor = torch.zeros(3, rs.image_height, rs.image_width, dtype=torch.float32, device=xyz.device)
    if dL_ddepth is None:
        dL_ddepth = torch.zeros(rs.image_height, rs.image_width, dtype=torch.float32, device=xyz.device)
    return rasterize_gaussians_backward_depth(
        rs.bg, xyz, radii, scaling, rotation, rs.scale_modifier, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.limx_neg,
        rs.limx_pos, rs.limy_neg, rs.limy_pos, dL_dcolor, dL_ddepth, dc, sh, rs.sh_degree, rs.campos, geom, ctx.R, binning, img, ctx.B,
        sample, rs.lambda_erank, False, raw_params=raw)


class GaussianRasterizerDepthFunction(torch.autograd.Function):
    """GaussianRasterizerFunction plus a differentiable depth image (activated parameters): forward returns (color, radii, final_T, depth)."""

    @staticmethod
    def forward(ctx, means3D, means2D, dc, sh, opacities, scales, rotations, rs):
        (R, B, color, final_T, depth, radii, geom, binning, img, sample) = rasterize_gaussians_depth(
            rs.bg, means3D, opacities, scales, rotations, rs.scale_modifier, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy,
            rs.image_height, rs.image_width, rs.limx_neg, rs.limx_pos, rs.limy_neg, rs.limy_pos, dc, sh, rs.sh_degree, rs.campos,
            rs.prefiltered, rs.debug, tie_rank=rs.tie_rank)
        ctx.rs, ctx.R, ctx.B = rs, R, B
        ctx.save_for_backward(means3D, dc, sh, opacities, scales, rotations, radii, geom, binning, img, sample)
        ctx.mark_non_differentiable(radii, final_T)
        return color, radii, final_T, depth

    @staticmethod
    def backward(ctx, dL_dcolor, _dL_dradii, _dL_dfinal_T, dL_ddepth):
        means3D, dc, sh, opacities, scales, rotations, radii, geom, binning, img, sample = ctx.saved_tensors
        g = _depth_grads(ctx, dL_dcolor, dL_ddepth, means3D, dc, sh, opacities, scales, rotations, radii, geom, binning, img, sample, False)
        (dL_dmeans2D, _dL_dcolors, dL_dopacities, dL_dmeans3D, _dL_dcov3D, dL_ddc, dL_dsh, dL_dscales, dL_drotations) = g
        return (dL_dmeans3D, dL_dmeans2D, dL_ddc, dL_dsh, dL_dopacities, dL_dscales, dL_drotations, None)


class RawGaussianRasterizerDepthFunction(torch.autograd.Function):
    """RawGaussianRasterizerFunction plus a differentiable depth image (raw parameters): forward returns (color, radii, final_T, depth)."""

    @staticmethod
    def forward(ctx, xyz, dc, sh, opacity_raw, scaling_raw, rotation_raw, rs):
        (R, B, color, final_T, depth, radii, geom, binning, img, sample) = rasterize_gaussians_depth(
            rs.bg, xyz, opacity_raw, scaling_raw, rotation_raw, rs.scale_modifier, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy,
            rs.image_height, rs.image_width, rs.limx_neg, rs.limx_pos, rs.limy_neg, rs.limy_pos, dc, sh, rs.sh_degree, rs.campos,
            rs.prefiltered, rs.debug, raw_params=True, tie_rank=rs.tie_rank)
        ctx.rs, ctx.R, ctx.B = rs, R, B
        ctx.save_for_backward(xyz, dc, sh, opacity_raw, scaling_raw, rotation_raw, radii, geom, binning, img, sample)
        ctx.mark_non_differentiable(radii, final_T)
        return color, radii, final_T, depth

    @staticmethod
    def backward(ctx, dL_dcolor, _dL_dradii, _dL_dfinal_T, dL_ddepth):
        xyz, dc, sh, opacity_raw, scaling_raw, rotation_raw, radii, geom, binning, img, sample = ctx.saved_tensors
        g = _depth_grads(ctx, dL_dcolor, dL_ddepth, xyz, dc, sh, opacity_raw, scaling_raw, rotation_raw, radii, geom, binning, img, sample, True)
        (_m2, _c, dL_dopacity, dL_dxyz, _cov, dL_ddc, dL_dsh, dL_dscaling, dL_drotation) = g
        if ctx.rs.mean2d_grad_out is not None:
            ctx.rs.mean2d_grad_out.copy_(_m2)
        return (dL_dxyz, dL_ddc.view_as(dc), dL_dsh.view_as(sh), dL_dopacity.view_as(opacity_raw), dL_dscaling, dL_drotation, None)


class GaussianRasterizerFunction(torch.autograd.Function):
    """rasterizer.cpp:21-183.  forward returns (color, radii, final_T); only d/dcolor flows back."""

    @staticmethod
    def forward(ctx, means3D, means2D, dc, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, rs):
        (R, B, color, final_T, radii, geom, binning, img, sample) = rasterize_gaussians(
            rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp, rs.viewmatrix,
            rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, rs.limx_neg, rs.limx_pos, rs.limy_neg,
            rs.limy_pos, dc, sh, rs.sh_degree, rs.campos, rs.prefiltered, rs.debug, rs.no_color, tie_rank=rs.tie_rank)
        ctx.rs, ctx.R, ctx.B = rs, R, B
        ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, dc, sh, geom, binning, img, sample)
        ctx.mark_non_differentiable(radii, final_T)
        return color, radii, final_T

    @staticmethod
    def backward(ctx, dL_dcolor, _dL_dradii, _dL_dfinal_T):
        rs = ctx.rs
        colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, dc, sh, geom, binning, img, sample = ctx.saved_tensors
        (dL_dmeans2D, dL_dcolors_precomp, dL_dopacities, dL_dmeans3D, dL_dcov3Ds_precomp, dL_ddc, dL_dsh, dL_dscales,
         dL_drotations) = rasterize_gaussians_backward(
            rs.bg, means3D, radii, colors_precomp, scales, rotations, rs.scale_modifier, cov3Ds_precomp, rs.viewmatrix,
            rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.limx_neg, rs.limx_pos, rs.limy_neg, rs.limy_pos, dL_dcolor, dc, sh,
            rs.sh_degree, rs.campos, geom, ctx.R, binning, img, ctx.B, sample, rs.lambda_erank, False)
        return (dL_dmeans3D, dL_dmeans2D, dL_ddc, dL_dsh, None, dL_dopacities, dL_dscales, dL_drotations, None, None)


class GaussianRasterizer(torch.nn.Module):
    """rasterizer.cpp:185-216."""

    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def forward(self, means3D, means2D, opacities, dc, shs, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None):
        dev = means3D.device
        colors_precomp = torch.empty(0, device=dev)   # rasterizer.cpp:200-201: always empty
        cov3D_precomp = torch.empty(0, device=dev)
        return GaussianRasterizerFunction.apply(means3D, means2D, dc, shs, colors_precomp, opacities, scales, rotations,
                                                cov3D_precomp, self.raster_settings)


class RawGaussianRasterizerFunction(torch.autograd.Function):
    """The autograd node behind render(): same forward / backward as GaussianRasterizerFunction (rasterizer.cpp:21-183), but on the model's
    RAW leaf tensors — sigmoid(opacity_), exp(scaling_), normalize(rotation_) of gaussian.cpp:147-175 run inside preprocess / preprocess_bwd
    (raw_params = 1), so the six LibTorch elementwise launches of the activations, the ten of their backward nodes and the zeros_like of the
    screen-space points disappear from the step.  Gradients are w.r.t. the raw tensors: exactly what autograd would have chained to.
    Only the six gradients the host's optimiser reads are materialised (rasterizer.cpp:171-182 discards the other four)."""

    @staticmethod
    def forward(ctx, xyz, dc, sh, opacity_raw, scaling_raw, rotation_raw, rs):
        e = torch.empty(0, device=xyz.device)
        (R, B, color, final_T, radii, geom, binning, img, sample) = rasterize_gaussians(
            rs.bg, xyz, e, opacity_raw, scaling_raw, rotation_raw, rs.scale_modifier, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy,
            rs.image_height, rs.image_width, rs.limx_neg, rs.limx_pos, rs.limy_neg, rs.limy_pos, dc, sh, rs.sh_degree, rs.campos, rs.prefiltered,
            rs.debug, rs.no_color, raw_params=True, tie_rank=rs.tie_rank)
        ctx.rs, ctx.R, ctx.B = rs, R, B
        ctx.save_for_backward(xyz, dc, sh, opacity_raw, scaling_raw, rotation_raw, radii, geom, binning, img, sample)
        ctx.mark_non_differentiable(radii, final_T)
        return color, radii, final_T

    @staticmethod
    def backward(ctx, dL_dcolor, _dL_dradii, _dL_dfinal_T):
        rs = ctx.rs
        xyz, dc, sh, opacity_raw, scaling_raw, rotation_raw, radii, geom, binning, img, sample = ctx.saved_tensors
        e = torch.empty(0, device=xyz.device)
        out = dict(xyz=torch.empty_like(xyz), features_dc=torch.empty_like(dc), features_rest=torch.empty_like(sh), opacity=torch.empty_like(opacity_raw),
                   scaling=torch.empty_like(scaling_raw), rotation=torch.empty_like(rotation_raw))   # (every row is written by the kernel)
        rasterize_gaussians_backward(rs.bg, xyz, radii, e, scaling_raw, rotation_raw, rs.scale_modifier, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx,
                                     rs.tanfovy, rs.limx_neg, rs.limx_pos, rs.limy_neg, rs.limy_pos, dL_dcolor, dc, sh, rs.sh_degree, rs.campos, geom, ctx.R,
                                     binning, img, ctx.B, sample, rs.lambda_erank, False, raw_params=True, out=out, mean2d_out=rs.mean2d_grad_out)
        return out["xyz"], out["features_dc"], out["features_rest"], out["opacity"], out["scaling"], out["rotation"], None


def _raw_leaves(model):
    """The six raw parameter tensors of a GaussianModel (xyz_, features_dc_, features_rest_, opacity_, scaling_, rotation_: gaussian.h:153-158),
    or None when the model only offers the activated accessors."""
    # An explicit marker, not duck typing: a model whose attributes of these names hold ACTIVATED values would otherwise be
    # activated a second time.  trainer.GaussianModel sets raw_parameter_leaves = True; any other model opts in by providing raw_leaves().
    if callable(getattr(model, "raw_leaves", None)):
        return tuple(model.raw_leaves())
    names = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")
    if getattr(model, "raw_parameter_leaves", False) and all(torch.is_tensor(getattr(model, n, None)) for n in names):
        return tuple(getattr(model, n) for n in names)
    return None


def render(camera, model, bg_color, no_color=False, scaling_modifier=1.0, raw=None, return_depth=False, mean2d_grad_out=None):
    """renderer.cpp:21-88 — same signature, same five results (image, final_T, screenspace_points, visible, radii).  `camera` =
    gaussian_lic_amd.camera.Camera with device tensors attached via to_device(); `model` exposes get_xyz / get_opacity / get_scaling /
    get_rotation / get_features_dc / get_features_rest, sh_degree, lambda_erank.

    raw (default: on whenever the model exposes its raw leaf tensors; GSLIC_RENDER_RAW=0 turns it off): the renderer feeds the RAW parameters to
    one autograd node whose kernels apply the activations (RawGaussianRasterizerFunction) instead of calling getOpacity() / getScaling() /
    getRotation() (renderer.cpp:57-63).  Image and gradients equal the operator path's up to fp32 rounding of the activation chain
    (tests/test_fused_gpu.py).  screenspace_points is then a zero-stride view of one zero row: the reference allocates and zero-fills
    [P,3] for a gradient (dL_dmeans2D) no caller of render() reads (gaussian.cpp:506,683,757,797); raw=False restores it.

    return_depth=True (not in the reference; LiDAR depth supervision): a sixth result, depth [H,W] = sum T alpha z over exactly the
    contributors of the pixel's colour (z = view-space depth of the Gaussian), differentiable on the raw and the activated path.  It is
    NOT normalised: the background contributes 0, and depth / (1 - final_T) is the expected depth of the covered part.  The five other
    results are bit-identical to return_depth=False's.  Needs the colour (no_color=False).

    mean2d_grad_out (not in the reference; float32 [P,3] on the device): on the raw path, whose screenspace_points carries no gradient, the backward
    writes dL_dmeans2D there (what screenspace_points.grad holds on the raw=False path) — the input of the gradient densification statistics."""
    import os
    leaves = _raw_leaves(model)
    if raw is None:
        raw = leaves is not None and os.environ.get("GSLIC_RENDER_RAW", "1") != "0"
    rs = GaussianRasterizationSettings(
        camera.image_height, camera.image_width, float(camera.tanfovx), float(camera.tanfovy), float(camera.limx_neg),
        float(camera.limx_pos), float(camera.limy_neg), float(camera.limy_pos), bg_color, scaling_modifier,
        camera.d_world_view_transform, camera.d_full_proj_transform, model.sh_degree, camera.d_camera_center, False, False,
        no_color, model.lambda_erank, getattr(model, "tie_rank", None), mean2d_grad_out)
    if raw and leaves is None:
        raise TypeError("render(raw=True): the model does not expose its raw parameter leaves (set raw_parameter_leaves = True on a model whose "
                        "xyz / features_dc / features_rest / opacity / scaling / rotation attributes are the PRE-activation tensors, or provide raw_leaves())")
    if return_depth and no_color:
        raise ValueError("render(return_depth=True) needs the colour (no_color=False)")
    depth = ()
    if raw:
        xyz, dc, rest, opacity, scaling, rotation = leaves
        if return_depth:
            image, radii, final_T, *depth = RawGaussianRasterizerDepthFunction.apply(xyz, dc, rest, opacity, scaling, rotation, rs)
        else:
            image, radii, final_T = RawGaussianRasterizerFunction.apply(xyz, dc, rest, opacity, scaling, rotation, rs)
        screenspace_points = torch.zeros(1, 3, dtype=xyz.dtype, device=xyz.device).expand(xyz.shape[0], 3)
        return (image, final_T, screenspace_points, radii > 0, radii, *depth)
    xyz = model.get_xyz()
    screenspace_points = torch.zeros_like(xyz, requires_grad=True)
    if return_depth:
        image, radii, final_T, *depth = GaussianRasterizerDepthFunction.apply(
            xyz, screenspace_points, model.get_features_dc(), model.get_features_rest(), model.get_opacity(), model.get_scaling(),
            model.get_rotation(), rs)
    else:
        image, radii, final_T = GaussianRasterizer(rs)(xyz, screenspace_points, model.get_opacity(), model.get_features_dc(),
                                                       model.get_features_rest(), None, model.get_scaling(), model.get_rotation(), None)
    return (image, final_T, screenspace_points, radii > 0, radii, *depth)


def sh_grad_from_rgb(means3D, campos_all, rgb_all, degree, dL_ddc, dL_dsh, input_is_ddc=False, n_views=None, view_stride=0):
    """gslic_sh_grad_from_rgb: dL_ddc [P,1,3] and dL_dsh [P,M,3] summed over the views from the views' masked colour gradients
    rgb_all [n_views,P,3] and camera centres campos_all [n_views,3] (all device fp32, contiguous); written in place.
    view_stride > 0 (floats): rgb_all / campos_all point at view 0's block inside an all-gathered payload, n_views blocks view_stride apart."""
    P = means3D.size(0)
    n = rgb_all.size(0) if n_views is None else int(n_views)
    M = dL_dsh.size(1) if dL_dsh is not None and dL_dsh.numel() else 0
    assert dL_ddc.is_contiguous() and (M == 0 or dL_dsh.is_contiguous())
    if not view_stride:
        assert rgb_all.is_contiguous() and campos_all.is_contiguous() and tuple(rgb_all.shape) == (n, P, 3) and tuple(campos_all.shape) == (n, 3)
    p = _lib.ptr
    _lib.check(_lib.lib().gslic_sh_grad_from_rgb(P, int(degree), M, n, p(_f32c(means3D)), p(campos_all), p(rgb_all), int(bool(input_is_ddc)), p(dL_ddc),
                                                 p(dL_dsh) if M else None, int(view_stride), _lib.current_stream_ptr()))


def grad_stats_descriptor(grad_sum, n_seen, max_radius, P):
    """The _lib.GradStats (gslic_grad_stats) of three device accumulators of at least P rows: float32, int32 (uint32 bits), int32."""
    for t, dt in ((grad_sum, torch.float32), (n_seen, torch.int32), (max_radius, torch.int32)):
        if not (torch.is_tensor(t) and t.is_contiguous() and t.dtype == dt and t.numel() >= int(P)):
            raise ValueError(f"gradient statistics: an accumulator must be a contiguous {dt} tensor of at least {int(P)} rows")
    return _lib.GradStats(grad_sum.data_ptr(), n_seen.data_ptr(), max_radius.data_ptr())


def gradient_stats_accumulate(dL_dmean2D, radii, grad_sum, n_seen, max_radius, rows=None):
    """gslic_gradient_stats_accumulate: applies the rule of the gradient densification statistics (include/gslic_hip.h) to a dL_dmeans2D [P,3] and
    radii [P] the caller already has — rows [rows[0], rows[1]) or all — adding into grad_sum float32 / n_seen int32 / max_radius int32 [>= P].
    One launch on the current stream, no synchronisation; bit-identical to the fused backward's own accumulation on the same gradient."""
    P = int(radii.shape[0])
    if not (dL_dmean2D.is_contiguous() and dL_dmean2D.dtype == torch.float32 and dL_dmean2D.numel() >= 3 * P):
        raise ValueError(f"gradient_stats_accumulate: dL_dmean2D must be a contiguous float32 tensor of at least {P} rows of 3")
    if not (radii.is_contiguous() and radii.dtype == torch.int32):
        raise ValueError("gradient_stats_accumulate: radii must be a contiguous int32 tensor")
    gs = grad_stats_descriptor(grad_sum, n_seen, max_radius, P)
    r0, r1 = (0, -1) if rows is None else (int(rows[0]), int(rows[1]))
    _lib.check(_lib.lib().gslic_gradient_stats_accumulate(P, _lib.ptr(dL_dmean2D), _lib.ptr(radii), ctypes.byref(gs), r0, r1, _lib.current_stream_ptr()))


def contribution_accumulate(P, H, W, R, B, geom, binning, img, w_min, max_w=None, n_pix=None, sum_w=None, error=None, err_sum=None,
                            near_bound=None, free_sum=None, meas_sum=None):
    """gslic_contribution_accumulate: adds ONE view's per-Gaussian contribution statistics, replayed from the buffers of a completed forward
    (rasterize_gaussians / _depth / _capacity / _depth_capacity; R, B as that forward returned them), to the caller's accumulators —
    max_w int32 [>= P] (float bits), n_pix int32 [>= P], sum_w int64 [>= P] (32.32 fixed point), device tensors indexed by storage row, any of
    them None.  The rule is written out in include/gslic_hip.h.  One launch on the current stream, no synchronisation.
    error (float32 [H, W] device tensor) together with err_sum (int64 [>= P], 32.32 fixed point) takes gslic_contribution_accumulate_error: the
    same launch, which also adds sum w e(p) to err_sum (e = error clamped to [0, 4], NaN and negative values read as 0).
    near_bound (float32 [H, W] device tensor) together with free_sum and meas_sum (int64 [>= P], 32.32 fixed point) takes
    gslic_contribution_accumulate_free_space instead: meas_sum += sum of w over the pixels with near_bound > 0, free_sum += sum of w over those of
    them with the Gaussian's view depth < near_bound.  One call takes one of the two images (they are two entry points)."""
    if (error is None) != (err_sum is None):
        raise ValueError("contribution_accumulate: error and err_sum go together")
    if not ((near_bound is None) == (free_sum is None) == (meas_sum is None)):
        raise ValueError("contribution_accumulate: near_bound, free_sum and meas_sum go together")
    if error is not None and near_bound is not None:
        raise ValueError("contribution_accumulate: error and near_bound are two launches (call twice, the second with max_w = n_pix = sum_w = None)")
    if near_bound is not None and not (near_bound.is_contiguous() and near_bound.dtype == torch.float32 and tuple(near_bound.shape) == (int(H), int(W))
                                       and near_bound.device == free_sum.device):
        raise ValueError(f"contribution_accumulate: near_bound must be a contiguous float32 [{int(H)}, {int(W)}] tensor on the accumulators' device")
    if error is not None and not (error.is_contiguous() and error.dtype == torch.float32 and tuple(error.shape) == (int(H), int(W)) and error.device == err_sum.device):
        raise ValueError(f"contribution_accumulate: error must be a contiguous float32 [{int(H)}, {int(W)}] tensor on the accumulators' device")
    for t, dt in ((max_w, torch.int32), (n_pix, torch.int32), (sum_w, torch.int64), (err_sum, torch.int64), (free_sum, torch.int64), (meas_sum, torch.int64)):
        if t is not None and not (t.is_contiguous() and t.dtype == dt and t.numel() >= int(P)):
            raise ValueError(f"contribution_accumulate: an accumulator must be a contiguous {dt} tensor of at least {int(P)} rows")
    prm = _params(P, 0, 0, H, W, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, False, False, False)   # (only P, W and H are read)
    bp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    if error is not None:
        _lib.check(_lib.lib().gslic_contribution_accumulate_error(ctypes.byref(prm), int(R), int(B), bp(geom), bp(binning), bp(img), float(w_min),
                                                                  bp(max_w), bp(n_pix), bp(sum_w), bp(error), bp(err_sum), _lib.current_stream_ptr()))
        return
    if near_bound is not None:
        _lib.check(_lib.lib().gslic_contribution_accumulate_free_space(ctypes.byref(prm), int(R), int(B), bp(geom), bp(binning), bp(img), float(w_min),
                                                                       bp(max_w), bp(n_pix), bp(sum_w), bp(near_bound), bp(free_sum), bp(meas_sum),
                                                                       _lib.current_stream_ptr()))
        return
    _lib.check(_lib.lib().gslic_contribution_accumulate(ctypes.byref(prm), int(R), int(B), bp(geom), bp(binning), bp(img), float(w_min), bp(max_w),
                                                        bp(n_pix), bp(sum_w), _lib.current_stream_ptr()))


GEOMETRY_IMAGES = ("transmittance", "opacity", "depth_sum", "depth_norm", "depth_median", "top_row", "top_weight")   # the argument order of the export


def geometry_images(P, H, W, R, B, geom, binning, img, a_min, out):
    """gslic_geometry_images: ONE view's per-pixel geometry, replayed from the buffers of a completed forward (rasterize_gaussians / _depth /
    _capacity / _depth_capacity; R, B as that forward returned them), written into the caller's images.  out: a dict of contiguous device tensors
    of H * W elements keyed by the names of GEOMETRY_IMAGES — float32, top_row int32; a name that is absent (or None) is not computed.  Every
    pixel of every image given is written (a capacity forward whose status reports an overflow writes nothing).  The rule is written out in
    include/gslic_hip.h.  One launch on the current stream, no allocation, no synchronisation."""
    unknown = set(out) - set(GEOMETRY_IMAGES)
    if unknown:
        raise ValueError(f"geometry_images: unknown image(s) {sorted(unknown)}; the images are {GEOMETRY_IMAGES}")
    ptrs = []
    for name in GEOMETRY_IMAGES:
        t = out.get(name)
        dt = torch.int32 if name == "top_row" else torch.float32
        if t is not None and not (torch.is_tensor(t) and t.is_contiguous() and t.dtype == dt and t.numel() == int(H) * int(W) and t.numel() > 0):
            raise ValueError(f"geometry_images: {name} must be a contiguous {dt} tensor of {int(H)} x {int(W)} elements")
        ptrs.append(None if t is None else ctypes.c_void_p(t.data_ptr()))
    prm = _params(P, 0, 0, H, W, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, False, False, False)   # (only P, W and H are read)
    bp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    _lib.check(_lib.lib().gslic_geometry_images(ctypes.byref(prm), int(R), int(B), bp(geom), bp(binning), bp(img), float(a_min), *ptrs,
                                                _lib.current_stream_ptr()))


def debug_export(settings, P, M, R, B, geom, binning, img, sample, what=("tiles_touched", "point_list", "ranges")):
    """Test-only: copy stage boundaries out of the opaque scratch buffers (gslic_debug_export)."""
    L = _lib.lib()
    rs = settings
    dev = geom.device
    H, W = rs.image_height, rs.image_width
    T = ((W + 15) // 16) * ((H + 15) // 16)
    prm = _params(P, rs.sh_degree, M, H, W, rs.tanfovx, rs.tanfovy, rs.limx_neg, rs.limx_pos, rs.limy_neg, rs.limy_pos,
                  rs.scale_modifier, False, False, rs.no_color)
    out = {}
    mk = dict(
        tiles_touched=lambda: torch.zeros(P, dtype=torch.int32, device=dev),
        means2D=lambda: torch.zeros(P, 2, device=dev), depths=lambda: torch.zeros(P, device=dev),
        conic_opacity=lambda: torch.zeros(P, 4, device=dev), rgb=lambda: torch.zeros(P, 3, device=dev),
        sorted_keys=lambda: torch.zeros(max(R, 1), dtype=torch.int64, device=dev),
        point_list=lambda: torch.zeros(max(R, 1), dtype=torch.int32, device=dev),
        ranges=lambda: torch.zeros(T, 2, dtype=torch.int32, device=dev),
        n_contrib=lambda: torch.zeros(H, W, dtype=torch.int32, device=dev),
        max_contrib=lambda: torch.zeros(T, dtype=torch.int32, device=dev))
    order = ["tiles_touched", "means2D", "depths", "conic_opacity", "rgb", "sorted_keys", "point_list", "ranges", "n_contrib",
             "max_contrib"]
    args = []
    for k in order:
        if k in what:
            out[k] = mk[k]()
            args.append(ctypes.c_void_p(out[k].data_ptr()))
        else:
            args.append(None)
    bp = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None
    _lib.check(L.gslic_debug_export(ctypes.byref(prm), int(R), int(B), bp(geom), bp(binning), bp(img), bp(sample), *args,
                                    _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    for k in ("sorted_keys", "point_list"):
        if k in out:
            out[k] = out[k][:R]
    return out
