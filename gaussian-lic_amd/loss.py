"""Loss operators — mirrors src/loss_utils.h (l1_loss :30-33, FusedSSIMMap :130-193, psnr :35-39) on top of
gslic_fusedssim_forward/_backward (replacing src/fused-ssim/ssim.cu)."""
import torch

from . import _lib

C1 = 0.01 ** 2
C2 = 0.03 ** 2


def fusedssim(C1_, C2_, img1, img2, train):
    """fusedssim(C1, C2, img1, img2, train) -> (ssim_map, dm_dmu1, dm_dsigma1_sq, dm_dsigma12)  (ssim.h:7-15)."""
    img1, img2 = img1.contiguous(), img2.contiguous()
    B, CH, H, W = img1.shape
    m = torch.empty_like(img1)
    if train:
        d = [torch.empty_like(img1) for _ in range(3)]
    else:
        d = [torch.empty(0, device=img1.device) for _ in range(3)]
    p = _lib.ptr
    _lib.check(_lib.lib().gslic_fusedssim_forward(B, CH, H, W, float(C1_), float(C2_), p(img1), p(img2), p(m), p(d[0]), p(d[1]),
                                                  p(d[2]), _lib.current_stream_ptr()))
    return m, d[0], d[1], d[2]


def fusedssim_backward(C1_, C2_, img1, img2, dL_dmap, dm_dmu1, dm_dsigma1_sq, dm_dsigma12):
    """fusedssim_backward(...) -> dL_dimg1  (ssim.h:17-26)."""
    img1, img2, dL_dmap = img1.contiguous(), img2.contiguous(), dL_dmap.contiguous()
    B, CH, H, W = img1.shape
    out = torch.empty_like(img1)
    p = _lib.ptr
    _lib.check(_lib.lib().gslic_fusedssim_backward(B, CH, H, W, float(C1_), float(C2_), p(img1), p(img2), p(dL_dmap), p(dm_dmu1),
                                                   p(dm_dsigma1_sq), p(dm_dsigma12), p(out), _lib.current_stream_ptr()))
    return out


class FusedSSIMMap(torch.autograd.Function):
    """loss_utils.h:130-187 with padding == "same"."""

    @staticmethod
    def forward(ctx, C1_, C2_, img1, img2):
        m, d1, d2, d3 = fusedssim(C1_, C2_, img1, img2, True)
        ctx.save_for_backward(img1.detach(), img2, d1, d2, d3)
        ctx.C = (C1_, C2_)
        return m

    @staticmethod
    def backward(ctx, dL_dmap):
        img1, img2, d1, d2, d3 = ctx.saved_tensors
        grad = fusedssim_backward(ctx.C[0], ctx.C[1], img1, img2, dL_dmap, d1, d2, d3)
        return None, None, grad, None


def fused_ssim(img1, img2):
    """loss_utils.h:189-193."""
    return FusedSSIMMap.apply(C1, C2, img1, img2).mean()


def l1_loss(network_output, gt):
    """loss_utils.h:30-33."""
    return torch.abs(network_output - gt).mean()


def depth_weight(weight):
    """A per-pixel depth weight as the weighted depth loss kernels read it: NaN, negative and +inf values are 0; NO clamp at 1 (inverse-variance
    weights are not bounded by 1, and the loss divides by their sum)."""
    return torch.where((weight > 0) & (weight < float("inf")), weight, torch.zeros_like(weight))


def depth_l1(depth, gt_depth, weight=None, huber=0.0):
    """Masked L1 for LiDAR depth supervision: mean |depth - gt_depth| over the pixels where gt_depth > 0 (a sparse projected depth image,
    Camera.project_depth); 0 when there are none (still a tensor connected to `depth`, so backward() works).
    weight [H,W] (no gradient to it; depth_weight's reading) and huber = delta >= 0: the rule of gslic_depth_loss_weighted_forward_backward in
    torch ops — sum_m w rho / sum_m w over m = gt_depth > 0 and w > 0, rho the smooth-L1 of the residual with beta = delta (delta = 0: |r|);
    0 when the weights sum to 0.  With the defaults the graph and the bits are the ones above."""
    huber = float(huber)
    if not (0.0 <= huber < float("inf")):
        raise ValueError(f"depth_l1: huber = {huber} must be finite and >= 0")
    if weight is None and huber == 0.0:
        mask = gt_depth > 0
        n = mask.sum()
        diff = torch.where(mask, (depth - gt_depth).abs(), torch.zeros_like(depth))
        return diff.sum() / n.clamp_min(1).to(depth.dtype)
    mask = gt_depth > 0
    if weight is None:
        w = mask.to(depth.dtype)
    else:
        w = depth_weight(weight.detach().to(depth.dtype))
        mask = mask & (w > 0)
        w = torch.where(mask, w, torch.zeros_like(w))
    r = torch.where(mask, depth - gt_depth, torch.zeros_like(depth))   # (an unmeasured pixel's depth, NaN included, reaches neither value nor gradient)
    a = r.abs()
    rho = a if huber == 0.0 else torch.where(a < huber, ((0.5 * a) * a) / huber, a - 0.5 * huber)
    S = w.sum()
    T = (w * rho).sum()
    return torch.where(S > 0, T / S.clamp_min(torch.finfo(depth.dtype).tiny), torch.zeros_like(T))


def depth_metrics(depth, gt_depth, weight=None):
    """Depth evaluation over the measured pixels (gt_depth > 0; with weight [H,W], depth_weight's reading: the pixels of positive weight, each counted
    by its weight), accumulated in float64: dict of device scalars mae = mean |D - d|, rmse = sqrt(mean (D - d)^2), abs_rel = mean |D - d| / d,
    delta1 = share with max(D / d, d / D) < 1.25, n = the sum of the weights (the number of pixels without one).  All 0 when n == 0."""
    D, d = depth.detach().double(), gt_depth.detach().double()
    m = d > 0
    w = m.double() if weight is None else torch.where(m, depth_weight(weight.detach().double()), torch.zeros_like(d))
    m = w > 0
    one = torch.ones_like(d)
    D, d = torch.where(m, D, one), torch.where(m, d, one)
    e = (D - d).abs()
    S = w.sum()
    n = S.clamp_min(torch.finfo(torch.float64).tiny)
    ratio = torch.maximum(D / d, d / D)
    ok = ((ratio < 1.25) & (D > 0)).double()   # (a NaN or non-positive rendered depth fails)
    return dict(mae=(w * e).sum() / n, rmse=((w * e * e).sum() / n).sqrt(), abs_rel=(w * e / d).sum() / n, delta1=(w * ok).sum() / n, n=S)


def clamp_weight(weight):
    """A per-pixel weight image as the weighted loss kernels read it: NaN and negative values are 0, values above 1 (+inf included) are 1."""
    return torch.where(weight > 0, weight.clamp(max=1.0), torch.zeros_like(weight))


def psnr(img1, img2, weight=None):
    """loss_utils.h:35-39.  weight [H,W] (not in the reference): the MSE is the weighted mean sum_p w_p sum_c d^2 / (C sum_p w_p), so that an
    evaluation can leave out the pixels the training left out."""
    if weight is None:
        mse = torch.pow(img1 - img2, 2).mean()
    else:
        w = clamp_weight(weight.to(img1.dtype))
        mse = (torch.pow(img1 - img2, 2) * w).sum() / (img1.size(-3) * w.sum())
    return 10.0 * torch.log10(1.0 / mse)


def _gaussian_window(window_size, sigma, channel, like):
    """gaussian() + create_window() of loss_utils.h:41-74 (float math like the reference)."""
    import math
    import numpy as np
    # std::exp(-temp * temp / (2.0f * sigma * sigma)) with a float argument (loss_utils.h:50-51): the quotient is rounded to float BEFORE the exponential
    # (expf: correctly rounded here, like the double exp of the float argument rounded once); tests/golden/eval_*.npz hold the reference's window
    den = np.float32(2.0) * np.float32(sigma) * np.float32(sigma)
    g = torch.tensor([float(np.float32(math.exp(float(np.float32(-((x - window_size // 2) ** 2)) / den)))) for x in range(window_size)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    w2 = g.mm(g.t()).float().unsqueeze(0).unsqueeze(0)
    return w2.expand(channel, 1, window_size, window_size).contiguous().to(like.device).type_as(like)


def ssim(img1, img2, window_size=11, size_average=True):
    """Evaluation SSIM — loss_utils.h:80-128 (conv2d with an 11x11 Gaussian window, zero padding); used by
    evaluateVisualQuality (gaussian.cpp:721-831).  LibTorch conv2d stays the host's op, exactly as in the reference."""
    channel = img1.size(-3)
    window = _gaussian_window(window_size, 1.5, channel, img1)
    pad = window_size // 2
    conv = lambda x: torch.nn.functional.conv2d(x, window, padding=pad, groups=channel)
    mu1, mu2 = conv(img1), conv(img2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = conv(img1 * img1) - mu1_sq
    sigma2_sq = conv(img2 * img2) - mu2_sq
    sigma12 = conv(img1 * img2) - mu1_mu2
    c1, c2 = 0.01 * 0.01, 0.03 * 0.03
    ssim_map = ((2 * mu1_mu2 + c1) * (2 * sigma12 + c2)) / ((mu1_sq + mu2_sq + c1) * (sigma1_sq + sigma2_sq + c2))
    if size_average is None:
        return ssim_map                                         # (the map itself: evaluate_visual_quality's weighted mean)
    return ssim_map.mean() if size_average else ssim_map.mean(1).mean(1).mean(1)


def evaluate_visual_quality(model, cameras, gt_images, bg, fused=True, weights=None, gt_depths=None, depth_weights=None, depth_kind="sum",
                            depth_a_min=0.05, exposures=None, views=None):
    """PSNR / SSIM over a set of views — the metric part of evaluateVisualQuality (gaussian.cpp:751-789): render, clamp to [0,1],
    psnr + SSIM per image, averaged over the views.  fused=True evaluates the SSIM map with the fused-SSIM kernel
    (gslic_fusedssim_forward, train = 0: the same 11-tap sigma-1.5 window with zero padding as loss_utils.h:41-128, separable, one
    launch) instead of five LibTorch conv2d calls; fused=False is the reference's formulation verbatim.  Returns device scalars
    (mean PSNR, mean SSIM).  (LPIPS needs the TorchScript AlexNet blob the reference does not ship.)
    weights: one [H,W] weight image per view (or None per view): PSNR from the weighted MSE and SSIM as the weighted mean of the SSIM map
    (window statistics over all pixels, as in the weighted training loss), in plain torch on top of the same map.
    gt_depths: one [H,W] depth target per view (or None per view; depth_weights likewise, optional): the views that have one are rendered with
    their depth and the result gains a third element, the dict of depth_metrics averaged over those views (float64 device scalars).  Without
    gt_depths the result is the pair it always was.
    depth_kind: which rendered depth the metrics are taken of.  "sum" (the default): D = sum T alpha z, the image the depth loss trains on — biased
    low wherever the accumulated opacity is below 1.  "normalised": D / A where the accumulated opacity A >= depth_a_min, 0 elsewhere; "median": the
    view depth of the entry that takes the transmittance below one half (0: never reached) — both from trainer.geometry_images of the same view (one
    more forward and one replay launch per view with a depth target; a pixel whose depth is 0 fails delta1 and counts its full error).
    exposures (a trainer.Exposure) with views (one row index per camera): the image that is scored is the exposure-compensated one,
    clamp(E_view applied to the render) — what the training loss saw; the depth metrics are not touched.  By default the raw render is scored."""
    from .rasterizer import render
    if (exposures is None) != (views is None):
        raise ValueError("evaluate_visual_quality: exposures and views go together (one row index per camera)")
    if views is not None and len(views) != len(cameras):
        raise ValueError(f"evaluate_visual_quality: {len(views)} views for {len(cameras)} cameras")

    def shown(rendered, i):
        if exposures is None:
            return torch.clamp(rendered, 0.0, 1.0)
        rendered = rendered.contiguous()
        return torch.clamp(exposure_apply(rendered, exposures.matrix(views[i]), torch.empty_like(rendered)), 0.0, 1.0)

    kinds = {"sum": None, "normalised": "depth_norm", "median": "depth_median"}
    if depth_kind not in kinds:
        raise ValueError(f"evaluate_visual_quality: depth_kind must be one of {tuple(kinds)}, got {depth_kind!r}")
    ps, ss, dm = [], [], []
    with torch.no_grad():
        for i, (cam, gt) in enumerate(zip(cameras, gt_images)):
            gtd = None if gt_depths is None else gt_depths[i]
            if gtd is None:
                img = shown(render(cam, model, bg)[0], i)
            elif kinds[depth_kind] is not None:
                from .trainer import geometry_images
                img = shown(render(cam, model, bg)[0], i)
                geo = geometry_images(model, cam, bg, a_min=depth_a_min, what=(kinds[depth_kind],))
                dm.append(depth_metrics(geo[kinds[depth_kind]], gtd, None if depth_weights is None else depth_weights[i]))
            else:
                out = render(cam, model, bg, return_depth=True)
                img = shown(out[0], i)
                dm.append(depth_metrics(out[5], gtd, None if depth_weights is None else depth_weights[i]))
            gt = torch.clamp(gt, 0.0, 1.0)                      # gaussian.cpp:759
            w = None if weights is None else weights[i]
            ps.append(psnr(img, gt, w))
            if w is not None:
                m = (fusedssim(C1, C2, img.unsqueeze(0).contiguous(), gt.unsqueeze(0).contiguous(), False)[0] if fused
                     else ssim(img.unsqueeze(0), gt.unsqueeze(0), size_average=None))
                wc = clamp_weight(w.to(m.dtype))
                ss.append((m * wc).sum() / (m.size(-3) * wc.sum()))
            elif fused:
                ss.append(fusedssim(C1, C2, img.unsqueeze(0).contiguous(), gt.unsqueeze(0).contiguous(), False)[0].mean())
            else:
                ss.append(ssim(img.unsqueeze(0), gt.unsqueeze(0)))
    if gt_depths is None:
        return torch.stack(ps).mean(), torch.stack(ss).mean()
    if depth_weights is not None and not dm:
        raise ValueError("evaluate_visual_quality: depth_weights without a depth target in gt_depths")
    keys = ("mae", "rmse", "abs_rel", "delta1", "n")
    depth_result = {k: torch.stack([m[k] for m in dm]).mean() for k in keys} if dm else {}
    return torch.stack(ps).mean(), torch.stack(ss).mean(), depth_result


class _L1SsimLoss(torch.autograd.Function):
    """(1 - lambda) * l1_loss + lambda * (1 - fused_ssim) as ONE autograd node on gslic_l1_ssim_loss_forward / _backward: what
    gaussian.cpp:685-691 builds from l1_loss (loss_utils.h:30-33: sub, abs, mean), fused_ssim (:130-193: the map kernel + mean) and four
    scalar ops, with their backward nodes — two kernels forward, one backward.  dL/dimage equals the chain's bit for bit
    (tests/test_vs_reference_kernels_gpu.py::test_fused_loss_gradient_is_the_reference_chain_bit_for_bit) times the upstream scalar."""

    @staticmethod
    def forward(ctx, image, gt, lambda_dssim, weight=None):
        fl = FusedLoss(lambda_dssim)
        ctx.fl, ctx.shape = fl, image.shape
        img3, gt3 = image.reshape(image.shape[-3:]), gt.reshape(gt.shape[-3:])
        dL, terms = fl.forward_backward(img3, gt3, weight)
        ctx.save_for_backward(dL)
        return fl.value(terms)

    @staticmethod
    def backward(ctx, g):
        (dL,) = ctx.saved_tensors
        return (dL * g).reshape(ctx.shape), None, None, None


def l1_ssim_loss(image, gt, lambda_dssim=0.2, weight=None):
    """Optional one-call replacement for the loss lines of optimize() (gaussian.cpp:685-691): `loss = l1_ssim_loss(rendered_image, gt_image,
    lambda_dssim)`.  image, gt: [3,H,W] (or [1,3,H,W]).  weight [H,W]: the weighted loss of FusedLoss.forward_backward (no gradient to it)."""
    if weight is None:
        return _L1SsimLoss.apply(image, gt, float(lambda_dssim))
    return _L1SsimLoss.apply(image, gt, float(lambda_dssim), weight.detach())


def _exposure_args(image, E):
    if image.dim() != 3 or image.size(0) != 3 or image.dtype != torch.float32 or not image.is_contiguous():
        raise ValueError("exposure: the image must be a contiguous float32 [3,H,W] tensor")
    if E.numel() != 12 or E.dtype != torch.float32 or E.device != image.device or not E.is_contiguous():
        raise ValueError("exposure: E must be 12 contiguous float32 values ([3,4]) on the image's device")
    return int(image.size(1)), int(image.size(2))


def exposure_apply(image, E, out):
    """gslic_exposure_apply: out_c = ((E[c,0] r + E[c,1] g) + E[c,2] b) + E[c,3] on a planar [3,H,W] image, every step one float32 operation."""
    H, W = _exposure_args(image, E)
    p = _lib.ptr
    _lib.check(_lib.lib().gslic_exposure_apply(H, W, p(E), p(image), p(out), _lib.current_stream_ptr()))
    return out


def exposure_backward(image, E, dL_dout, dL_dimage, partials, dL_dE, adam=None):
    """gslic_exposure_backward: dL_dimage = E^T dL_dout and dL_dE [3,4] (twelve fixed-order sums over the pixels of dL_dout x [image | 1]) in two
    launches; adam (a _lib.ExposureAdam or None): the second launch also applies torch-style Adam to the row the descriptor names."""
    H, W = _exposure_args(image, E)
    if tuple(dL_dout.shape) != tuple(image.shape) or dL_dout.dtype != torch.float32 or not dL_dout.is_contiguous():
        raise ValueError("exposure: dL_dout must be a contiguous float32 tensor of the image's shape")
    import ctypes
    p = _lib.ptr
    _lib.check(_lib.lib().gslic_exposure_backward(H, W, p(E), p(image), p(dL_dout), p(dL_dimage), p(partials), p(dL_dE),
                                                  None if adam is None else ctypes.byref(adam), _lib.current_stream_ptr()))
    return dL_dimage


class _ApplyExposure(torch.autograd.Function):
    """gslic_exposure_apply / gslic_exposure_backward as one autograd node with gradients to the image and to E."""

    @staticmethod
    def forward(ctx, image, E):
        img3 = image.detach().reshape(image.shape[-3:]).contiguous()
        E12 = E.detach().contiguous()
        ctx.save_for_backward(img3, E12)
        ctx.shapes = (image.shape, E.shape)
        return exposure_apply(img3, E12, torch.empty_like(img3)).reshape(image.shape)

    @staticmethod
    def backward(ctx, g):
        img3, E12 = ctx.saved_tensors
        g3 = g.reshape(img3.shape).contiguous()
        dL_dimage, dL_dE = torch.empty_like(img3), torch.empty(12, device=img3.device)
        partials = torch.empty(int(_lib.lib().gslic_exposure_partials_count(img3.shape[1], img3.shape[2])), device=img3.device)
        exposure_backward(img3, E12, g3, dL_dimage, partials, dL_dE)
        return dL_dimage.reshape(ctx.shapes[0]), dL_dE.reshape(ctx.shapes[1])


def apply_exposure(image, E):
    """The exposure-compensated image E[:, :3] @ rgb + E[:, 3] of a rendered [3,H,W] (or [1,3,H,W]) image, differentiable in both arguments: for the
    autograd training_step and for a host that builds its own graph (`E` its own [3,4] leaf with its own optimiser, as the reference's exposure_
    and exposure_optimizer_).  Forward and backward are the two exports; the values are theirs bit for bit."""
    return _ApplyExposure.apply(image, E)


class FusedLoss:
    """loss = (1-lambda) * L1 + lambda * (1 - SSIM) of optimize() (gaussian.cpp:685-691) computed by two kernels
    (gslic_l1_ssim_loss_forward / _backward) with no LibTorch elementwise ops and no autograd graph; with LiDAR depth supervision
    (depth_forward_backward) + lambda_depth * L_d by two more.  The terms of a step live in one device tensor [mean L1, mean SSIM, L_d]:
    forward_backward returns its first two elements, depth_forward_backward the third, `terms3` all of them."""

    def __init__(self, lambda_dssim=0.2):
        self.lambda_dssim = float(lambda_dssim)
        self._shape, self._buf = None, None
        self._dshape, self._dbuf = None, None
        self._terms = None
        self._wshape, self._wbuf = None, None
        self._dwshape, self._dwbuf = None, None
        self._eshape, self._ebuf = None, None

    def _terms_buf(self, device):
        if self._terms is None or self._terms.device != device:
            self._terms = torch.zeros(3, device=device)
        return self._terms

    @property
    def terms3(self):
        """The device tensor [mean L1, mean SSIM, L_d] the last calls wrote (L_d: of the last depth_forward_backward)."""
        return self._terms

    def _scratch(self, img):
        if self._shape != tuple(img.shape) or self._buf[0].device != img.device:
            n = int(_lib.lib().gslic_loss_partials_count(1, img.shape[0], img.shape[1], img.shape[2]))
            self._buf = [torch.empty_like(img) for _ in range(4)] + [torch.empty(n, device=img.device), self._terms_buf(img.device)[:2]]
            self._shape = tuple(img.shape)
        return self._buf

    def _depth_scratch(self, depth):
        if self._dshape != tuple(depth.shape) or self._dbuf[0].device != depth.device:
            n = int(_lib.lib().gslic_depth_l1_loss_partials_count(depth.shape[0], depth.shape[1]))
            self._dbuf = [torch.empty_like(depth), torch.empty(n, device=depth.device), self._terms_buf(depth.device)[2:3]]
            self._dshape = tuple(depth.shape)
        return self._dbuf

    def depth_forward_backward(self, depth, gt_depth, lambda_depth, weight=None, huber=0.0):
        """depth, gt_depth: [H,W] (gt_depth 0 = no measurement).  Returns (dL/ddepth of lambda_depth * L_d, term) with term = device [1] view of
        L_d = depth_l1(depth, gt_depth) — gslic_depth_l1_loss_forward_backward, two launches; dL/ddepth equals autograd's bit for bit.
        weight [H,W] float32 (NaN, negative and +inf read as 0; NOT clamped at 1) and / or huber = delta > 0 (the smooth-L1 threshold, in the unit
        of depth): L_d = depth_l1(depth, gt_depth, weight, huber) and its gradient by gslic_depth_loss_weighted_forward_backward — two launches and
        a 4-byte copy into `terms3`; `depth_weight_sum` is then S, the sum of the weights over the measured pixels.  S == 0: L_d 0 and a zero
        gradient.  weight=None with huber == 0 is the call above, launch for launch."""
        depth, gt_depth = depth.contiguous(), gt_depth.contiguous()
        H, W = depth.shape
        assert tuple(gt_depth.shape) == (H, W), "gt_depth must have the depth image's shape [H,W]"
        huber = float(huber)
        p = _lib.ptr
        if weight is not None or huber != 0.0:
            if weight is not None:
                if tuple(weight.shape) != (H, W) or weight.dtype != torch.float32 or weight.device != depth.device:
                    raise ValueError(f"depth weight must be a float32 [H,W] = [{H},{W}] tensor on the depth image's device")
                weight = weight.contiguous()
            dL, _partials, term = self._depth_scratch(depth)
            wpartials, wterms = self._depth_weighted_scratch(depth)
            _lib.check(_lib.lib().gslic_depth_loss_weighted_forward_backward(H, W, float(lambda_depth), huber, p(depth), p(gt_depth), p(weight),
                                                                             p(wpartials), p(wterms), p(dL), _lib.current_stream_ptr()))
            term.copy_(wterms[:1])   # terms3 stays [L1, SSIM, L_d]; S is `depth_weight_sum`
            return dL, term
        dL, partials, term = self._depth_scratch(depth)
        _lib.check(_lib.lib().gslic_depth_l1_loss_forward_backward(H, W, float(lambda_depth), p(depth), p(gt_depth), p(partials), p(term), p(dL),
                                                                   _lib.current_stream_ptr()))
        return dL, term

    @property
    def depth_weight_sum(self):
        """S = sum of the depth weights over the measured pixels of the last depth_forward_backward(weight= / huber=): a device [1] view; None
        before the first such call."""
        return None if self._dwbuf is None else self._dwbuf[1][1:2]

    def _depth_weighted_scratch(self, depth):
        if self._dwshape != tuple(depth.shape) or self._dwbuf[0].device != depth.device:
            n = int(_lib.lib().gslic_depth_loss_weighted_partials_count(depth.shape[0], depth.shape[1]))
            self._dwbuf = [torch.empty(n, device=depth.device), torch.zeros(2, device=depth.device)]
            self._dwshape = tuple(depth.shape)
        return self._dwbuf

    @property
    def weight_sum(self):
        """S = sum of the (clamped) weights of the last forward_backward(weight=...): a device [1] view; None before the first such call."""
        return None if self._wbuf is None else self._wbuf[1][2:3]

    def _weighted_scratch(self, img):
        if self._wshape != tuple(img.shape) or self._wbuf[0].device != img.device:
            n = int(_lib.lib().gslic_l1_ssim_loss_weighted_partials_count(img.shape[0], img.shape[1], img.shape[2]))
            self._wbuf = [torch.empty(n, device=img.device), torch.zeros(3, device=img.device)]
            self._wshape = tuple(img.shape)
        return self._wbuf

    def forward_backward(self, image, gt, weight=None):
        """image, gt: [3,H,W].  Returns (dL/dimage, terms) with terms = device tensor [mean|img-gt|, mean ssim].
        weight [H,W] float (a mask is the 0/1 case; NaN and negative read as 0, above 1 as 1): the weighted loss — terms are the weighted means
        sum_p w_p sum_c (.) / (3 S), S = sum_p w_p (`weight_sum`), and dL/dimage their gradient (gslic_l1_ssim_loss_weighted_forward_backward:
        three launches and an 8-byte copy into `terms3`).  The SSIM window statistics still run over all pixels.  S == 0: terms 0, 0 and a zero
        gradient.  weight=None is the unweighted call, the same two launches as ever."""
        image, gt = image.contiguous(), gt.contiguous()
        CH, H, W = image.shape
        if weight is not None:
            if tuple(weight.shape) != (H, W) or weight.dtype != torch.float32 or weight.device != image.device:
                raise ValueError(f"weight must be a float32 [H,W] = [{H},{W}] tensor on the image's device")
            weight = weight.contiguous()
            d1, d2, d3, dL, _partials, terms = self._scratch(image)
            wpartials, wterms = self._weighted_scratch(image)
            p, L = _lib.ptr, _lib.lib()
            _lib.check(L.gslic_l1_ssim_loss_weighted_forward_backward(CH, H, W, C1, C2, self.lambda_dssim, p(image), p(gt), p(weight), p(d1), p(d2),
                                                                      p(d3), p(wpartials), p(wterms), p(dL), _lib.current_stream_ptr()))
            terms.copy_(wterms[:2])   # terms3 stays [L1, SSIM, L_d]; S is `weight_sum`
            return dL, terms
        d1, d2, d3, dL, partials, terms = self._scratch(image)
        p, L = _lib.ptr, _lib.lib()
        # (two launches: the reduction of the forward's partial sums rides on the backward kernel; gslic_l1_ssim_loss_forward + _backward are three)
        _lib.check(L.gslic_l1_ssim_loss_forward_backward(1, CH, H, W, C1, C2, self.lambda_dssim, p(image), p(gt), p(d1), p(d2), p(d3), p(partials),
                                                         p(terms), p(dL), _lib.current_stream_ptr()))
        return dL, terms

    def _exposure_scratch(self, img):
        if self._eshape != tuple(img.shape) or self._ebuf[0].device != img.device:
            n = int(_lib.lib().gslic_exposure_partials_count(img.shape[1], img.shape[2]))
            self._ebuf = [torch.empty_like(img), torch.empty_like(img), torch.empty(n, device=img.device)]
            self._eshape = tuple(img.shape)
        return self._ebuf

    def exposure_apply(self, image, E):
        """image [3,H,W], E 12 device floats ([3,4], e.g. a row of trainer.Exposure.params): the exposure-compensated image, in a scratch image kept
        here (gslic_exposure_apply, one launch)."""
        image = image.contiguous()
        out = self._exposure_scratch(image)[0]
        exposure_apply(image, E, out)
        return out

    def exposure_backward(self, image, E, dL_dout, dL_dE, adam=None):
        """The other half: dL/dimage = E^T dL_dout into a scratch image kept here (returned), dL/dE into dL_dE [3,4]; adam: a _lib.ExposureAdam —
        the second launch then also updates the row it names (gslic_exposure_backward, two launches)."""
        image = image.contiguous()
        _out, dL_dimage, partials = self._exposure_scratch(image)
        exposure_backward(image, E, dL_dout, dL_dimage, partials, dL_dE, adam)
        return dL_dimage

    def value(self, terms, lambda_depth=0.0):
        """The loss from the terms: [mean L1, mean SSIM] or, with lambda_depth != 0, [mean L1, mean SSIM, L_d]."""
        v = (1.0 - self.lambda_dssim) * terms[0] + self.lambda_dssim * (1.0 - terms[1])
        if lambda_depth:
            v = v + float(lambda_depth) * terms[2]
        return v
