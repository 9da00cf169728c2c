"""float64 torch reference of the weighted L1 + SSIM loss (FusedLoss.forward_backward(weight=...), gslic_l1_ssim_loss_weighted_forward_backward):
conv2d SSIM with the window of loss._gaussian_window, the definition of include/gslic_hip.h, autograd for the gradient.  CPU only.

    w [H,W] shared by the channels, clamped as the kernels clamp it (NaN, negative -> 0; above 1, +inf -> 1),  S = sum_p w_p
    L1_w = sum_p w_p sum_c |img - gt| / (3 S),   SSIM_w = sum_p w_p sum_c ssim_c(p) / (3 S),   loss = (1-lambda) L1_w + lambda (1 - SSIM_w)
    S == 0: both terms 0 and a zero gradient.  The SSIM statistics (the five 11-tap means) run over ALL pixels: only the map is weighted."""
import numpy as np
import torch

C1 = 0.01 ** 2
C2 = 0.03 ** 2

# ---- margins of the float32 kernels against this reference (check 4 of tests/test_weighted_loss_gpu.py).  Not fixed in advance: measured on one
# MI355X with the EXISTING unweighted kernels on the same images at w == 1 (the "[weighted loss gap]" lines the test prints before it asserts;
# profiles/weighted_loss_config3.log), and set to 4x the larger measured gap — the rule of contribution_ref.MARGIN.
#   terms: a weighted mean is a convex combination of the per-pixel values, so its distance to the reference is bounded by the largest per-pixel
#   distance of the existing kernels' values: max over the six shapes of max_p |fusedssim map - float64 map| (measured MAP_GAP) and of
#   max_p | |img-gt|_f32 - |img-gt|_f64 | (measured ABS_GAP), beside the distance of the unweighted terms themselves (measured TERM_GAP).
#   gradient: max |dL/dimg - reference| / max |reference| of gslic_l1_ssim_loss_forward_backward (measured GRAD_GAP); where the reference
#   gradient is exactly zero (the 1 x 1 image) relative to (1 - lambda) / (3 S), one pixel's L1 gradient.
MAP_GAP = 2.254e-6      # (33 x 65; the others 1.2e-6 .. 2.1e-6)
ABS_GAP = 1.490e-8
TERM_GAP = 9.954e-8
GRAD_GAP = 5.857e-7     # (70 x 45; the others 4.3e-7 .. 5.2e-7, the 1 x 1 image 5.6e-8)
TERMS_MARGIN = 9.1e-6   # 4 * max(MAP_GAP, ABS_GAP, TERM_GAP), absolute (the terms lie in [0, 1]).  Weighted kernels, worst case measured: 2.4e-7
GRAD_MARGIN = 2.35e-6   # 4 * GRAD_GAP, relative (test_weighted_loss_gpu._grad_gap).  Weighted kernels, worst case measured: 5.8e-7


def clamp_weight(w):
    """The weight image as the kernels read it."""
    w = torch.as_tensor(w)
    return torch.where(w > 0, w.clamp(max=1.0), torch.zeros_like(w))


def window64(channel):
    from gaussian_lic_amd.loss import _gaussian_window
    return _gaussian_window(11, 1.5, channel, torch.zeros(1, dtype=torch.float64))


def ssim_map64(img, gt):
    """[C,H,W] float64 SSIM map (zero padding, 11x11 Gaussian window)."""
    img, gt = img.double().unsqueeze(0), gt.double().unsqueeze(0)
    ch = img.size(1)
    win = window64(ch)
    conv = lambda x: torch.nn.functional.conv2d(x, win, padding=5, groups=ch)
    mu1, mu2 = conv(img), conv(gt)
    s11 = conv(img * img) - mu1 * mu1
    s22 = conv(gt * gt) - mu2 * mu2
    s12 = conv(img * gt) - mu1 * mu2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))
    return m[0]


def weighted_terms(img, gt, weight):
    """(L1_w, SSIM_w, S) as float64 tensors (differentiable in img)."""
    w = clamp_weight(weight.double() if torch.is_tensor(weight) else torch.as_tensor(weight, dtype=torch.float64))
    S = w.sum()
    if float(S) == 0.0:
        z = (img.double() * 0.0).sum()
        return z, z, S
    n = img.size(0) * S
    l1 = (w * (img.double() - gt.double()).abs()).sum() / n
    ss = (w * ssim_map64(img, gt)).sum() / n
    return l1, ss, S


def weighted_loss(img, gt, weight, lambda_dssim=0.2):
    l1, ss, S = weighted_terms(img, gt, weight)
    if float(S) == 0.0:
        return l1          # nothing to train on: the terms are 0, 0 and the gradient is zero
    return (1.0 - lambda_dssim) * l1 + lambda_dssim * (1.0 - ss)


def unweighted_loss(img, gt, lambda_dssim=0.2):
    """The formula every path applies without a weight: 0.8 mean|d| + 0.2 (1 - mean ssim), in float64."""
    return (1.0 - lambda_dssim) * (img.double() - gt.double()).abs().mean() + lambda_dssim * (1.0 - ssim_map64(img, gt).mean())


def weighted_reference(img, gt, weight, lambda_dssim=0.2):
    """(terms float64 numpy [L1_w, SSIM_w, S], dL/dimg float64 tensor [C,H,W]) by autograd."""
    x = img.detach().double().clone().requires_grad_(True)
    l1, ss, S = weighted_terms(x, gt.detach(), weight)
    if float(S) == 0.0:
        return np.zeros(3), torch.zeros_like(x)
    ((1.0 - lambda_dssim) * l1 + lambda_dssim * (1.0 - ss)).backward()
    return np.array([float(l1.detach()), float(ss.detach()), float(S)]), x.grad.detach()


def images(H, W, seed):
    """A rendered / target pair in [0,1] with a patch where they are equal (sign(0) = 0), float32 [3,H,W]."""
    rng = np.random.default_rng(seed)
    a = rng.random((3, H, W)).astype(np.float32)
    b = np.clip(a + 0.1 * rng.standard_normal((3, H, W)), 0.0, 1.0).astype(np.float32)
    a[:, :min(4, H), :min(6, W)] = b[:, :min(4, H), :min(6, W)]
    return torch.from_numpy(a), torch.from_numpy(b)


PATTERNS = ("ones", "zeros", "single", "mask", "tiles", "frame", "uniform", "dirty")


def weight_pattern(name, H, W, seed=0):
    """The weight images of the tests, float32 [H,W]."""
    g = torch.Generator().manual_seed(1000 + seed)
    if name == "ones":
        return torch.ones(H, W)
    if name == "zeros":
        return torch.zeros(H, W)
    if name == "single":
        w = torch.zeros(H, W)
        w[(2 * H) // 3, W // 3] = 1.0
        return w
    if name == "mask":
        return (torch.rand(H, W, generator=g) < 0.5).float()
    if name == "tiles":   # whole 32x32 tiles alternately 0 and 1
        ty, tx = torch.arange(H).div(32, rounding_mode="floor"), torch.arange(W).div(32, rounding_mode="floor")
        return ((ty[:, None] + tx[None, :] + 1) % 2).float()    # (the first tile is kept)
    if name == "frame":   # a zero frame one tenth wide (the undistortion border)
        w = torch.zeros(H, W)
        by, bx = max(1, H // 10), max(1, W // 10)
        w[by:H - by, bx:W - bx] = 1.0
        return w
    if name == "uniform":
        return torch.rand(H, W, generator=g)
    if name == "dirty":   # uniform with NaN, -1, 2 and +inf sprinkled in
        w = torch.rand(H, W, generator=g)
        r = torch.rand(H, W, generator=g)
        w[r < 0.05] = float("nan")
        w[(r >= 0.05) & (r < 0.10)] = -1.0
        w[(r >= 0.10) & (r < 0.15)] = 2.0
        w[(r >= 0.15) & (r < 0.20)] = float("inf")
        return w
    raise KeyError(name)
