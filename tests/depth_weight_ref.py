"""The rule of gslic_depth_loss_weighted_forward_backward (include/gslic_hip.h) restated in numpy: every step one float32 operation rounded on
its own, in the header's order.  The gradient takes S — the float32 sum of the weights, whose bits depend on the kernel's summation order — as an
input, so it can be held against the kernel bit for bit; the sums themselves are given in float64.  No GPU, no library."""
import numpy as np

F = np.float32


def read_weight(weight, shape):
    """w_p: None weighs every pixel 1; NaN, negative and +inf weights read as 0; no clamp at 1."""
    if weight is None:
        return np.ones(shape, F)
    w = np.asarray(weight, F)
    with np.errstate(invalid="ignore"):
        return np.where((w > 0) & (w < np.inf), w, F(0)).astype(F)


def pieces(depth, gt, weight, delta):
    """(m, w, r, rho, rho') per pixel, float32: the mask, the weight as read, the residual, the penalty and its derivative."""
    depth, gt, delta = np.asarray(depth, F), np.asarray(gt, F), F(delta)
    w = read_weight(weight, depth.shape)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        m = (gt > 0) & (w > 0)
        r = (depth - gt).astype(F)
        a = np.abs(r)
        sign = np.where(r > 0, F(1), np.where(r < 0, F(-1), F(0))).astype(F)
        if delta == 0:
            rho, drho = a, sign
        else:
            inside = a < delta
            rho = np.where(inside, ((F(0.5) * a).astype(F) * a).astype(F) / delta, a - (F(0.5) * delta)).astype(F)
            drho = np.where(inside, (r / delta).astype(F), sign).astype(F)
    return m, w, r, rho, drho


def gradient(depth, gt, weight, delta, lambda_depth, S):
    """dL_ddepth [H,W] float32 for the float32 weight sum S the kernel formed (terms[1])."""
    m, w, r, rho, drho = pieces(depth, gt, weight, delta)
    S, lam = F(S), F(lambda_depth)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        k = lam / S if S > 0 else F(0)
        kw = (F(k) * w).astype(F) if weight is not None else np.full(w.shape, k, F)
        if F(delta) == 0:
            g = np.where(r > 0, kw, np.where(r < 0, -kw, F(0)))
        else:
            g = (kw * drho).astype(F)
        return np.where(m, g, F(0)).astype(F)


def sums64(depth, gt, weight, delta):
    """(S, T, number of masked pixels): the two sums over the mask in float64, of the float32 summands w_p and w_p * rho_p."""
    m, w, r, rho, drho = pieces(depth, gt, weight, delta)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        wr = (w * rho).astype(F) if weight is not None else rho
    return float(w[m].astype(np.float64).sum()), float(wr[m].astype(np.float64).sum()), int(m.sum())


def loss64(depth, gt, weight, delta):
    """L_d = T / S in float64 (0 when S == 0)."""
    S, T, _n = sums64(depth, gt, weight, delta)
    return T / S if S > 0 else 0.0
