"""The rules of gslic_exposure_apply / gslic_exposure_backward (include/gslic_hip.h) restated in numpy: the float32 rule with every product and sum
one operation rounded on its own, in the header's order; the same in float64; and torch.optim.Adam's bias-corrected rule in float64 and as the
kernel words it in float32.  No tests here: tests/test_exposure_cpu.py and tests/test_exposure_gpu.py use it."""
import numpy as np

F = np.float32


def apply32(E, image):
    """out_c = ((E[c,0] r + E[c,1] g) + E[c,2] b) + E[c,3] on a planar [3,H,W] float32 image (numpy rounds every float32 operation on its own)."""
    E, x = np.asarray(E, F).reshape(3, 4), np.asarray(image, F)
    return np.stack([((E[c, 0] * x[0] + E[c, 1] * x[1]) + E[c, 2] * x[2]) + E[c, 3] for c in range(3)]).astype(F)


def dimage32(E, g):
    """dL_dimage_k = ((E[0,k] g_0 + E[1,k] g_1) + E[2,k] g_2)."""
    E, g = np.asarray(E, F).reshape(3, 4), np.asarray(g, F)
    return np.stack([(E[0, k] * g[0] + E[1, k] * g[1]) + E[2, k] * g[2] for k in range(3)]).astype(F)


def apply64(E, image):
    E, x = np.asarray(E, np.float64).reshape(3, 4), np.asarray(image, np.float64)
    return np.einsum("ck,khw->chw", E[:, :3], x) + E[:, 3][:, None, None]


def backward64(E, image, g):
    """(dL_dimage [3,H,W], dL_dE [3,4], the bound's sum_p |g_c x_k| [3,4]) in float64; x is the model's INPUT image."""
    E, x, g = np.asarray(E, np.float64).reshape(3, 4), np.asarray(image, np.float64), np.asarray(g, np.float64)
    x1 = np.concatenate([x, np.ones_like(x[:1])])                      # [4,H,W]: the pixel and the constant 1
    dE = np.einsum("chw,khw->ck", g, x1)
    mag = np.einsum("chw,khw->ck", np.abs(g), np.abs(x1))
    return np.einsum("ck,chw->khw", E[:, :3], g), dE, mag


def adam64(p, m, v, t, g, lr, beta1, beta2, eps):
    """One torch.optim.Adam step (bias-corrected) in float64 on arrays: returns (p, m, v, t) after it.  t: the step count BEFORE the step."""
    p, m, v, g = (np.asarray(a, np.float64) for a in (p, m, v, g))
    lr, beta1, beta2, eps = float(lr), float(beta1), float(beta2), float(eps)
    t = int(t) + 1
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    p = p - (lr / (1.0 - beta1 ** t)) * m / (np.sqrt(v) / np.sqrt(1.0 - beta2 ** t) + eps)
    return p, m, v, t


def adam32(p, m, v, t, g, lr, beta1, beta2, eps):
    """The same step as the kernel words it: the two bias terms in double from the integer t, each rounded to float32 once, every other step one
    float32 operation."""
    p, m, v, g = (np.asarray(a, F) for a in (p, m, v, g))
    lr, beta1, beta2, eps = F(lr), F(beta1), F(beta2), F(eps)
    t = int(t) + 1
    step = F(float(lr) / (1.0 - float(beta1) ** t))
    q = F(np.sqrt(1.0 - float(beta2) ** t))
    m = beta1 * m + (F(1.0) - beta1) * g
    v = beta2 * v + ((F(1.0) - beta2) * g) * g
    p = p - (step * m) / (np.sqrt(v) / q + eps)
    return p.astype(F), m.astype(F), v.astype(F), t


def case(H, W, seed):
    """(E [3,4] with entries in [-1.5, 1.5], image [3,H,W] in [0,1] with some exact zeros, g [3,H,W] of mixed sign) as float32 arrays."""
    rng = np.random.default_rng(seed)
    E = rng.uniform(-1.5, 1.5, (3, 4)).astype(F)
    x = rng.uniform(0.0, 1.0, (3, H, W)).astype(F)
    x[rng.uniform(size=x.shape) < 0.1] = 0.0
    g = (rng.standard_normal((3, H, W)) * 1e-3).astype(F)
    return E, x, g


IDENTITY = np.eye(3, 4, dtype=F)
