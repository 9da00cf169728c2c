"""The rule of gslic_pose_step (include/gslic_hip.h) restated in numpy float64: the se(3) chain of the three camera gradients, torch.optim.Adam
with bias correction on the six tangent coordinates (a rate for the translation, one for the rotation), the retraction T_cw <- exp(delta^) T_cw,
Gram-Schmidt on the rows of R and the recomposition of view / proj / campos.  Same formulas, same branches, same order; only the precision
differs (the kernel's float32 steps are float64 here; the bias terms and the three exp coefficients are double in both).  No tests in this file."""
import math

import numpy as np

SERIES_THETA = 1e-4   # GSLIC_POSE_SERIES_THETA


def mat(a16):
    """float[16] with element (r, c) at [4 c + r] -> the 4x4 math matrix, float64."""
    return np.asarray(a16, np.float64).reshape(4, 4).T


def flat(M):
    return np.ascontiguousarray(np.asarray(M, np.float64).T).reshape(16)


def chain(view, projection, dview, dproj, dcampos):
    """g [6] = dL/d(rho, phi) of the left increment, from the row's view [16], the projection [16] and the three camera gradients."""
    V, Pm, Gv, Gp = mat(view), mat(projection), mat(dview), mat(dproj)
    gc = np.asarray(dcampos, np.float64).reshape(3)
    R, t = V[:3, :3], V[:3, 3]
    G = (Gv + Pm.T @ Gp)[:3, :]
    GR = G[:, :3] - np.outer(t, gc)
    Gt = G[:, 3] - R @ gc
    M = GR @ R.T
    dphi = np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]]) + np.cross(t, Gt)
    return np.concatenate([Gt, dphi])


def adam(g, m, v, step, lr_trans, lr_rot, betas=(0.9, 0.999), eps=1e-8):
    """One step of torch.optim.Adam's rule on the six coordinates: (delta [6], m, v, step + 1).  betas / eps / rates are taken as the float32 values
    the kernel is handed."""
    b1, b2, eps = float(np.float32(betas[0])), float(np.float32(betas[1])), float(np.float32(eps))
    lr = np.array([float(np.float32(lr_trans))] * 3 + [float(np.float32(lr_rot))] * 3)
    n = int(step) + 1
    g = np.asarray(g, np.float64)
    m = b1 * np.asarray(m, np.float64) + (1.0 - b1) * g
    v = b2 * np.asarray(v, np.float64) + (1.0 - b2) * g * g
    s, q = lr / (1.0 - b1 ** n), math.sqrt(1.0 - b2 ** n)
    return -(s * m) / (np.sqrt(v) / q + eps), m, v, n


def series_coefficients(theta):
    """(a, b, c) by the series the rule uses below SERIES_THETA: the first two terms of sin(t) / t, (1 - cos t) / t^2, (t - sin t) / t^3."""
    th2 = theta * theta
    return 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0


def closed_coefficients(theta):
    th2 = theta * theta
    return math.sin(theta) / theta, (1.0 - math.cos(theta)) / th2, (theta - math.sin(theta)) / (th2 * theta)


def exp_coefficients(theta):
    return series_coefficients(theta) if theta < SERIES_THETA else closed_coefficients(theta)


def se3_exp(xi):
    """exp of (rho, phi) as a 4x4 matrix by the kernel's formulas (K2 written out, the series below SERIES_THETA)."""
    xi = np.asarray(xi, np.float64)
    rho, (x, y, z) = xi[:3], xi[3:]
    a, b, c = exp_coefficients(math.sqrt((x * x + y * y) + z * z))
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    K2 = np.array([[-(y * y + z * z), x * y, x * z], [x * y, -(x * x + z * z), y * z], [x * z, y * z, -(x * x + y * y)]])
    E = np.eye(4)
    E[:3, :3] = np.eye(3) + a * K + b * K2
    E[:3, 3] = (np.eye(3) + b * K + c * K2) @ rho
    return E


def orthonormalise(R):
    """Gram-Schmidt on the rows in the order 0, 1; row 2 is their cross product."""
    r0 = R[0] / math.sqrt(R[0] @ R[0])
    u = R[1] - (r0 @ R[1]) * r0
    r1 = u / math.sqrt(u @ u)
    return np.stack([r0, r1, np.cross(r0, r1)])


def retract(view, delta):
    """The new 4x4 V = [R | t; 0 0 0 1] of a row moved by delta."""
    V = mat(view)
    E = se3_exp(delta)
    out = np.eye(4)
    out[:3, :3] = orthonormalise(E[:3, :3] @ V[:3, :3])
    out[:3, 3] = E[:3, :3] @ V[:3, 3] + E[:3, 3]
    return out


def recompose(V, projection):
    """(view [16], proj [16], campos [3]) of a 4x4 V."""
    return flat(V), flat(mat(projection) @ V), -(V[:3, :3].T @ V[:3, 3])


def step(row, projection, grads, lr_trans, lr_rot, betas=(0.9, 0.999), eps=1e-8, skip=False):
    """One gslic_pose_step on a row = dict(view, proj, campos, m, v, steps) (float64 arrays; float32 inputs are taken as they are): returns
    (new row, g).  The three no-ops of the header leave what they leave."""
    g = chain(row["view"], projection, *grads)
    new = {k: np.array(a, np.float64) if k != "steps" else int(a) for k, a in row.items()}
    if skip or not np.isfinite(g).all():
        return new, g
    delta, new["m"], new["v"], new["steps"] = adam(g, row["m"], row["v"], row["steps"], lr_trans, lr_rot, betas, eps)
    if np.isfinite(delta).all() and (delta != 0).any():
        new["view"], new["proj"], new["campos"] = recompose(retract(row["view"], delta), projection)
    return new, g
