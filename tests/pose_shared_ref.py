"""The rules of gslic_pose_step_shared and gslic_pose_calibrate_rows (include/gslic_hip.h) restated in numpy float64 on top of tests/pose_ref.py:
the chain on the stepped row, g_tau = xi_i . g, Adam on the seven coordinates (rho_x, phi_x, tau), every row moved by d_x + d_tau xi_j through
pose_ref's retraction, Gram-Schmidt and recomposition, the accumulated correction X moved by d_x and tau by d_tau; and the calibration of a fresh
row, T <- exp((tau xi)^) (X T).  Same formulas, same branches, same order; only the precision differs.  No tests in this file.

A set is a dict: view [V,16], proj [V,16], campos [V,3], twist [V,6], sm [7], sv [7], ssteps (int), X [3,4] and tau (float)."""
import math

import numpy as np

import pose_ref as ref


def new_set(view, proj, campos, twist=None):
    view = np.array(view, np.float64).reshape(-1, 16)
    V = view.shape[0]
    return dict(view=view, proj=np.array(proj, np.float64).reshape(V, 16), campos=np.array(campos, np.float64).reshape(V, 3),
                twist=np.zeros((V, 6)) if twist is None else np.array(twist, np.float64).reshape(V, 6), sm=np.zeros(7), sv=np.zeros(7), ssteps=0,
                X=np.eye(3, 4), tau=0.0)


def copy_set(s):
    return {k: (np.array(a, np.float64) if isinstance(a, np.ndarray) else a) for k, a in s.items()}


def gradient(s, projection, grads, view):
    """(g [6], g_tau): pose_ref.chain on row `view`, then xi . g with k ascending."""
    g = ref.chain(s["view"][view], projection, *grads)
    xi = s["twist"][view]
    g_tau = 0.0
    for k in range(6):
        g_tau = g_tau + g[k] * xi[k] if k else g[0] * xi[0]
    return np.concatenate([g, [g_tau]])


def adam7(g7, sm, sv, ssteps, lr_trans, lr_rot, lr_time, betas=(0.9, 0.999), eps=1e-8):
    """pose_ref.adam's rule on seven coordinates: (delta [7], sm, sv, ssteps + 1); scalars taken as the float32 values the kernel is handed."""
    b1, b2, eps = float(np.float32(betas[0])), float(np.float32(betas[1])), float(np.float32(eps))
    lr = np.array([float(np.float32(lr_trans))] * 3 + [float(np.float32(lr_rot))] * 3 + [float(np.float32(lr_time))])
    n = int(ssteps) + 1
    g = np.asarray(g7, np.float64)
    m = b1 * np.asarray(sm, np.float64) + (1.0 - b1) * g
    v = b2 * np.asarray(sv, np.float64) + (1.0 - b2) * g * g
    s, q = lr / (1.0 - b1 ** n), math.sqrt(1.0 - b2 ** n)
    with np.errstate(divide="ignore", invalid="ignore"):
        return -(s * m) / (np.sqrt(v) / q + eps), m, v, n


def moves(d):
    d = np.asarray(d, np.float64)
    return bool(np.isfinite(d).all() and (d != 0).any())


def retract34(X, d):
    """The 3x4 [R | t] moved by d: pose_ref's exp and Gram-Schmidt, no recomposition."""
    E = ref.se3_exp(d)
    out = np.empty((3, 4))
    out[:, :3] = ref.orthonormalise(E[:3, :3] @ X[:, :3])
    out[:, 3] = E[:3, :3] @ X[:, 3] + E[:3, 3]
    return out


def step(s, projection, grads, view, lr_trans, lr_rot, lr_time, betas=(0.9, 0.999), eps=1e-8, skip=False):
    """One gslic_pose_step_shared: (new set, grad_out [7] or None when nothing at all is written).  The no-ops of the header leave what they leave."""
    new = copy_set(s)
    V = s["view"].shape[0]
    if not 0 <= int(view) < V:
        return new, None
    g7 = gradient(s, projection, grads, int(view))
    if skip or not np.isfinite(g7).all():
        return new, g7
    delta, new["sm"], new["sv"], new["ssteps"] = adam7(g7, s["sm"], s["sv"], s["ssteps"], lr_trans, lr_rot, lr_time, betas, eps)
    d_x, d_tau = delta[:6], delta[6]
    for j in range(V):
        with np.errstate(invalid="ignore"):
            d_j = d_x + d_tau * s["twist"][j]
        if moves(d_j):
            new["view"][j], new["proj"][j], new["campos"][j] = ref.recompose(ref.retract(s["view"][j], d_j), projection)
    if moves(d_x):
        new["X"] = retract34(s["X"], d_x)
    if np.isfinite(d_tau) and d_tau != 0:
        new["tau"] = s["tau"] + d_tau
    return new, g7


def calibrate_rows(s, projection, first, count):
    """gslic_pose_calibrate_rows: rows [first, first + count) <- exp((tau xi_j)^) (X T), through retraction, Gram-Schmidt and recomposition."""
    new = copy_set(s)
    X4 = np.eye(4)
    X4[:3, :] = s["X"]
    for j in range(first, first + count):
        d = s["tau"] * s["twist"][j]
        if not np.isfinite(d).all():
            continue
        A = X4 @ ref.mat(s["view"][j])
        new["view"][j], new["proj"][j], new["campos"][j] = ref.recompose(ref.retract(ref.flat(A), d), projection)
    return new
