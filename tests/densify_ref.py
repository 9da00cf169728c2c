"""Shared by tests/test_densify_{cpu,gpu}.py: restatements of the densification rules of include/gslic_hip.h that the device code is held
against (no test in this file) — the counter generator in numpy integers (u_n exact), float64 Box-Muller and split-child positions, the
selection rule in torch comparisons, and the float64 replay of contribution_ref.replay extended by the per-pixel error e(p)."""
import math

import numpy as np
import torch

M32 = 0xFFFFFFFF
SHRINK = np.float32(math.log(1.6))     # the float32 a split child's raw scaling is reduced by

# Relative margins of the float32 kernels against the float64 restatements.  Not fixed in advance: measured on one MI355X (the lines
# test_densify_gpu.py prints before it asserts; profiles/densify_config3.log) and set to 4x the larger of the measured gaps, the project's rule
# for contribution_ref.MARGIN.
#   err_sum against the float64 replay, gap relative to the tensor's max: scene (a) ERR_GAP_A, scene (b) ERR_GAP_B; against the backward's
#   dL_dcolor[:, 0] under dL_dpix = (e, 0, 0): ERR_BWD_GAP_A / _B
ERR_GAP_A, ERR_GAP_B, ERR_BWD_GAP_A, ERR_BWD_GAP_B = 3.249e-8, 9.161e-8, 1.611e-7, 4.974e-8
ERR_MARGIN = 6.5e-7
#   split children's xyz against child_xyz(), gap relative to the parent's largest activated scale, largest over the emission cases (the case with
#   quaternions scaled to 1e-18 was added after the bar was set and is held to the same bar: it measures 1.481e-6)
XYZ_GAP = 1.162e-6
XYZ_MARGIN = 4.7e-6


# ---------------------------------------------------------------------------------------------------- the counter generator
def fmix32(h):
    h = np.asarray(h, dtype=np.uint64) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(M32)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    return h


def key(seed, o):
    """fmix32(fmix32(seed) ^ o) for an array of original indices o."""
    return fmix32(fmix32(np.uint64(int(seed) & M32)) ^ (np.asarray(o, dtype=np.uint64) & np.uint64(M32)))


def word(seed, o, n):
    return fmix32((key(seed, o) + np.uint64(0x9E3779B9) * np.uint64(n + 1)) & np.uint64(M32))


def u24(seed, o, n):
    """The integer 2 (word >> 9) + 1 in [1, 2^24): u_n = u24 / 2^24 exactly (also in float32)."""
    return np.uint64(2) * (word(seed, o, n) >> np.uint64(9)) + np.uint64(1)


def uniform(seed, o, n):
    return u24(seed, o, n).astype(np.float64) / float(1 << 24)


def normal3(seed, o, child):
    """z_c [len(o), 3] in float64."""
    u = [uniform(seed, o, 4 * child + i) for i in range(4)]
    r0, r2 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    return np.stack([r0 * np.cos(2.0 * np.pi * u[1]), r0 * np.sin(2.0 * np.pi * u[1]), r2 * np.cos(2.0 * np.pi * u[3])], axis=1)


def rotation_matrix(q):
    """R(q / |q|) [n,3,3] in float64 for q = (r, x, y, z) [n,4]."""
    q = np.asarray(q, np.float64)
    q = q / np.sqrt((q * q).sum(1, keepdims=True))
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - r * z); R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y); R[:, 2, 1] = 2 * (y * z + r * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def child_xyz(xyz, scaling_raw, rotation_raw, o, seed, child):
    """xyz + R(q/|q|) (exp(scaling_raw) (.) z_child) in float64 on the parents' float32 values; o: the parents' original indices."""
    s = np.exp(np.asarray(scaling_raw, np.float64))
    v = s * normal3(seed, o, child)
    return np.asarray(xyz, np.float64) + np.einsum("nij,nj->ni", rotation_matrix(rotation_raw), v)


# ---------------------------------------------------------------------------------------------------- the selection rule
def select(xyz, dc, opacity, scaling, rotation, grow, protect, tie, thr):
    """The rule in torch comparisons on tensors of one device.  Returns (parent_index LongTensor [count], count, count_split, split mask [P])."""
    P = xyz.shape[0]
    fin = lambda t: torch.isfinite(t.reshape(P, -1)).all(1)
    rot = rotation.reshape(P, 4)
    q = rot.float()
    norm2 = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]      # float32, each op rounded on its own, the header's order
    eligible = grow.bool() & fin(xyz) & fin(dc) & fin(opacity) & fin(scaling) & fin(rot) & (norm2 > 0)
    if protect is not None:
        eligible &= ~protect.bool()
    split = eligible & (scaling.reshape(P, 3) > thr).any(1)
    o = torch.arange(P, device=xyz.device) if tie is None else tie.long()
    rows = eligible.nonzero().squeeze(1)
    parent_index = rows[torch.argsort(o[rows])]
    return parent_index, int(eligible.sum()), int(split.sum()), split


# ---------------------------------------------------------------------------------------------------- the error-weighted replay
def error_value(err):
    """e(p): err clamped to [0, 4], NaN and negative values read as 0, +inf as 4 (float64 of the float32 input)."""
    e = np.asarray(err, np.float64)
    return np.clip(np.where(np.isnan(e), 0.0, e), 0.0, 4.0)


def replay_error(means2D, conic_opacity, point_list, ranges, n_contrib, W, H, P, err):
    """contribution_ref.replay's walk with the pairs weighted by e(p): float64 err_sum [P] = sum of w e(p)."""
    m2d = np.asarray(means2D, np.float64).reshape(P, 2)
    co = np.asarray(conic_opacity, np.float64).reshape(P, 4)
    pl = np.asarray(point_list).astype(np.int64).reshape(-1)
    rg = np.asarray(ranges).astype(np.int64).reshape(-1, 2)
    nc_img = np.asarray(n_contrib).astype(np.int64).reshape(H, W)
    e_img = error_value(err).reshape(H, W)
    gx = (W + 15) // 16
    out = np.zeros(P)
    for t in range(rg.shape[0]):
        x0, y0 = (t % gx) * 16, (t // gx) * 16
        ys, xs = np.mgrid[y0:min(y0 + 16, H), x0:min(x0 + 16, W)]
        if ys.size == 0:
            continue
        nc = nc_img[ys, xs]
        T = np.ones(nc.shape)
        lo, hi = rg[t]
        for k in range(int(min(hi - lo, nc.max()))):
            g = pl[lo + k]
            dx, dy = m2d[g, 0] - xs, m2d[g, 1] - ys
            power = -0.5 * (co[g, 0] * dx * dx + co[g, 2] * dy * dy) - co[g, 1] * dx * dy
            alpha = np.minimum(0.99, co[g, 3] * np.exp(np.minimum(power, 0.0)))
            hit = (k < nc) & ~(power > 0.0) & ~(alpha < 1.0 / 255.0)
            if not hit.any():
                continue
            w = np.where(hit, alpha * T, 0.0)
            T = np.where(hit, T * (1.0 - alpha), T)
            out[g] += (w * e_img[ys, xs]).sum()
    return out


def max_gap(got, ref):
    """Largest absolute gap relative to the reference tensor's largest magnitude."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))
