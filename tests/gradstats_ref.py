"""Shared by tests/test_gradstats_{cpu,gpu}.py (no test in this file): the rule of the gradient densification statistics (include/gslic_hip.h,
gslic_grad_stats) transcribed into numpy float32, the two mask rules, and the scenes of the GPU tests.

The transcription never sees the code under test's output: it is fed the dL_dmean2D of the ten-gradient backward and the forward's radii."""
import numpy as np
import torch

SENT_SUM = np.float32(3.25)          # pre-fill of grad_sum: finite, so an addition that should not happen shows
SENT_SEEN = np.uint32(0x5A5A5A5A)    # pre-fill of n_seen
SENT_RADIUS = np.int32(7)            # pre-fill of max_radius: between the radii of the scenes, so both arms of the max are taken
GUARD = 0x7E57C0DE                   # the words around the three arrays


def sentinels(P):
    return np.full(P, SENT_SUM, np.float32), np.full(P, SENT_SEEN, np.uint32), np.full(P, SENT_RADIUS, np.int32)


def apply_rule(grad_sum, n_seen, max_radius, dL_dmean2D, radii, rows=None):
    """One backward's update, in place, on float32 / uint32 / int32 arrays [P]; dL_dmean2D float32 [P,3] (elements 0 and 1 are mx, my), radii int32 [P];
    rows = (begin, end) or None for all.  Every operation is one float32 operation, rounded on its own."""
    assert grad_sum.dtype == np.float32 and n_seen.dtype == np.uint32 and max_radius.dtype == np.int32
    g = np.ascontiguousarray(dL_dmean2D, dtype=np.float32)
    r = np.asarray(radii, dtype=np.int32)
    mx, my = g[:, 0], g[:, 1]
    with np.errstate(all="ignore"):
        xx = (mx * mx).astype(np.float32)
        yy = (my * my).astype(np.float32)
        n = np.sqrt((xx + yy).astype(np.float32)).astype(np.float32)
    vis = r > 0
    if rows is not None:
        inside = np.zeros_like(vis)
        inside[rows[0]:rows[1]] = True
        vis &= inside
    upd = vis & np.isfinite(n)
    with np.errstate(all="ignore"):
        grad_sum[upd] = (grad_sum[upd] + n[upd]).astype(np.float32)
    n_seen[upd] = n_seen[upd] + np.uint32(1)
    max_radius[vis] = np.maximum(max_radius[vis], r[vis])
    return n


def grow_mask(grad_sum, n_seen, grad_above, min_seen=1):
    """n_seen >= max(min_seen, 1) and grad_sum >= float32(grad_above) * float32(n_seen): comparisons and one float32 product."""
    n = np.asarray(n_seen).astype(np.uint32)
    with np.errstate(all="ignore"):
        lim = (np.float32(grad_above) * n.astype(np.float32)).astype(np.float32)
        return ((n >= max(int(min_seen), 1)) & (np.asarray(grad_sum, np.float32) >= lim)).astype(np.uint8)


def big_mask(max_radius, max_screen_radius):
    return (np.asarray(max_radius, np.int32) > int(max_screen_radius)).astype(np.uint8)


W, H = 128, 96
# the view sequence of the rule tests: the identity pose, a yawed one, and one looking the other way (nearly every row invisible)
VIEWS = (None, dict(ypr=(9.0, -4.0, 2.0), t=(0.2, -0.1, 0.1)), dict(ypr=(180.0, 0.0, 0.0), t=(0.0, 0.0, 0.0)))


def scene(P, degree, seed=11):
    """Raw parameters (CPU) of a random scene of P rows for the W x H camera.  SH degree 3 keeps the 15 rest coefficients (the one-wave kernel with
    the SH rows in LDS), SH degree 1 keeps 3 (the generic 256-thread kernel).  P == 1: the one row sits in front of the identity camera (visible
    there, behind the camera of the third view); P > 1: row 0 is far off to the side of every view (never visible)."""
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd.synthetic import random_scene
    raw = random_scene(P, W, H, sh_degree=degree, seed=seed + P)
    if degree == 1:
        raw["features_rest"] = raw["features_rest"][:, :3].contiguous()
    if P == 1:
        raw["xyz"][0] = torch.tensor([0.1, -0.05, 5.0])
        raw["scaling"][0] = torch.log(torch.tensor([0.15, 0.1, 0.12]))
        raw["opacity"][0] = 1.0
    else:
        raw["xyz"][0] = torch.tensor([0.0, 60.0, 1.0])
        raw["scaling"][0] = torch.log(torch.tensor([0.01, 0.01, 0.01]))
    return raw
