"""Brute-force statement of csrc/knn.hip's result — the mean of the squared distances to the three nearest OTHER points — in numpy, and the
directed point clouds of tests/test_knn_edges_gpu.py.  Two precisions of the same float32 points:
  mean_dist2_f32: the kernel's own formula, dx*dx + dy*dy + dz*dz on float32 differences with every operation rounded to float32, the three
                  smallest taken in float32, summed ascending and divided by 3 in float32;
  mean_dist2_f64: everything in float64.
Self is excluded by INDEX, not by value: a duplicate of the query point is a neighbour at distance 0."""
import numpy as np

SIZES = (4, 5, 1023, 1024, 1025, 2047, 2049, 3073)
CLOUDS = ("gaussian", "shifted-positive", "shifted-negative", "plane-z0", "plane-z5", "line-x", "twice", "four-times", "two-clusters", "lattice")


def _mean_dist2(pts, dtype, chunk=512):
    p = np.ascontiguousarray(pts, np.float32).astype(dtype)
    P = p.shape[0]
    assert P >= 4
    out = np.empty(P, dtype)
    three = dtype(3.0)
    for a in range(0, P, chunk):
        q = p[a:a + chunk]
        d = p[None, :, :] - q[:, None, :]                 # [chunk, P, 3], rounded to dtype
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        d2[np.arange(q.shape[0]), a + np.arange(q.shape[0])] = np.inf
        best = np.sort(np.partition(d2, 2, axis=1)[:, :3], axis=1)
        out[a:a + chunk] = ((best[:, 0] + best[:, 1]) + best[:, 2]) / three
    return out


def mean_dist2_f32(pts):
    return _mean_dist2(pts, np.float32)


def mean_dist2_f64(pts):
    return _mean_dist2(pts, np.float64)


def cloud(kind, P, seed=0):
    """float32 [P, 3].  The kinds, and what of knn.hip they reach:
    gaussian          origin-centred, anisotropic (the cloud of test_knn_parity, its outliers beyond 2.8 sigma halved)
    shifted-positive  the same + (100, 50, 20): the bounding box starts at the zero it was initialised with, the Morton codes are squeezed
    shifted-negative  the same - (100, 50, 20)
    plane-z0          z == 0: max - min == 0 on that axis, 0 / 0 = NaN, code 0
    plane-z5          z == 5: every point has the axis' largest code
    line-x            y == z == 0
    twice             every point present twice (P odd: one of them three times)
    four-times        every point present four times at the least: the three nearest are copies, the result is exactly 0 (reject == 0)
    two-clusters      two Gaussian blobs 1e3 apart, 3 P / 8 + 1 and the rest: neither a multiple of the 1024-point box
    lattice           the first P points of an integer lattice of unit spacing, shuffled: exactly tied distances everywhere"""
    assert kind in CLOUDS
    base = np.random.default_rng([seed, P]).standard_normal((P, 3))                                # (the same points for every kind)
    base = np.where(np.abs(base) > 2.8, base / 2, base) * np.array([10.0, 3.0, 7.0])               # within 2.8 sigma: a shifted cloud stays on its side
    g = lambda n: base[:n].copy()
    rng = np.random.default_rng([seed, P, 1])
    shift = np.array([100.0, 50.0, 20.0])
    if kind == "gaussian":
        pts = g(P)
    elif kind == "shifted-positive":
        pts = g(P).astype(np.float32) + shift
    elif kind == "shifted-negative":
        pts = g(P).astype(np.float32) - shift
    elif kind in ("plane-z0", "plane-z5"):
        pts = g(P)
        pts[:, 2] = 0.0 if kind == "plane-z0" else 5.0
    elif kind == "line-x":
        pts = g(P)
        pts[:, 1:] = 0.0
    elif kind in ("twice", "four-times"):
        m = 2 if kind == "twice" else 4
        pts = g(max(P // m, 1))[np.arange(P) % max(P // m, 1)]
        pts = pts[rng.permutation(P)]
    elif kind == "two-clusters":
        n0 = 3 * P // 8 + 1
        pts = g(P)
        pts[n0:] += np.array([1e3, 0.0, 0.0])
    elif kind == "lattice":
        k = int(np.ceil(P ** (1.0 / 3.0) - 1e-9))
        while k ** 3 < P:
            k += 1
        i = np.arange(P)
        pts = np.stack([i % k, (i // k) % k, i // (k * k)], 1).astype(np.float64) - k // 2
        pts = pts[rng.permutation(P)]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(pts, np.float32)
