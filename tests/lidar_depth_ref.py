"""Reference of gslic_lidar_zbuffer_add / gslic_lidar_zbuffer_resolve (include/gslic_hip.h): a plain numpy float32 transcription of the rule, with
loops, and the clouds the LiDAR depth tests share.  Every np.float32 scalar operation below is ONE IEEE float32 operation rounded on its own, in
the header's order; nothing here calls the library.  test_lidar_depth_cpu.py pins it against Camera.project_depth on CPU tensors."""
import functools

import numpy as np

F = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)

SIZES = [(37, 23), (64, 64), (5, 3)]
COUNTS = [0, 1, 63, 64, 65, 257, 4097]
VIEWS = [None, "se3_c", "se3_d"]            # the identity camera and two general poses of synthetic_camera
FOOTPRINTS = [1, 3, 8]
MARGINS = [(0.0, 0.0), (0.1, 0.02), (100.0, 0.0)]   # the last is larger than every return of the clouds: bounds <= 0


def camera(W, H, view=None):
    from gaussian_lic_amd.camera import synthetic_camera
    return synthetic_camera(W, H, view)


def pose_f32(cam):
    """(R_cw [9] row-major, t_cw [3]) as Camera.project_depth forms them."""
    return (np.ascontiguousarray(cam.R_wc.T.astype(np.float32)).reshape(9), (-cam.R_wc.T @ cam.t_wc).astype(np.float32))


def _project(p, R, t, fx, fy, cx, cy):
    """(xf, yf, z) of one point by the header's rule (all np.float32 scalars)."""
    with np.errstate(all="ignore"):
        c = [F(F(F(F(p[0] * R[3 * k]) + F(p[1] * R[3 * k + 1])) + F(p[2] * R[3 * k + 2])) + t[k]) for k in range(3)]
        z = c[2]
        xf = np.floor(F(F(F(c[0] * fx) / z) + cx))
        yf = np.floor(F(F(F(c[1] * fy) / z) + cy))
    return xf, yf, z


def zbuffer_add(zbuf, points, R, t, fx, fy, cx, cy, W, H, index_base=0):
    """One thread per point, in a loop: zbuf [H*W] uint64 is updated in place."""
    points, R, t = np.asarray(points, F), np.asarray(R, F), np.asarray(t, F)
    fx, fy, cx, cy = F(fx), F(fy), F(cx), F(cy)
    with np.errstate(all="ignore"):
        for i in range(points.shape[0]):
            xf, yf, z = _project(points[i], R, t, fx, fy, cx, cy)
            if not (z > 0 and z < np.inf):
                continue
            if not (xf >= 0 and xf < F(W) and yf >= 0 and yf < F(H)):
                continue
            pix = int(yf) * W + int(xf)
            key = (np.uint64(z.view(np.uint32)) << np.uint64(32)) | np.uint64(index_base + i)
            if key < zbuf[pix]:
                zbuf[pix] = key
    return zbuf


def resolve(zbuf, W, H, footprint=0, margin_abs=0.0, margin_rel=0.0):
    """dict(depth float32 [H,W], index int32 [H,W], near float32 [H,W], n_measured int): per pixel the minimum key of the clipped window."""
    z2 = np.asarray(zbuf, np.uint64).reshape(H, W)
    r = int(footprint)
    ma, mr = F(margin_abs), F(margin_rel)
    depth, index, near = np.zeros((H, W), F), np.full((H, W), -1, np.int32), np.zeros((H, W), F)
    n = 0
    for y in range(H):
        for x in range(W):
            key = z2[max(0, y - r):min(H, y + r + 1), max(0, x - r):min(W, x + r + 1)].min()
            if key == EMPTY:
                continue
            d = np.uint32(key >> np.uint64(32)).view(F)
            depth[y, x] = d
            index[y, x] = np.int32(np.uint32(key & np.uint64(0xFFFFFFFF)))
            near[y, x] = F(d - F(ma + F(mr * d)))
            n += 1
    return dict(depth=depth, index=index, near=near, n_measured=n)


def empty(W, H):
    return np.full(W * H, EMPTY, np.uint64)


# ------------------------------------------------------------------------------------------------------------------------------- the clouds
def _pix_point(cam, u, v, z):
    """The camera-frame point that projects to (u, v) at depth z, in float64."""
    return np.array([(u - float(cam.cx)) * z / float(cam.fx), (v - float(cam.cy)) * z / float(cam.fy), z], np.float64)


def _nudged(cam, axis, other, z, want):
    """A camera-frame float32 point at depth z (identity pose) whose projected coordinate on `axis` — by the float32 rule, before the floor —
    satisfies want(value); the other axis lands in pixel `other`.  Found by stepping the coordinate through neighbouring floats."""
    f, c = (cam.fx, cam.cx) if axis == 0 else (cam.fy, cam.cy)
    for zz in (F(z), F(3.0), F(1.5), F(5.0), F(2.5), F(7.0), F(1.25), F(6.0), F(4.0), F(9.0)):   # (an exact value is not on every depth's lattice)
        q = F((want.target - float(c)) * float(zz) / float(f))
        for _ in range(48):
            q = np.nextafter(q, F(-np.inf))
        for _ in range(97):
            if want(F(F(F(q * f) / zz) + c)):
                p = _pix_point(cam, other + 0.5, other + 0.5, float(zz)).astype(F)
                p[axis] = q
                return p
            q = np.nextafter(q, F(np.inf))
    raise AssertionError(f"no float32 coordinate projects as wanted on axis {axis}")


class _Want:
    def __init__(self, target, lo, hi):
        self.target, self.lo, self.hi = target, lo, hi

    def __call__(self, v):
        return self.lo <= float(v) <= self.hi


def planted(cam):
    """(points float32 [K,3] in the IDENTITY camera's frame, notes): the cases the issue lists.  notes["equal_z"] = (k_a, k_b): the two planted rows
    with the same coordinates, so bit-equal z on one pixel under every pose."""
    W, H = cam.image_width, cam.image_height
    P = lambda u, v, z: _pix_point(cam, u, v, z).astype(F)
    rows = [P(3.5, 2.5, 4.0), P(3.5, 2.5, 2.0), P(3.5, 2.5, 3.0),                 # three on one pixel, different z
            P(1.5, 1.5, 5.0), P(1.5, 1.5, 2.5),                                    # two on one pixel, different z
            P(2.5, 0.5, 0.25), P(2.5, 0.5, 6.0), P(2.5, 0.5, 0.25)]                 # rows 5 and 7: bit-equal z (nearer than every random return), the lower index must win
    rows += [np.array(v, F) for v in ([0.1, 0.1, 0.0], [0.1, 0.1, -2.0], [0.0, 0.0, np.nan], [0.0, 0.0, np.inf], [np.nan, 0.0, 2.0])]
    rows.append((-_pix_point(cam, 2.5, 1.5, 3.0)).astype(F))                       # behind the camera, and it would land inside the image
    for axis, size in ((0, W), (1, H)):
        rows.append(_nudged(cam, axis, 1, 2.0, _Want(-0.5, -0.75, -0.25)))          # -0.5: floor -1, dropped
        rows.append(_nudged(cam, axis, 1, 2.0, _Want(0.0, 0.0, 0.0)))              # exactly 0: kept
        rows.append(_nudged(cam, axis, 1, 2.0, _Want(size - 1e-3, size - 0.01, float(np.nextafter(F(size), F(0))))))   # just below the size: kept
        rows.append(_nudged(cam, axis, 1, 2.0, _Want(float(size), float(size), float(size))))   # exactly the size: dropped
    return np.stack(rows), dict(equal_z=(5, 7), edges=len(rows) - 8)


@functools.lru_cache(maxsize=None)
def cloud(W, H, n, view=None, seed=0, plant=True):
    """(points float32 [n,3] in the WORLD frame of synthetic_camera(W, H, view), notes).  Random returns around the image (a fifth outside it), depth
    in [0.5, 20); from n = 63 on (unless plant=False) the planted rows stand at scattered indices (notes["planted"][k] = index of planted row k).  Generated in the
    camera frame and moved into the pose in float64, rounded once."""
    cam = camera(W, H, view)
    rng = np.random.default_rng(1000 * seed + 17 * n + W)
    u, v = rng.uniform(-0.1 * W, 1.1 * W, n), rng.uniform(-0.1 * H, 1.1 * H, n)
    z = rng.uniform(0.5, 20.0, n)
    pc = np.stack([(u - float(cam.cx)) * z / float(cam.fx), (v - float(cam.cy)) * z / float(cam.fy), z], 1) if n else np.zeros((0, 3))
    notes = dict(planted=None)
    if n == 1:
        pc[0] = _pix_point(cam, 0.4 * W, 0.6 * H, 3.0)
    if n >= 63 and plant:
        pl, pn = planted(camera(W, H, None))
        at = np.sort(rng.permutation(n)[:pl.shape[0]])
        pc[at] = pl.astype(np.float64)
        notes = dict(planted=at, equal_z=(int(at[pn["equal_z"][0]]), int(at[pn["equal_z"][1]])))
    with np.errstate(all="ignore"):
        world = pc @ np.asarray(cam.R_wc, np.float64).T + np.asarray(cam.t_wc, np.float64) if view is not None else pc
    pts = np.ascontiguousarray(world.astype(F))
    pts.setflags(write=False)
    return pts, notes


@functools.lru_cache(maxsize=None)
def zbuffer_of(W, H, n, view=None, seed=0):
    """The reference z-buffer of cloud(W, H, n, view, seed) seen from its camera (read-only)."""
    cam = camera(W, H, view)
    R, t = pose_f32(cam)
    zb = zbuffer_add(empty(W, H), cloud(W, H, n, view, seed)[0], R, t, cam.fx, cam.fy, cam.cx, cam.cy, W, H)
    zb.setflags(write=False)
    return zb


@functools.lru_cache(maxsize=None)
def images_of(W, H, n, view=None, footprint=0, margins=(0.0, 0.0), seed=0):
    return resolve(zbuffer_of(W, H, n, view, seed), W, H, footprint, *margins)
