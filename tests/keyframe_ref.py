"""The numpy restatement of the keyframe store's three rules (include/gslic_hip.h, gslic_keyframe_decode / gslic_keyframe_encode): storage, decode
at a pyramid level, encode — and the edge values and pooling helpers the CPU and GPU tests share.  No GPU, no library."""
import numpy as np

MAX_LEVEL = 4
C0 = np.float32(1.0) / np.float32(255.0)   # float32(1/255): the float32 quotient


def scale(level):
    """c_l = float32(1/255) * 2^(-2l): exact."""
    return np.float32(C0 * np.float32(2.0 ** (-2 * int(level))))


def level_size(W, H, level):
    """(W_l, H_l); either may be 0: the level does not exist."""
    return int(W) >> int(level), int(H) >> int(level)


def levels(W, H, top=MAX_LEVEL):
    """The levels 0 .. top a W x H image admits."""
    return [l for l in range(top + 1) if min(level_size(W, H, l)) >= 1]


def block_sums(u8, level):
    """Integer sums of the 4^l bytes of every block: u8 [H,W] or [H,W,C] -> uint32 [H_l,W_l] or [H_l,W_l,C]; remainder columns and rows dropped."""
    a = np.asarray(u8)
    assert a.dtype == np.uint8
    H, W = a.shape[:2]
    Wl, Hl = level_size(W, H, level)
    assert Wl >= 1 and Hl >= 1
    n = 1 << level
    a = a[:Hl * n, :Wl * n].astype(np.uint32)
    return a.reshape((Hl, n, Wl, n) + a.shape[2:]).sum(axis=(1, 3), dtype=np.uint32)


def decode(u8, level=0):
    """The decode rule: (float)S * c_l, one float32 multiply.  u8 [H,W,3] -> float32 [3,H_l,W_l] (planar); u8 [H,W] (a mask) -> float32 [H_l,W_l]."""
    S = block_sums(u8, level)
    out = (S.astype(np.float32) * scale(level)).astype(np.float32)
    return np.ascontiguousarray(out.transpose(2, 0, 1)) if out.ndim == 3 else out


def quantise(x):
    """The encode rule per value: x' = x clamped to [0, 1] (NaN -> 0), q = (uint8) floor(fl(x' * 255) + 0.5), every step a float32 operation."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        xc = np.where(x > 0, np.where(x < 1, x, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
    p = (xc * np.float32(255.0)).astype(np.float32)
    return np.floor((p + np.float32(0.5)).astype(np.float32)).astype(np.uint8)


def encode(image):
    """float32 [3,H,W] -> uint8 [H,W,3] (interleaved); float32 [H,W] (a mask) -> uint8 [H,W]."""
    q = quantise(image)
    return np.ascontiguousarray(q.transpose(1, 2, 0)) if q.ndim == 3 else q


def quantise_exact(x):
    """The same rule for ONE float32 value through exact arithmetic: the product x' * 255 is exact in float64 (24 + 8 bits), rounded to float32
    once; adding 0.5 is exact in float64 too, rounded to float32 once; then floor.  Independent of numpy's float32 arithmetic."""
    x = float(np.float32(x))
    xc = (x if x < 1.0 else 1.0) if x > 0.0 else 0.0
    p = float(np.float32(xc * 255.0))
    return int(np.floor(float(np.float32(p + 0.5))))


def _ulp_step(v, up):
    return np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf), dtype=np.float32)


def edge_values():
    """(values float32 [n], expected bytes uint8 [n] by quantise_exact): for every k the decoded value d(k) = k c_0 and the float32 quotient k / 255,
    each with its two float32 neighbours; the midpoints (k + 0.5) / 255 with their neighbours; NaN, +-inf, -0.0, the values around 0 and 1."""
    vals = []
    k = np.arange(256, dtype=np.float32)
    for centre in (k * C0, k / np.float32(255.0), (k + np.float32(0.5)) / np.float32(255.0)):
        centre = centre.astype(np.float32)
        vals += [centre, _ulp_step(centre, True), _ulp_step(centre, False)]
    one = np.float32(1.0)
    vals.append(np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, _ulp_step(one, True), _ulp_step(one, False), 2.0, -1.0, 1e-45, -1e-45, 3.4e38, -3.4e38], np.float32))
    v = np.concatenate(vals).astype(np.float32)
    return v, np.array([quantise_exact(x) for x in v], np.uint8)


def positive_min_pool(depth, level):
    """Per 2^l x 2^l block the smallest POSITIVE value, 0 where the block has none (remainder columns and rows dropped): what a LiDAR range image
    of the level-l camera is, given the level-0 image (0 = no return)."""
    d = np.asarray(depth, np.float32)
    H, W = d.shape
    Wl, Hl = level_size(W, H, level)
    n = 1 << level
    b = d[:Hl * n, :Wl * n].reshape(Hl, n, Wl, n)
    m = np.where(b > 0, b, np.float32(np.inf)).min(axis=(1, 3))
    return np.where(np.isinf(m), np.float32(0.0), m).astype(np.float32)


def random_frames(n, W, H, seed, masks=False):
    """n seeded frames of random bytes, uint8 [n,H,W,3], and (masks=True) as many masks uint8 [n,H,W] (None otherwise)."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    m = rng.integers(0, 256, (n, H, W), dtype=np.uint8) if masks else None
    return f, m
