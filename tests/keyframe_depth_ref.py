"""The numpy restatement of the keyframe store's three depth rules (include/gslic_hip.h, gslic_keyframe_decode_depth / gslic_keyframe_encode_depth):
storage as 16-bit codes of a power-of-two step, encode, decode at a pyramid level as the unsigned minimum of integer keys — and the seeded frames
with the edge values the CPU and GPU tests share.  No GPU, no library."""
import numpy as np

import keyframe_ref as kref

MAX_LEVEL = kref.MAX_LEVEL
DEFAULT_STEP = np.float32(2.0 ** -9)
MAX_CODE = 65535
NO_RETURN = np.uint32(0xffffffff)   # above every key: a key is at most (65535 << 8) | 255


def step_ok(step):
    """float32 2^e with -16 <= e <= 0."""
    s = np.float32(step)
    if not (s > 0 and s <= 1):
        return False
    m, e = np.frexp(s)
    return bool(m == 0.5 and -15 <= e <= 1)


def encode(depth, step=DEFAULT_STEP):
    """float32 [...] -> uint16 codes: measured iff d > 0 and finite; t = d * (1/step) (exact), k = floor(t + 0.5) in float32; the code is k where
    1 <= k <= 65535, else 0 (sub-half-step and out-of-range depths are NOT MEASURED, never clamped)."""
    assert step_ok(step)
    d = np.asarray(depth, np.float32)
    inv = np.float32(1.0) / np.float32(step)
    with np.errstate(invalid="ignore", over="ignore"):
        measured = (d > 0) & np.isfinite(d)
        t = (np.where(measured, d, np.float32(0.0)).astype(np.float32) * inv).astype(np.float32)
        k = np.floor((t + np.float32(0.5)).astype(np.float32))
        ok = measured & (k >= 1) & (k <= MAX_CODE)
    return np.where(ok, k, 0).astype(np.uint16)


def encode_weight(weight):
    """The mask's byte rule (keyframe_ref.quantise)."""
    return kref.quantise(weight)


def keys(codes, wcodes=None):
    """uint32 key per pixel: the code, or (code << 8) | (255 - wcode) with weights; NO_RETURN where the code is 0."""
    c = np.asarray(codes).astype(np.uint32)
    k = c if wcodes is None else (c << np.uint32(8)) | (np.uint32(255) - np.asarray(wcodes).astype(np.uint32))
    return np.where(c != 0, k, NO_RETURN).astype(np.uint32)


def decode(codes, wcodes=None, level=0, step=DEFAULT_STEP):
    """codes uint16 [H,W] (wcodes uint8 [H,W] or None) -> depth float32 [H_l,W_l], or (depth, weight) with wcodes: per block the unsigned minimum m
    of the keys; depth = (float)code(m) * step, weight = (float)(255 - (m & 255)) * float32(1/255); both 0 where the block has no measured pixel."""
    assert np.asarray(codes).dtype == np.uint16 and (wcodes is None or np.asarray(wcodes).dtype == np.uint8)
    H, W = np.asarray(codes).shape
    Wl, Hl = kref.level_size(W, H, level)
    assert Wl >= 1 and Hl >= 1
    n = 1 << level
    m = keys(codes, wcodes)[:Hl * n, :Wl * n].reshape(Hl, n, Wl, n).min(axis=(1, 3))
    some = m != NO_RETURN
    code = m if wcodes is None else m >> np.uint32(8)
    depth = np.where(some, (code.astype(np.float32) * np.float32(step)).astype(np.float32), np.float32(0.0)).astype(np.float32)
    if wcodes is None:
        return depth
    w = ((np.uint32(255) - (m & np.uint32(255))).astype(np.float32) * kref.C0).astype(np.float32)
    return depth, np.where(some, w, np.float32(0.0)).astype(np.float32)


def quantised(depth, step=DEFAULT_STEP):
    """The code-rounded depth image: decode_0(encode(D))."""
    return decode(encode(depth, step), None, 0, step)


def edge_depths(step=DEFAULT_STEP):
    """{name: float32 array} of the depths a frame must hold besides ordinary ones."""
    s = np.float32(step)
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf), dtype=np.float32)
    dn = lambda v: np.nextafter(np.float32(v), np.float32(-np.inf), dtype=np.float32)
    half = np.float32(s * np.float32(0.5))
    bound = np.array([(k + 0.5) for k in (1, 2, 77, 1000, 40000, 65533)], np.float32) * s     # code boundaries: exact products
    last = np.float32(MAX_CODE) * s
    past = np.float32(MAX_CODE + 0.5) * s                                                      # the first depth beyond the range
    return dict(
        below_boundary=dn(bound), at_boundary=bound, above_boundary=up(bound),
        below_half_step=np.array([half * np.float32(0.999), half * np.float32(0.5), np.float32(1e-30), np.float32(1e-45)], np.float32),
        half_step=np.array([half, dn(half)], np.float32),   # (the float32 below step / 2: t + 0.5f rounds to 1.0f, so the rule's k is 1 as well)
        last_code=np.array([last, dn(past), np.float32(last - s * np.float32(0.25))], np.float32),
        beyond=np.array([past, up(past), np.float32(MAX_CODE + 1) * s, np.float32(1e9), np.float32(3.4e38)], np.float32),
        not_finite_or_positive=np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, -1e-45], np.float32))


def random_depth_frames(n, W, H, seed, step=DEFAULT_STEP):
    """n seeded frames: depth float32 [n,H,W] and weight float32 [n,H,W].  About a third of the pixels are unmeasured (0); the measured ones come
    from a few dozen depth values per frame, so that blocks hold TIES of one code under different weights; every edge depth of edge_depths() is
    written into every frame (as many as fit, cycling through the kinds), at seeded positions."""
    rng = np.random.default_rng(seed)
    s = np.float32(step)
    depth = np.zeros((n, H, W), np.float32)
    weight = rng.uniform(-0.1, 1.1, (n, H, W)).astype(np.float32)
    edges = edge_depths(step)
    order = [v for vals in zip(*[np.resize(a, 8) for a in edges.values()]) for v in vals]     # round-robin over the kinds
    for f in range(n):
        palette = (rng.integers(2, 60000, 24).astype(np.float32) * s + rng.uniform(-0.4, 0.4, 24).astype(np.float32) * s).astype(np.float32)
        d = palette[rng.integers(0, 24, (H, W))]
        d[rng.random((H, W)) < 0.35] = 0.0
        at = rng.permutation(H * W)[:len(order)]
        d.reshape(-1)[at] = np.array(order[:at.size], np.float32)
        depth[f] = d
    return depth, weight
