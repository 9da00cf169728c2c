"""The masked, bias-correction-free Adam of adam_scalar (csrc/gslic_common.h) evaluated with numpy, one rounded operation at a time.

adam_scalar is three statements under `#pragma clang fp contract(off)`:

    m = b1 * m + (1.0f - b1) * g;
    v = b2 * v + (1.0f - b2) * g * g;          // C associates to the left: ((1 - b2) * g) * g
    p += -lr * m / (sqrtf(v) + eps);           // ((-lr) * m) / (sqrtf(v) + eps)

Every operation in it is a correctly rounded IEEE fp32 operation (the library is built with correctly rounded divide and sqrt), and numpy's
float32 +, -, *, / and sqrt are correctly rounded too, so adam_ref() evaluated in the same order gives the same bits: the GPU tests compare
`.view(np.uint32)`, with no tolerance (on an MI355X every case of tests/test_adam_paths_gpu.py matches to the bit: no distance in ulps is in
use anywhere).  The scalars lr, b1, b2, eps are rounded to float32 first, as the C ABI (float arguments) does.

The one thing IEEE leaves to the machine is what happens below 2^-126: adam_ref() therefore also returns a per-element `subnormal` flag, true
where an input, an intermediate or a result is non-zero and smaller than 2^-126 in magnitude.  Tests leave those elements out and assert (on the
CPU) that their inputs produce none, so the GPU's fp32 denormal mode never decides a test.

adam_ref64() is the same sequence in float64 on the float32-rounded scalars, for the CPU self-check of the reference against the C oracle.

Also here, numpy only: the float4 / row bookkeeping the GPU tests rely on (quad_rows, quad_kinds) and three deliberately WRONG evaluations
(adam_wrong_*), each the outcome of one plausible kernel mistake; tests/test_adam_ref_cpu.py asserts that the inputs of the GPU cases tell every
one of them from adam_ref.
"""
import numpy as np

TINY = np.float32(2.0 ** -126)     # smallest normal float32


def _sub(x):
    """Non-zero and below the smallest normal (NaN and Inf compare false)."""
    a = np.abs(x)
    return (a > 0) & (a < TINY)


def _as_rows(x, dtype):
    x = np.ascontiguousarray(x, dtype)
    assert x.ndim == 2, "adam_ref works on [N, M] arrays"
    return x


def _visible_rows(vis, N):
    vis = np.asarray(vis)
    assert vis.shape == (N,)
    return (vis != 0)[:, None]          # a row is updated when its byte is not 0 (any of 1, 2, 255, True)


def adam_ref(p, g, m, v, vis, lr, b1, b2, eps):
    """(p', m', v', subnormal) for float32 [N, M] arrays p, g, m, v and a visibility array [N] (bool or bytes): rows with vis != 0 get the update,
    every other row is copied through bit for bit.  subnormal [N, M] bool: see the module docstring (all False on rows that are not updated)."""
    f32 = np.float32
    p, g, m, v = (_as_rows(x, f32) for x in (p, g, m, v))
    lr, b1, b2, eps = f32(lr), f32(b1), f32(b2), f32(eps)
    upd = _visible_rows(vis, p.shape[0])
    sub = np.zeros(p.shape, bool)

    def keep(x):        # every intermediate passes through here: float32 it must be, and it is looked at for the flag
        assert x.dtype == f32, x.dtype
        np.logical_or(sub, _sub(x), out=sub)
        return x

    with np.errstate(all="ignore"):
        for x in (p, g, m, v):
            keep(x)
        one_b1 = keep(f32(1) - b1)
        m1 = keep(keep(b1 * m) + keep(one_b1 * g))
        one_b2 = keep(f32(1) - b2)
        v1 = keep(keep(b2 * v) + keep(keep(one_b2 * g) * g))
        neg_lr = -lr
        p1 = keep(p + keep(keep(neg_lr * m1) / keep(keep(np.sqrt(v1)) + eps)))
    sub |= bool(_sub(lr) or _sub(b1) or _sub(b2) or _sub(eps))
    return np.where(upd, p1, p), np.where(upd, m1, m), np.where(upd, v1, v), sub & upd


def adam_ref64(p, g, m, v, vis, lr, b1, b2, eps):
    """The float64 twin: the same statements in the same order on float64 arrays, the four scalars first rounded to float32 (what the library
    receives) and then widened.  Returns (p', m', v')."""
    f64 = np.float64
    p, g, m, v = (_as_rows(x, f64) for x in (p, g, m, v))
    lr, b1, b2, eps = (f64(np.float32(x)) for x in (lr, b1, b2, eps))
    upd = _visible_rows(vis, p.shape[0])
    with np.errstate(all="ignore"):
        m1 = b1 * m + (1.0 - b1) * g
        v1 = b2 * v + ((1.0 - b2) * g) * g
        p1 = p + ((-lr) * m1) / (np.sqrt(v1) + eps)
    return np.where(upd, p1, p), np.where(upd, m1, m), np.where(upd, v1, v)


def same_bits(a, b):
    """Boolean array: a and b hold the same float32 bit patterns."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.view(np.uint32) == b.view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# float4 / row bookkeeping: the kernel walks a group's N*M scalars as float4 "quads" q = scalars [4q, 4q+3] (row of scalar e: e // M) and a scalar
# tail of N*M % 4 elements behind the last whole quad.

def quad_rows(N, M):
    """int64 [N*M // 4, 4]: the row of each of the four scalars of every whole quad."""
    nq = (N * M) // 4
    return (np.arange(4 * nq, dtype=np.int64) // M).reshape(nq, 4)


def quad_kinds(vis, M):
    """Per whole quad: 0 = all four scalars on invisible rows (the kernel issues no traffic), 1 = all on visible rows, 2 = mixed."""
    vis = np.asarray(vis) != 0
    r = quad_rows(vis.shape[0], M)
    n = vis[r].sum(1)
    return np.where(n == 0, 0, np.where(n == 4, 1, 2)).astype(np.int8)


def tail_elements(N, M):
    """Flat indices of the scalar tail behind the last whole quad."""
    return np.arange((N * M) // 4 * 4, N * M)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# What a kernel with one mistake would compute.  Each returns (p', m', v') like adam_ref without the flag.

def _blend(take, new, old):
    return tuple(np.where(take, n, o) for n, o in zip(new, old))


def adam_wrong_quad_visibility(p, g, m, v, vis, lr, b1, b2, eps):
    """Every whole quad takes the visibility of its FIRST scalar's row for all four scalars (the tail is right)."""
    N, M = p.shape
    full = adam_ref(p, g, m, v, np.ones(N, np.uint8), lr, b1, b2, eps)[:3]
    take = np.repeat(np.asarray(vis) != 0, M)
    nq = (N * M) // 4
    take[:4 * nq] = np.repeat(take[:4 * nq:4], 4)
    return _blend(take.reshape(N, M), full, (p, m, v))


def adam_wrong_tail_skipped(p, g, m, v, vis, lr, b1, b2, eps):
    """The N*M % 4 scalars behind the last whole quad are never updated."""
    N, M = p.shape
    right = adam_ref(p, g, m, v, vis, lr, b1, b2, eps)[:3]
    take = np.ones(N * M, bool)
    take[tail_elements(N, M)] = False
    return _blend(take.reshape(N, M), right, (p, m, v))


def adam_wrong_groups_past_eight(groups, vis, b1, b2, eps):
    """groups: list of (p, g, m, v, lr).  Only the first eight are updated; the others come back unchanged."""
    out = []
    for i, (p, g, m, v, lr) in enumerate(groups):
        out.append(adam_ref(p, g, m, v, vis, lr, b1, b2, eps)[:3] if i < 8 else (p, m, v))
    return out
