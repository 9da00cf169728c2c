"""Inputs of the Adam path tests (numpy only): one definition for tests/test_adam_paths_gpu.py, which runs them through the kernels, and for
tests/test_adam_ref_cpu.py, which checks on the CPU that none of them reaches below 2^-126 and that each tells a wrong kernel from a right one."""
import numpy as np

LR, B1, B2, EPS = 1.6e-4, 0.9, 0.999, 1e-15      # the values of test_adam_parity (eps: trainer.GaussianModel.training_setup)
HYPER = dict(lr=LR, b1=B1, b2=B2, eps=EPS)


def tensors(N, M, seed, scale=1.0):
    """(p, g, m, v) float32 [N, M] with test_adam_parity's distributions times `scale` (v: times scale^2, like the fuzz)."""
    rng = np.random.default_rng(seed)
    p = (scale * rng.standard_normal((N, M))).astype(np.float32)
    g = (scale * rng.standard_normal((N, M))).astype(np.float32)
    m = (0.1 * scale * rng.standard_normal((N, M))).astype(np.float32)
    v = (0.01 * scale * scale * rng.random((N, M))).astype(np.float32)
    return p, g, m, v


def mask(N, seed, frac=0.6):
    """uint8 [N] random mask, first and last row visible (the scalar tail lives in the last row)."""
    vis = (np.random.default_rng(seed).random(N) < frac).astype(np.uint8)
    vis[0] = vis[-1] = 1
    return vis


# (a) unaligned bases: offsets in floats for (param, grad, exp_avg, exp_avg_sq)
A_SHAPES = [(700, 3), (700, 1)]
A_WHICH = ("param", "grad", "exp_avg", "exp_avg_sq", "all")


def a_offsets(which, off):
    return tuple(off if which in (n, "all") else 0 for n in ("param", "grad", "exp_avg", "exp_avg_sq"))


# (b) tails behind an aligned base: N*M % 4 in {1, 2, 3} for every instantiation (M = 1, 3, 45, 4 compile-time; the others run adam_span<0>)
B_SHAPES = [(5, 1), (333, 3), (11, 45), (3, 4), (101, 7), (33, 2), (13, 5), (9, 64), (1, 1), (1, 3), (1, 45)]

# (c) quads that straddle rows of different visibility
C_N = 1025
C_WIDTHS = (3, 45, 7, 1)
C_PATTERNS = ("0101", "0011", "row0", "rowlast", "none", "all", "runs", "bytes")
_RUNS = (1, 4, 1, 5, 2, 7, 1, 9, 3, 4, 1, 6, 1, 8)      # visible, invisible, visible, ... run lengths (every invisible run >= 4)


def vis_pattern(name, N):
    i = np.arange(N)
    if name == "0101":
        return (i % 2).astype(np.uint8)
    if name == "0011":
        return ((i // 2) % 2).astype(np.uint8)
    if name in ("row0", "rowlast", "none"):
        vis = np.zeros(N, np.uint8)
        if name != "none":
            vis[0 if name == "row0" else N - 1] = 1
        return vis
    if name == "all":
        return np.ones(N, np.uint8)
    if name == "runs":
        period = np.concatenate([np.full(n, 1 - k % 2, np.uint8) for k, n in enumerate(_RUNS)])
        return np.resize(period, N)
    if name == "bytes":       # any non-zero byte is "visible"
        return np.resize(np.array([2, 0, 255, 0, 0, 255, 2, 2, 0], np.uint8), N)
    raise KeyError(name)


# (d) threads take a second grid-stride trip (blocks are capped at 8192: 8192 * 256 quads = 8 388 608 scalars).  186 500 * 45 = 8 392 500 is a
# multiple of 4: the second shape, one row more, puts a scalar tail behind the second trip
D_SHAPES = [(186500, 45), (186501, 45)]

# (e) more than eight groups in one call: two launches, and narrow groups in a grid sized for M = 45
E_N = 777
E_WIDTHS = (1, 3, 4, 45, 7, 2, 1, 3, 5, 45, 4)
E_LRS = tuple(1.6e-4 * (1.0 + 0.37 * i) for i in range(len(E_WIDTHS)))
E_OFFSETS = {2: (1, 0, 0, 0), 9: (3, 3, 3, 3)}        # group index -> float offsets of (param, grad, exp_avg, exp_avg_sq); the rest aligned


def e_groups():
    """[(p, g, m, v, lr)] of case (e)."""
    return [tensors(E_N, M, 500 + i) + (E_LRS[i],) for i, M in enumerate(E_WIDTHS)]


# (f) value edges on (257, 3), every row visible
F_SHAPE = (257, 3)
F_SCALES = (1e-12, 1.0, 1e4)
F_ZERO, F_V0, F_NEG0 = slice(0, 40), slice(40, 80), slice(80, 120)      # flat element ranges of the three overlays
F_NAN, F_INF = 401, 610                                                 # flat elements of the NaN and the Inf gradient (quads 100 and 152)


def f_tensors(scale, nonfinite=False):
    p, g, m, v = tensors(*F_SHAPE, seed=600, scale=scale)
    for x in (p, g, m, v):
        x.shape = (-1,)
    g[F_ZERO] = 0; m[F_ZERO] = 0; v[F_ZERO] = 0          # nothing to do: p must come back unchanged
    v[F_V0] = 0                                          # first step of a moment with history in m only
    g[F_V0.start:F_V0.start + 8] = 0                     # ... eight of them with g = 0 too: the step is -lr m / eps
    g[F_NEG0] = -0.0
    if nonfinite:
        g[F_NAN] = np.nan
        g[F_INF] = np.inf
    for x in (p, g, m, v):
        x.shape = F_SHAPE
    return p, g, m, v


# (g) - (j): the six groups of a model
MODEL_P = 1061
GROUP_WIDTHS = {3: (3, 3, 45, 1, 3, 4), 0: (3, 3, 0, 1, 3, 4)}        # by SH degree: xyz, features_dc, features_rest, opacity, scaling, rotation
CHUNKS = 5                                                             # _ChunkedExchange(1061, ., 5): bounds at multiples of 256, last n = 37


def moments(P, widths, seed):
    """[(m, v)] per group, [P, M] float32 (None for an empty group): non-zero history, v >= 0."""
    rng = np.random.default_rng(seed)
    out = []
    for M in widths:
        out.append(None if M == 0 else ((0.1 * rng.standard_normal((P, M))).astype(np.float32), (0.01 * rng.random((P, M))).astype(np.float32)))
    return out


def small_grads(P, seed):
    """dL_dxyz [P,3], dL_dopacity [P,1], dL_dscaling [P,3], dL_drotation [P,4]: what the all-reduce delivers."""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((P, M)).astype(np.float32) for M in (3, 1, 3, 4)]


def view_masks(P, n_views):
    """uint8 [n_views, P]: row r is seen by no view, by exactly view k (each in turn) or by all, as r runs through a cycle of n_views + 2."""
    k = np.arange(P) % (n_views + 2)
    return np.stack([((k == v + 1) | (k == n_views + 1)) for v in range(n_views)]).astype(np.uint8)


def view_payload(P, n_views, seed):
    """(rgb_all [n_views, P, 3] float32 — zero where the view does not see the row, like the backward writes it —, campos_all [n_views, 3], masks)."""
    rng = np.random.default_rng(seed)
    masks = view_masks(P, n_views)
    rgb = rng.standard_normal((n_views, P, 3)).astype(np.float32) * masks[:, :, None]
    campos = (np.array([[0.3, -0.2, -4.0]]) + 0.5 * rng.standard_normal((n_views, 3))).astype(np.float32)
    return rgb, campos, masks
