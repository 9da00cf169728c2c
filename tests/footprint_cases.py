"""Scenes whose FOOTPRINTS and ROW BLOCKS are designed, for the forward's front end (csrc/preprocess.hip: preprocess_kernel, keybuild_kernel,
finalize_ranges_kernel; the tile grouping and the scans behind them): every switch of those kernels is reached on purpose —
  SEQ_TILES = 16   a rectangle of up to 16 tiles is tested by its own lane (the result travels as `seqmask`), larger ones are swept by the wave,
                   64 tiles per step from tile 16 on: 16 | 17, 80 | 81, 144 | 145, several swept lanes in a wave, a swept lane between culled ones;
  KB_CAP = 1024    a wave whose rows emit at most 1024 instances stages them in LDS, a larger one stores directly: 1024 | 1025;
  LDS_SH           (M == 15, D > 0) SH rows pass through LDS in two half-blocks of 32 rows as float4 columns, fetched only where a visible row
                   touches them; short last blocks take the scalar copy;  M == 15 with D == 0 leaves for the 256-thread kernel;
  the culls        vz <= 0.2f, op < 1 / 255, a rectangle clamped to nothing, a rectangle none of whose tiles passes (cnt == 0);
  get_rect         the border clamps and the literal rounding order ((p + r) + 16) - 1.
No GPU, no library: numpy and the scene generator only.  The numpy restatements below (get_rect, the tile count's schedule, the staging rule,
the float4 column predicate) serve the DESIGN checks of tests/test_footprint_cases_cpu.py — what a scene reaches, and which wrong rule it would
expose — never as the yardstick of a GPU test: that is the CPU oracle.

The construction.  Identity pose, so depth is z.  A Gaussian that is to have the mean (mx, my) in image coordinates sits at
x = (mx + 1/2 - cx) z / fx (tile_lists.build's formula: the projection puts x fx / z + cx - 1/2 into the image); its scale is solved in float64
so that 3 sqrt(lambda_1) lies half a pixel below the wanted integer radius.  Isotropic Gaussians have opacity 0.99: the exact tile test then
keeps whatever lies within the radius.  A rectangle of n tiles in a one-tile-high image: n = 2 k + 1 has the mean in the middle of a tile and
radius 16 k (3 for k = 0), n = 2 k the mean on a tile boundary and radius 16 k - 8 — both keep (mx -+ r) / 16 half a tile from an integer.

Every builder returns dict(raw, act, sc, camd, cam, plan): the raw parameters (for the raw-parameter path), synthetic.activate's tensors (what
hip_forward takes as act=), their numpy view for the oracle — the same bits on both sides — and the plan of what was designed."""
import math

import numpy as np
import torch

from gaussian_lic_amd.camera import synthetic_camera
from gaussian_lic_amd.synthetic import activate, to_numpy

SEQ_TILES, SWEEP, KB_CAP, SCAN_TILE = 16, 64, 1024, 4096
OPACITY = 0.99
STRIP_W, STRIP_H, STRIP_GX = 16 * 160, 16, 160
STRIP_SIZES = (1, 2, 15, 16, 17, 18, 79, 80, 81, 143, 144, 145, 160)
STRIP_LANES = (0, 31, 32, 63)
ROW_COUNTS = (255, 256, 257, 4095, 4096, 4097, 8193)
SH_P = (1, 31, 32, 33, 63, 64, 65, 97, 128 + 45)
SH_SINGLE = (0, 1, 2, 3, 30, 31, 32, 33, 62, 63)
SH_PATTERNS = ("all",) + tuple(f"single-{r}" for r in SH_SINGLE) + ("alternate", "none")
SH_LDS = ((1, 15), (2, 15), (3, 15))             # (D, M) of preprocess_kernel<true, 64>
SH_PLAIN = ((0, 15), (0, 0), (1, 3), (2, 8))     # ... of preprocess_kernel<false, 256>
F32 = np.float32


# ------------------------------------------------------------------------------------------------ numpy restatements (design checks only)
def trunc_clamped(v, hi):
    v = np.asarray(v, F32)
    with np.errstate(invalid="ignore"):
        i = np.clip(np.where(np.isfinite(v), v, 0).astype(np.int64), 0, hi)      # (C truncation towards zero)
        return np.where(~(v > F32(-1.0)), 0, np.where(v >= F32(hi + 1), hi, i)).astype(np.int64)


def get_rect(px, py, radius, gx, gy, plus15=False):
    """getRect (auxiliary.h:46-56) in float32 and in the reference's LITERAL operation order ((p + r) + 16) - 1; plus15=True is the wrong
    rule (p + r) + 15.  Returns int64 arrays x0, y0, x1, y1."""
    px, py, r, t = np.asarray(px, F32), np.asarray(py, F32), np.asarray(radius).astype(F32), F32(16.0)
    hi = (lambda p: (p + r) + F32(15.0)) if plus15 else (lambda p: ((p + r) + t) - F32(1.0))
    return (trunc_clamped((px - r) / t, gx), trunc_clamped((py - r) / t, gy), trunc_clamped(hi(px) / t, gx), trunc_clamped(hi(py) / t, gy))


def rect_tiles(rect):
    x0, y0, x1, y1 = rect
    return (x1 - x0) * (y1 - y0)


def scheduled_count(passed, lane_tiles=SEQ_TILES, sweep_step=SWEEP):
    """tiles_touched of one rectangle as the two-phase schedule of preprocess_kernel counts it.  passed: bool per tile of the rectangle
    (row-major).  The owning lane tests tiles t < min(n, lane_tiles); a rectangle of more than SEQ_TILES tiles is then swept from tile
    SEQ_TILES on, 64 lanes wide, the base advancing by sweep_step.  The right rule is (16, 64); (17, 64) is `t < 16` read as `t <= 16`
    (tile 16 counted twice), (16, 63) a sweep stepping 63 (tiles 79, 142, ... counted twice)."""
    passed = np.asarray(passed, bool)
    n = passed.size
    c = int(passed[:min(n, lane_tiles)].sum())
    if n > SEQ_TILES:
        for base in range(SEQ_TILES, n, sweep_step):
            c += int(passed[base:min(base + SWEEP, n)].sum())
    return c


def staged(wcount, strict=False):
    """keybuild_kernel's choice for a wave of wcount instances: staged in LDS (True) or stored directly.  strict=True is the wrong rule
    `wcount < KB_CAP`.  Both paths must write the same lists, so the two rules differ in the PATH of a wave, not in its output."""
    return wcount < KB_CAP if strict else wcount <= KB_CAP


def wave_totals(tiles_touched):
    """instances per wave of 64 rows (keybuild_kernel's wcount), and the wave's last lane (< 63 only for the partial last wave)"""
    tt = np.asarray(tiles_touched, np.int64)
    P = tt.size
    n = (P + 63) // 64
    return np.add.reduceat(tt, np.arange(0, P, 64)) if P else np.zeros(0, np.int64), np.minimum(P - 1 - 64 * np.arange(n), 63)


def lost_floats(visible, rows, without_second_term=True):
    """LDS_SH staging of one 64-row block: bool [64, 45], True where a float of a VISIBLE row would not reach LDS under the column predicate
    lds_v[e / 45] alone (the wrong rule; the right one also asks lds_v[(e + 3) / 45]).  visible: bool [64]; rows: rows the block has.
    Half-blocks with fewer than 32 rows take the scalar copy and lose nothing."""
    lost = np.zeros((64, 45), bool)
    for h in range(2):
        if min(rows - 32 * h, 32) != 32:
            continue
        v = np.asarray(visible[32 * h:32 * h + 32], bool)
        e = 4 * np.arange(32 * 45 // 4)
        load = v[e // 45] | (False if without_second_term else v[(e + 3) // 45])
        got = np.repeat(load, 4).reshape(32, 45)
        lost[32 * h:32 * h + 32] = ~got & v[:, None]
    return lost


def project32(cam, xyz):
    """means2D of preprocess_kernel in numpy float32 (identity or any pose): hx, hw left to right, pw = 1 / (hw + 1e-7f), ndc2Pix in double"""
    Pm = np.asarray(cam.full_proj_transform, F32).reshape(16)
    p = np.asarray(xyz, F32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    row = lambda k: ((Pm[k] * x + Pm[4 + k] * y) + Pm[8 + k] * z) + Pm[12 + k]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        pw = F32(1.0) / (row(3) + F32(0.0000001))
        to_pix = lambda v, S: ((((v * pw).astype(np.float64) + 1.0) * float(S) - 1.0) * 0.5).astype(F32)
        return to_pix(row(0), cam.image_width), to_pix(row(1), cam.image_height)


# ------------------------------------------------------------------------------------------------ placement
def _xyz(cam, mx, my, z):
    mx, my, z = (np.atleast_1d(np.asarray(v, np.float64)) for v in np.broadcast_arrays(mx, my, z))
    return np.stack([(mx + 0.5 - float(cam.cx)) / float(cam.fx) * z, (my + 0.5 - float(cam.cy)) / float(cam.fy) * z, z], 1)


def _rot_z(deg):
    a = math.radians(deg)
    return np.array([math.cos(a / 2), 0.0, 0.0, math.sin(a / 2)])


def _quat_matrix(q):
    r, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                     [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]])


def radius64(cam, xyz, scales, quat):
    """float64 restatement of computeCov2D's radius for one Gaussian (identity pose): (3 sqrt(lambda_1) before the ceil, det)"""
    x, y, z = (float(v) for v in xyz)
    fx, fy = cam.image_width / (2.0 * float(cam.tanfovx)), cam.image_height / (2.0 * float(cam.tanfovy))
    tx = min(float(cam.limx_pos), max(float(cam.limx_neg), x / z)) * z
    ty = min(float(cam.limy_pos), max(float(cam.limy_neg), y / z)) * z
    J = np.array([[fx / z, 0.0, -fx * tx / (z * z)], [0.0, fy / z, -fy * ty / (z * z)]])
    R = _quat_matrix(np.asarray(quat, np.float64))
    S = R @ np.diag(np.asarray(scales, np.float64) ** 2) @ R.T
    c = J @ S @ J.T
    c0, c1, c2 = c[0, 0] + 0.3, c[0, 1], c[1, 1] + 0.3
    det = c0 * c2 - c1 * c1
    mid = 0.5 * (c0 + c2)
    return 3.0 * math.sqrt(mid + math.sqrt(max(0.1, mid * mid - det))), det


def _solve_scale(cam, xyz, radius, ratios=(1.0, 1.0, 1.0), quat=(1.0, 0.0, 0.0, 0.0)):
    """s with ceil(3 sqrt(lambda_1)) = radius for scales s * ratios, aimed half a pixel below the integer (bisection, float64)"""
    ratios = np.asarray(ratios, np.float64)
    lo, hi = 1e-9, 1e3
    assert radius64(cam, xyz, lo * ratios, quat)[0] < radius - 0.5, "the 0.3 px dilation alone exceeds this radius"
    for _ in range(64):
        mid = math.sqrt(lo * hi)
        if radius64(cam, xyz, mid * ratios, quat)[0] < radius - 0.5:
            lo = mid
        else:
            hi = mid
    return lo * ratios


def strip_rect(n, hint=80):
    """(mx, radius) of a 1 x n rectangle in the strip image, its middle near tile column `hint`"""
    k = n // 2
    if n % 2:
        tx = min(max(hint, k), STRIP_GX - 1 - k)
        return 16.0 * tx + 8.0, (16 * k if k else 3)
    tx = min(max(hint, k), STRIP_GX - k)
    return 16.0 * tx, 16 * k - 8


class _Rows:
    """rows of a scene under construction"""

    def __init__(self, cam, seed):
        self.cam, self.rng = cam, np.random.default_rng(seed)
        self.xyz, self.scales, self.quat, self.opac, self.tag = [], [], [], [], []

    def __len__(self):
        return len(self.xyz)

    def add(self, mx, my, radius, z=None, opacity=OPACITY, ratios=(1.0, 1.0, 1.0), quat=(1.0, 0.0, 0.0, 0.0), tag=""):
        z = float(self.rng.uniform(1.0, 30.0)) if z is None else z
        p = _xyz(self.cam, mx, my, z)[0]
        self.xyz.append(p); self.scales.append(_solve_scale(self.cam, p, radius, ratios, quat)); self.quat.append(np.asarray(quat, np.float64))
        self.opac.append(opacity); self.tag.append(tag)
        return len(self.xyz) - 1

    def culled(self, how, tag="culled"):
        """an invisible row: 'behind' (z = -1), 'near' (z = 0.1) or 'faint' (opacity 0.001 on an otherwise ordinary 1-tile row)"""
        i = self.add(16.0 * int(self.rng.integers(2, 8)) + 8.0, 8.0, 3, z=2.0, opacity=0.001 if how == "faint" else OPACITY, tag=tag)
        if how != "faint":
            self.xyz[i] = np.array([0.01, 0.01, -1.0 if how == "behind" else 0.1])
        return i

    def finish(self, D=0, M=0, sh_seed=0, **plan):
        P = len(self.xyz)
        g = np.random.default_rng(sh_seed)
        lg = lambda p: math.log(p / (1.0 - p))
        # colour: channel 1 + (row mod 2) of every row is far below zero (C0 * -8 + 1/2 = -1.76, beyond what the other fifteen terms add), so
        # it clamps at 0 whatever the degree; channel 0, where a row's first float lives, stays above zero (C0 * 5 + 1/2 = 1.91), so that a lost
        # first float shows; the third channel falls on either side
        dc = g.normal(0.0, 2.0, (P, 1, 3))
        dc[:, 0, 0] = 5.0
        dc[np.arange(P), 0, 1 + np.arange(P) % 2] = -8.0
        raw = dict(xyz=torch.from_numpy(np.asarray(self.xyz, np.float64).reshape(P, 3).astype(F32)).contiguous(),
                   scaling=torch.from_numpy(np.log(np.asarray(self.scales, np.float64).reshape(P, 3)).astype(F32)).contiguous(),
                   rotation=torch.from_numpy(np.asarray(self.quat, np.float64).reshape(P, 4).astype(F32)).contiguous(),
                   opacity=torch.from_numpy(np.array([lg(o) for o in self.opac], np.float64).reshape(P, 1).astype(F32)).contiguous(),
                   features_dc=torch.from_numpy(dc.astype(F32)).contiguous(),
                   features_rest=torch.from_numpy(g.normal(0.0, 0.4, (P, 15, 3)).astype(F32)[:, :M].copy()).contiguous(), sh_degree=int(D))
        return _scene(raw, self.cam, dict(tag=list(self.tag), dropped=[], **plan))


def _scene(raw, cam, plan, act=None):
    act = activate(raw) if act is None else act
    return dict(raw=raw, act=act, sc=to_numpy(act), camd=cam.as_dict(), cam=cam, plan=plan)


def _filler(rows, lane):
    """what stands in a lane nothing was designed for: ordinary 1- to 3-tile rows and the three kinds of invisible row"""
    kind = lane % 5
    if kind == 0:
        return rows.culled(("behind", "near", "faint")[(lane // 5) % 3], tag="filler")
    n = (1, 2, 3, 1)[kind - 1]
    mx, r = strip_rect(n, hint=int(rows.rng.integers(4, 150)))
    return rows.add(mx, 8.0, r, tag="filler")


# ------------------------------------------------------------------------------------------------ scenes
def strip():
    """Every size of STRIP_SIZES at every lane of STRIP_LANES (wave i holds size i), then a wave with five swept rows and a wave with a
    swept row between culled rows, then a partial wave.  plan: sizes [(row, n)], many_swept = its wave, between = (row, wave)."""
    cam = synthetic_camera(STRIP_W, STRIP_H)
    rows = _Rows(cam, 11)
    sizes = []
    for w, n in enumerate(STRIP_SIZES):
        for lane in range(64):
            if lane in STRIP_LANES:
                mx, r = strip_rect(n, hint=80 + (lane % 7) - 3)
                sizes.append((rows.add(mx, 8.0, r, tag=f"size-{n}"), n))
            else:
                _filler(rows, lane)
    many = len(rows) // 64
    swept_at = {3: 20, 17: 33, 40: 81, 41: 17, 63: 100}
    for lane in range(64):
        if lane in swept_at:
            mx, r = strip_rect(swept_at[lane], hint=60 + lane)
            rows.add(mx, 8.0, r, tag="many-swept")
        else:
            _filler(rows, lane)
    between_wave = len(rows) // 64
    between = None
    for lane in range(64):
        if lane in (19, 20, 22, 23):
            rows.culled(("behind", "near", "faint", "behind")[lane % 4], tag="around-swept")
        elif lane == 21:
            mx, r = strip_rect(40, hint=70)
            between = rows.add(mx, 8.0, r, tag="swept-between-culled")
        else:
            _filler(rows, lane)
    for lane in range(17):
        _filler(rows, lane + 1)
    return rows.finish(sizes=sizes, many_swept=many, between=(between, between_wave))


# (n tiles per row of a designed wave; 0 = an invisible row)
_WAVES = (
    ("1024-seqmask", [16] * 64),
    ("1025", [16] * 40 + [17] + [16] * 23),
    ("empty", [0] * 64),
    ("1024-swept", [16] * 10 + [80] + [0] * 6 + [16] * 20 + [100, 80] + [0] * 7 + [16] * 17 + [12]),
    ("thousands", ([160, 16, 1, 16] * 16)[:50] + [160] * 7 + [0, 16, 1, 145, 81, 17, 2]),
    ("1023", [16] * 30 + [15] + [16] * 33),
    ("partial", [16, 0, 33, 1, 16, 2, 0, 16] * 4 + [16, 18, 3, 0, 5]),
)


def _waves_rows(rows):
    for name, ns in _WAVES:
        assert len(ns) == 64 or name == "partial"
        for lane, n in enumerate(ns):
            if n == 0:
                rows.culled(("behind", "near", "faint")[lane % 3], tag=name)
            else:
                mx, r = strip_rect(n, hint=int(rows.rng.integers(10, 150)))
                rows.add(mx, 8.0, r, tag=name)


def waves():
    """Whole waves designed by their instance total (the sum of _WAVES' rows); plan: waves [(name, first row, rows, designed total)]"""
    cam = synthetic_camera(STRIP_W, STRIP_H)
    rows = _Rows(cam, 12)
    _waves_rows(rows)
    at = np.cumsum([0] + [len(ns) for _, ns in _WAVES])
    return rows.finish(waves=[(name, int(at[i]), len(ns), int(sum(ns))) for i, (name, ns) in enumerate(_WAVES)])


def row_counts(P):
    """the waves mixture tiled to P rows (its 421 rows repeated: the designed waves then fall on every lane offset), M = 0"""
    base = scene("waves")
    n = base["raw"]["xyz"].shape[0]
    idx = torch.from_numpy(np.arange(P) % n)
    raw = {k: (v[idx].contiguous() if torch.is_tensor(v) else v) for k, v in base["raw"].items()}
    return _scene(raw, base["cam"], dict(P=P, period=n))


BORDER_W, BORDER_H = 333, 190
_TIE_X = np.array([0x4357FFFF], np.uint32).view(F32)[0]      # 215.99998: (215.99998 + 25) + 16 = 257.0 exactly (gslic_common.h, get_rect)


def _mean_with_bits(cam, want_mx, my, z):
    """float32 x of a point whose projected means2D.x has exactly the bits of want_mx (searched over the neighbouring floats of the ideal x
    with the float32 restatement of the projection)"""
    p = _xyz(cam, float(want_mx), my, z).astype(F32)
    cand = np.repeat(p, 4001, 0)
    cand[:, 0] = (np.float64(p[0, 0]) + np.arange(-2000, 2001) * float(np.spacing(p[0, 0]))).astype(F32)
    mx, _ = project32(cam, cand)
    hit = np.nonzero(mx.view(np.uint32) == np.asarray(want_mx, F32).view(np.uint32))[0]
    assert hit.size, "no float32 x projects onto the wanted mean"
    return cand[hit[hit.size // 2]].astype(np.float64)


def border():
    """Ragged image 333 x 190 (21 x 12 tiles).  plan: sides {name: [rows]} the isotropic rows around each side and corner, zero [rows] the
    rectangles clamped to nothing, slanted [rows], none_passes [rows] (the cnt == 0 class), tie [rows]."""
    cam = synthetic_camera(BORDER_W, BORDER_H)
    rows = _Rows(cam, 13)
    W, H, r = BORDER_W, BORDER_H, 20
    # outward offsets from the image's edge pixel centre: inside, on the edge, half a radius and nearly a radius outside
    offs = (-5.0, 0.0, 10.0, 19.0)
    sides, zero = {}, []
    axis = {-1: lambda o, S: -o, 0: None, 1: lambda o, S: (S - 1) + o}
    for sy in (-1, 0, 1):
        for sx in (-1, 0, 1):
            if sx == 0 and sy == 0:
                continue
            name = {-1: "top", 0: "", 1: "bottom"}[sy] + {-1: "left", 0: "", 1: "right"}[sx]
            sides[name] = []
            # (a corner: 14 px outside on both axes is 19.8 px from the image — still seen; 18 px is 25.5 — a rectangle of one tile that fails)
            for o in (offs if sx == 0 or sy == 0 else offs[:3] + (14.0, 18.0)):
                mx = axis[sx](o, W) if sx else 0.37 * W
                my = axis[sy](o, H) if sy else 0.41 * H
                sides[name].append(rows.add(mx, my, r, tag=name))
            # clamped to nothing: beyond the padded tile grid by more than the radius (left / top: x1 = 0; right / bottom: x0 = gx)
            gx16, gy16 = 16 * ((W + 15) // 16), 16 * ((H + 15) // 16)
            mx = {-1: -(r + 3.0), 0: 0.37 * W, 1: gx16 + r + 3.0}[sx]
            my = {-1: -(r + 3.0), 0: 0.41 * H, 1: gy16 + r + 3.0}[sy]
            if abs(sx) + abs(sy) == 1:
                zero.append(rows.add(mx, my, r, tag="zero-" + name))
    # thin, rotated: the rectangle holds tiles the exact test rejects (more and fewer than SEQ_TILES tiles; inside and across the border)
    slanted = []
    for k, (mx, my, rad, deg) in enumerate([(100.0, 90.0, 22, 45.0), (200.0, 60.0, 22, -45.0), (160.0, 100.0, 60, 40.0), (60.0, 120.0, 75, -50.0),
                                            (300.0, 30.0, 50, 45.0), (20.0, 170.0, 45, 45.0), (250.0, 150.0, 30, 30.0)]):
        slanted.append(rows.add(mx, my, rad, ratios=(1.0, 0.04, 0.04), quat=_rot_z(deg), tag="slanted"))
    # cnt == 0: faint (cull threshold log(1.2) = 0.18: a tile passes within 0.6 sigma), the mean ten pixels outside the tile grid
    none_passes = []
    gx16, gy16 = 16 * ((W + 15) // 16), 16 * ((H + 15) // 16)
    for mx, my in [(-10.5, 60.0), (150.0, -10.5), (gx16 + 9.5, 100.0), (70.0, gy16 + 9.5), (-9.0, -9.0)]:
        none_passes.append(rows.add(mx, my, r, opacity=1.2 / 255.0, tag="none-passes"))
    # the documented tie and a second split of the same sum (200.99998 + 40)
    tie = []
    for want, rad in ((_TIE_X, 25), (F32(_TIE_X - F32(15.0)), 40)):
        i = rows.add(float(want), 100.0, rad, z=2.0, tag="tie")
        rows.xyz[i] = _mean_with_bits(cam, want, 100.0, 2.0)
        tie.append(i)
    for lane in range(9):
        rows.add(float(rows.rng.uniform(0, W)), float(rows.rng.uniform(0, H)), int(rows.rng.integers(3, 30)), tag="filler")
    return rows.finish(sides=sides, zero=zero, slanted=slanted, none_passes=none_passes, tie=tie, tie_x=[_TIE_X, F32(_TIE_X - F32(15.0))])


def culls():
    """Exact activated values injected into `act` (the raw parameters cannot hold them): plan maps a class name to (row, kept?)."""
    cam = synthetic_camera(160, 96)
    rows = _Rows(cam, 14)
    for lane in range(60):
        rows.add(float(rows.rng.uniform(5, 155)), float(rows.rng.uniform(5, 90)), int(rows.rng.integers(3, 25)), tag="filler")
    plan = {}
    near = F32(0.2)
    for name, z, kept in (("z=0.2", near, False), ("z=next(0.2)", np.nextafter(near, F32(1.0)), True)):
        plan[name] = (rows.add(80.0, 40.0, 12, z=float(z), tag=name), kept)
    one = F32(1.0) / F32(255.0)
    for name, op, kept in (("op=1/255", one, True), ("op=prev(1/255)", np.nextafter(one, F32(0.0)), False)):
        plan[name] = (rows.add(50.0, 50.0, 12, z=3.0, tag=name), kept)
    i = rows.add(30.0, 30.0, 12, z=3.0, tag="behind")
    rows.xyz[i] = np.array([0.3, -0.2, -3.0])
    plan["behind"] = (i, False)
    # 35 px left of the image (the Jacobian's window ends 24 px outside), radius 60: visible, t.x / t.z clamped
    plan["jacobian-clamped"] = (rows.add(-35.0, 48.0, 60, z=4.0, tag="jacobian-clamped"), True)
    for lane in range(9):
        rows.add(float(rows.rng.uniform(5, 155)), float(rows.rng.uniform(5, 90)), int(rows.rng.integers(3, 25)), tag="filler")
    s = rows.finish(**{"rows": plan})
    act = dict(s["act"])
    means, opac = act["means"].clone(), act["opac"].clone()
    means[plan["z=0.2"][0], 2] = float(near)
    means[plan["z=next(0.2)"][0], 2] = float(np.nextafter(near, F32(1.0)))
    opac[plan["op=1/255"][0], 0] = float(one)
    opac[plan["op=prev(1/255)"][0], 0] = float(np.nextafter(one, F32(0.0)))
    act["means"], act["opac"] = means.contiguous(), opac.contiguous()
    return _scene(s["raw"], cam, s["plan"], act=act)


SH_W, SH_H = 64, 48
_sh_base = {}


def sh_visible(P, pattern):
    """the designed visibility of sh_blocks' rows"""
    i = np.arange(P)
    if pattern == "all":
        return np.ones(P, bool)
    if pattern == "none":
        return np.zeros(P, bool)
    if pattern == "alternate":
        return (i % 2) == 0
    return (i % 64) == int(pattern.split("-")[1])


def sh_blocks(D, M, P, pattern):
    """P small Gaussians spread over a 64 x 48 image with large SH coefficients (the same rows, coefficients and means for every D, M and
    pattern: M truncates the coefficient rows, the pattern only makes rows invisible — odd rows by z = 0.1, even rows by opacity 0.001).
    Opacity 0.6, so that a backward reaches every row.  plan: visible [P] as designed."""
    if P not in _sh_base:
        cam = synthetic_camera(SH_W, SH_H)
        rows = _Rows(cam, 100 + P)
        for i in range(P):
            # (means at least six pixels from the principal point's row and column: no component of the view direction near zero)
            side = rows.rng.integers(0, 2, 2)
            rows.add(float(rows.rng.uniform(2, 24) if side[0] else rows.rng.uniform(38, SH_W - 2)),
                     float(rows.rng.uniform(2, 18) if side[1] else rows.rng.uniform(32, SH_H - 2)), int(rows.rng.integers(3, 9)),
                     z=float(rows.rng.uniform(1.0, 6.0)), opacity=0.6, tag="sh")
        _sh_base[P] = rows.finish(D=3, M=15, sh_seed=200 + P)
    base = _sh_base[P]
    vis = sh_visible(P, pattern)
    act = dict(base["act"])
    means, opac = act["means"].clone(), act["opac"].clone()
    hide = torch.from_numpy(~vis)
    odd = torch.from_numpy((np.arange(P) % 2) == 1)
    means[hide & odd, 2] = 0.1
    opac[hide & ~odd, 0] = 0.001
    act.update(means=means.contiguous(), opac=opac.contiguous(), shs=base["act"]["shs"][:, :M].contiguous(), D=int(D))
    raw = dict(base["raw"], features_rest=base["raw"]["features_rest"][:, :M].contiguous(), sh_degree=int(D))
    # (a single-r pattern in a scene none of whose blocks has a row r designs nothing: reported, and the scene still runs — all invisible)
    dropped = [(P, pattern)] if pattern.startswith("single-") and not vis.any() else []
    return _scene(raw, base["cam"], dict(visible=vis, D=D, M=M, pattern=pattern, dropped=dropped), act=act)


SCENES = {"strip": strip, "waves": waves, "border": border, "culls": culls}
_built = {}


def scene(name):
    """SCENES[name](), built once and never modified"""
    if name not in _built:
        _built[name] = SCENES[name]()
    return _built[name]
