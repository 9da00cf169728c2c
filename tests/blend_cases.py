"""Scenes whose blend DECISIONS are designed, and a plain float64 restatement of what the blend kernels must compute on them.
No GPU, no library: numpy, make_scene and the scene generator, as tests/tile_lists.py.

The blend kernels (csrc/render_fwd_body.inc, csrc/render_bwd_scan.hip, the pipeline of csrc/render.hip) decompose a tile's work by buckets
of GS_BUCKET = 64 list entries, 8x8 pixel quadrants, 8x4 half quadrants, compacted entry groups of 16, pixel chunks of 4 and two 32-bit
decision mask words.  Every case here owns one tile and puts a chosen (entry, pixel) decision pattern at one of those edges; `decisions`
restates the reference's sequential decisions per pixel, `halves` derives the strict backward's work lists from them (ne, npx, compacted
entries), `coverage` names the structural cells a set of decisions reaches and REQUIRED lists the cells that must be reached and by which
case.  `backward` restates the strict backward in the kernel's own decomposition, so that single structural mistakes (MUTANTS) can be
made in it; `judge` is the comparator of the GPU suites.

The construction.  Identity pose, depth key = the float32 bits of z.  A Gaussian is a disc facing the camera (scales (sx, sy, 1e-3 min),
rotation about the optical axis), so its 2D covariance is R diag(sx^2, sy^2) R^T + 0.3 I in pixels whatever its place in the image.  Three
kinds of entry:
  dot    sigma 0.5, opacity 0.006, 0.1 px off a pixel centre: alpha = 1.5 / 255 on that pixel, 0.73 / 255 on its nearest neighbour — blended
         by exactly one pixel;
  faint  opacity 0.0045 on a pixel CORNER: 0.73 / 255 at the four nearest centres — in the list (the mean lies inside the tile), blended nowhere;
  blob   anything larger; its position is nudged (seeded) until every pair of its tile keeps the cut margins.
Case tiles lie on even tile columns and rows (the ragged scene: also on the last column and row), so an empty tile separates any two."""
import math

import numpy as np
import torch

from conftest import make_scene
import tile_lists as tl

BUCKET, GROUP, CHUNK = 64, 16, 4          # GS_BUCKET, the compacted entry groups, the pixel rows of a wave (csrc/render_bwd_scan.hip)
ALPHA_MIN, T_MIN, ALPHA_MAX = 1.0 / 255.0, 1e-4, 0.99
MARGIN = 1e-3                             # cut_margins; the builder nudges with twice that
DOT_OP, FAINT_OP = 0.006, 0.0045
FACTOR = 5                                # judge(): twice the largest measured ratio (2.219), rounded up — profiles/blend_cases_factors.txt

_I = np.arange(256)
LX = ((_I >> 6) & 1) * 8 + (_I & 7)       # tile_pix_x / tile_pix_y of gslic_common.h: element q * 64 + lane of the tile-major arrays
LY = (_I >> 7) * 8 + ((_I >> 3) & 7)


def pix_index(lx, ly):
    return ((ly >> 3) * 2 + (lx >> 3)) * 64 + (ly & 7) * 8 + (lx & 7)


# ------------------------------------------------------------------------------------------------------------------ entries
def dot(lx, ly):
    return dict(x=lx + 0.1, y=ly + 0.07, sx=0.5, sy=0.5, th=0.0, op=DOT_OP, jit=False)


def faint(lx, ly):
    return dict(x=lx + 0.5, y=ly + 0.5, sx=0.5, sy=0.5, th=0.0, op=FAINT_OP, jit=False)


def blob(x, y, s, op, sy=None, th=0.0):
    return dict(x=x, y=y, sx=s, sy=s if sy is None else sy, th=th, op=op, jit=True)


def opaque(lx, ly):
    """sigma 0.5, opacity 0.99, on pixel (lx, ly): alpha 0.977 there — two of them leave T = 5.4e-4, the third stops the pixel"""
    return dict(x=lx + 0.1, y=ly + 0.07, sx=0.5, sy=0.5, th=0.0, op=0.99, jit=False)


def half_pixels(q, h):
    return [(8 * (q & 1) + x, 8 * (q >> 1) + 4 * h + y) for y in range(4) for x in range(8)]


def dots_on(pixels, count):
    return [dot(*pixels[i % len(pixels)]) for i in range(count)]


def _case_ne_small():
    e = dots_on(half_pixels(0, 0)[9:10], 1) + dots_on(half_pixels(1, 0)[9:12], 15) + dots_on(half_pixels(2, 0)[9:13], 16)
    return e + dots_on(half_pixels(3, 0)[9:14], 17)


def _case_ne_31_32():
    return dots_on(half_pixels(0, 0)[:31], 31) + dots_on(half_pixels(2, 0), 32) + dots_on(half_pixels(3, 1)[9:10], 1)


def _case_ne_33():
    return dots_on(half_pixels(0, 0)[8:16], 33)


def _case_ne_47_48_49():
    px = half_pixels(0, 0)[9:14]
    f = [faint(12, 12)]
    return dots_on(px, 47) + f * 17 + dots_on(px, 48) + f * 16 + dots_on(px, 49)


def _case_ne_63():
    return dots_on(half_pixels(1, 1)[9:15], 63)


def _case_ne_64():
    return [blob(3.3 + 0.9 * math.cos(0.7 * k), 1.6 + 0.5 * math.sin(1.1 * k), 1.6 + 0.02 * (k % 9), 0.03 + 0.002 * (k % 17), sy=1.2, th=0.3 * k)
            for k in range(64)]


def _case_seam():
    return [faint(12, 3)] * 31 + [blob(3.1, 3.07, 0.5, 0.5), blob(5.1, 3.07, 0.5, 0.5)] + dots_on(half_pixels(3, 0)[9:14], 31)


def _case_unblended():
    e = dots_on(half_pixels(0, 0)[8:16], 40)
    for k in (0, 31, 32, 39):
        e[k] = faint(12, 12)
    return e


def _case_handoff():
    p, p1, q, q1 = (2, 1), (5, 1), (10, 9), (13, 9)
    b0 = dots_on([p], 16) + dots_on([p1], 16) + dots_on([p], 16) + [faint(12, 3)] * 16
    b1 = dots_on([q1], 15) + dots_on([q], 2) + dots_on([q1], 4) + [faint(12, 3)] * 43
    return b0 + b1


def _case_n200():
    others = half_pixels(1, 0)[8:16]
    e = dots_on(others, 200)
    for k in (5, 63):
        e[k] = dot(1, 1)          # pixel (1, 1): last contributor 64 = bstart of bucket 1
    for k in (9, 64):
        e[k] = dot(3, 1)          # pixel (3, 1): last contributor 65 = bstart + 1
    for k in range(130, 200, 3):
        e[k] = dot(4, 12)
    return e


def _case_clamp_reach():
    return [blob(11.05, 11.03, 1.0, 0.999), blob(7.6, 3.1, 0.5, 0.5), blob(3.1, 7.6, 0.5, 0.5), blob(11.4, 11.6, 2.0, 0.6, sy=1.4, th=0.5),
            faint(2, 12), blob(10.2, 12.3, 1.5, 0.4)]


def _case_maxc64():
    return dots_on(half_pixels(0, 0)[8:15], 64) + [faint(0, 1)]      # (seven pixels: entries 0 and 63 fall on pixel (0, 1), and entry 64 lies beside it)


def _case_maxc65():
    return dots_on(half_pixels(0, 0)[8:16], 65) + [faint(12, 12)] * 62


def _case_n1():
    return [blob(7.3, 8.2, 2.5, 0.7, sy=1.5, th=0.6)]


def _case_terminate():
    grid = (1.0, 5.35, 9.65, 14.0)
    layer = [blob(x, y, 3.0, 0.99) for y in grid for x in grid]
    e = layer * 3 + [blob(x, y, 3.0, 0.99) for y in (0.5, 14.5) for x in (0.5, 14.5)] * 2        # (the corners last: 56 entries stop every pixel)
    rng = np.random.default_rng(3)
    return e + [blob(float(rng.uniform(2, 13)), float(rng.uniform(2, 13)), 1.0, 0.5) for _ in range(129 - len(e))]


def _case_term_slots():
    e = dots_on([(6, 1)], 14) + [opaque(1, 1)] * 3 + dots_on([(14, 9)], 15) + [opaque(9, 9)] * 3 + dots_on([(14, 9)], 5)
    return e


def _ragged(ox, oy, visible):
    """a Gaussian with its mean at (ox, oy) — inside the tile, outside the image — reaching the visible pixels, blobs and 24 dots on them"""
    (ax, ay), (bx, by), (cx, cy) = visible
    return ([blob(ox, oy, 2.6, 0.7), blob(ax + 0.3, ay + 0.4, 1.5, 0.5, sy=0.9, th=0.8)] + dots_on(visible, 24)
            + [blob(bx - 0.2, by + 0.3, 2.2, 0.35, sy=1.1, th=-0.4), blob(ox - 1.0, oy - 1.0, 2.0, 0.3)])


def _case_ragged_x():
    return _ragged(8.2, 5.1, [(1, 1), (4, 2), (2, 9)])


def _case_ragged_y():
    return _ragged(7.3, 6.2, [(1, 1), (9, 2), (12, 3)])


def _case_ragged_corner():
    return _ragged(7.2, 5.3, [(1, 1), (4, 2), (2, 3)])


def _case_filler():
    """owns no cell: a free tile of the ragged scene given two buckets of dots — the knob on that scene's bucket count, which must not be a
    multiple of 128 (tests/test_blend_cases_cpu.py asserts it)"""
    return dots_on(half_pixels(0, 0)[:3], 70)


CASES = {
    "ne-small": _case_ne_small, "ne-31-32": _case_ne_31_32, "ne-33": _case_ne_33, "ne-47-48-49": _case_ne_47_48_49, "ne-63": _case_ne_63,
    "ne-64": _case_ne_64, "seam": _case_seam, "unblended": _case_unblended, "handoff": _case_handoff, "n200": _case_n200,
    "clamp-reach": _case_clamp_reach, "maxc64": _case_maxc64, "maxc65": _case_maxc65, "n1": _case_n1, "terminate": _case_terminate,
    "term-slots": _case_term_slots, "ragged-x": _case_ragged_x, "ragged-y": _case_ragged_y, "ragged-corner": _case_ragged_corner,
    "filler": _case_filler,
}
INTERIOR = tuple(k for k in CASES if not k.startswith("ragged") and k != "filler")      # the cases of the exact scene
# scene -> (W, H, {case: (tx, ty)})
SCENES = {
    "exact": (160, 112, {k: (2 * (i % 5), 2 * (i // 5)) for i, k in enumerate(INTERIOR)}),
    "ragged": (150, 100, {"ragged-x": (9, 2), "ragged-y": (3, 6), "ragged-corner": (9, 6), "handoff": (0, 0), "seam": (2, 0), "ne-47-48-49": (4, 0),
                          "terminate": (6, 0), "term-slots": (0, 2), "n200": (2, 2), "ne-64": (4, 2), "clamp-reach": (6, 2), "ne-small": (0, 4),
                          "maxc64": (2, 4), "unblended": (4, 4), "ne-31-32": (6, 4), "maxc65": (9, 0), "ne-33": (9, 4), "n1": (1, 6),
                          "ne-63": (5, 6), "filler": (7, 6)}),
}


# ------------------------------------------------------------------------------------------------------------------ decisions
def conic_of(e):
    """(A, B, C, opacity) of a designed entry: the inverse of R diag(sx^2, sy^2) R^T + 0.3 I (float64)"""
    c, s = math.cos(e["th"]), math.sin(e["th"])
    a, b = e["sx"] ** 2, e["sy"] ** 2
    xx, xy, yy = c * c * a + s * s * b + 0.3, c * s * (a - b), s * s * a + c * c * b + 0.3
    det = xx * yy - xy * xy
    return (yy / det, -xy / det, xx / det, e["op"])


def tile_decisions(m2, co, tx0, ty0, W, H, edge=True):
    """The reference's sequential blend of one tile's list (forward.cu:424-445) for its 256 pixels, in float64.  m2 [n, 2] means in pixels,
    co [n, 4] conic and opacity, both in list order.  Pixels are indexed as the kernels' tile-major arrays are (LX, LY).  edge=False drops
    the image-edge test (a mutant)."""
    m2, co = np.asarray(m2, np.float64).reshape(-1, 2), np.asarray(co, np.float64).reshape(-1, 4)
    n = m2.shape[0]
    px, py = (tx0 + LX).astype(np.float64), (ty0 + LY).astype(np.float64)
    inimg = ((tx0 + LX < W) & (ty0 + LY < H)) if edge else np.ones(256, bool)
    dx, dy = m2[:, 0:1] - px[None, :], m2[:, 1:2] - py[None, :]
    power = -0.5 * (co[:, 0:1] * dx * dx + co[:, 2:3] * dy * dy) - co[:, 1:2] * dx * dy
    G = np.exp(np.minimum(power, 0.0))
    araw = co[:, 3:4] * G
    alpha = np.minimum(ALPHA_MAX, araw)
    cand_static = ~(power > 0.0) & ~(alpha < ALPHA_MIN)
    T = np.ones(256)
    alive = inimg.copy()
    last = np.zeros(256, np.int64)
    stop_k = np.full(256, -1, np.int64)
    blended = np.zeros((n, 256), bool)
    alive_before = np.zeros((n, 256), bool)
    Tb = np.ones((n, 256))
    for k in range(n):
        Tb[k], alive_before[k] = T, alive
        cand = cand_static[k] & alive
        test_T = T * (1.0 - alpha[k])
        stop = cand & (test_T < T_MIN)
        b = cand & ~stop
        blended[k] = b
        T = np.where(b, test_T, T)
        last = np.where(b, k + 1, last)
        stop_k = np.where(stop, k, stop_k)
        alive = alive & ~stop
    return dict(n=n, tx0=tx0, ty0=ty0, inimg=inimg, dx=dx, dy=dy, power=power, G=G, araw=araw, alpha=alpha, blended=blended, Tb=Tb,
                alive_before=alive_before, n_contrib=last, final_T=np.where(inimg, T, 0.0), stop_k=stop_k,
                max_contrib=int(last.max()) if n else 0)


def blend_image(d, values):
    """sum T alpha v over a pixel's blended entries (values [n, C] in list order): the colour, or with v = z the depth — [256, C]"""
    w = np.where(d["blended"], d["Tb"] * d["alpha"], 0.0)
    return w.T @ np.asarray(values, np.float64).reshape(d["n"], -1)


def halves(d):
    """The strict backward's work lists: for every LIVE bucket (bstart < max_contrib), quadrant q and half h: dict(b, q, h, pix = the active
    pixels' indices in lane order, npx, entries = the compacted list (bucket-local, ascending), ne), and per live bucket the valid entries
    no pixel of the tile blended."""
    out, unblended = [], {}
    for b in range((d["n"] + BUCKET - 1) // BUCKET):
        bs, be = b * BUCKET, min(d["n"], (b + 1) * BUCKET)
        if bs >= d["max_contrib"]:
            continue
        blk = d["blended"][bs:be]
        unblended[b] = [int(k) for k in np.flatnonzero(~blk.any(axis=1))]
        for q in range(4):
            for h in range(2):
                idx = q * 64 + h * 32 + np.arange(32)
                act = d["inimg"][idx] & (d["n_contrib"][idx] > bs) & blk[:, idx].any(axis=0)
                pix = idx[act]
                ents = np.flatnonzero(blk[:, pix].any(axis=1))
                out.append(dict(b=b, q=q, h=h, pix=pix, npx=int(pix.size), entries=ents, ne=int(ents.size)))
    return out, unblended


def decisions(sc, camd, pre, bins, plan):
    """{case name: tile_decisions of its tile + halves / unblended / reach} from the oracle's preprocess output and lists"""
    out = {}
    for c in plan["cases"]:
        out[c["name"]] = _decide(pre, bins, plan, c["tile"])
    return out


def _decide(pre, bins, plan, t, edge=True):
    r0, r1 = (int(v) for v in bins["ranges"][t])
    g = bins["point_list"][r0:r1].astype(np.int64)
    d = tile_decisions(pre["means2D"][g], pre["conic_opacity"][g], 16 * (t % plan["gx"]), 16 * (t // plan["gx"]), plan["W"], plan["H"], edge)
    d["rows"], d["tile"] = g, t
    d["halves"], d["unblended"] = halves(d)
    reach = ~(d["power"] > 0) & ~(d["alpha"] < ALPHA_MIN)              # (entry, pixel) pairs the entry can reach at all, whatever T
    d["reach_q"] = np.stack([reach[:, 64 * q:64 * q + 64].any(axis=1) for q in range(4)], 1) if d["n"] else np.zeros((0, 4), bool)
    return d


def cut_margins(dec, margin=MARGIN):
    """Asserts that every (pixel, entry) pair of every case tile that TAKES a decision stays `margin` relative away from the blend's hard cuts.
    power < -1e-6 is asked of every pair without the rectangle exemption (stricter: no mean sits on a pixel centre).  The alpha cut is asked of
    the pairs whose pixel is still blending when the entry comes (in the image, not stopped): a finished pixel decides nothing, whatever its
    alpha.  The T cut is asked of those of them with alpha >= 1/255: only they reach the test T (1 - alpha) < 1e-4.  As long as the earlier
    pairs of a pixel keep their margins, two float32 blends agree on which pairs these are."""
    for name, d in dec.items():
        if d["n"] == 0:
            continue
        a = d["alive_before"]
        assert (d["power"] < -1e-6).all(), (name, "power", float(d["power"].max()))
        m = np.abs(255.0 * d["araw"] - 1.0)[a]
        assert m.size == 0 or m.min() > margin, (name, "alpha cut", float(m.min()))
        cand = a & ~(d["alpha"] < ALPHA_MIN)
        tt = np.abs(d["Tb"] * (1.0 - d["alpha"]) / T_MIN - 1.0)[cand]
        assert tt.size == 0 or tt.min() > margin, (name, "T cut", float(tt.min()))


# ------------------------------------------------------------------------------------------------------------------ coverage
def cells_of(d):
    """the structural cells one tile's decisions reach"""
    c = set()
    n, H_, bl = d["n"], d["halves"], d["blended"]
    c.add(f"n={n}")
    c.add(f"maxc={d['max_contrib']}")
    if d["max_contrib"] == BUCKET and n > BUCKET:
        c.add("dead-bucket-1")
    if d["max_contrib"] == BUCKET + 1:
        c.add("bucket-1-live-through-one-entry")
    by_bq = {}
    for x in H_:
        by_bq.setdefault((x["b"], x["q"]), {})[x["h"]] = x
        if x["npx"]:
            c.add(f"ne={x['ne']}")
            c.add(f"npx={x['npx']}")
            ents, pix = x["entries"], x["pix"]
            m = bl[x["b"] * BUCKET + ents][:, pix]                     # [ne, npx] in compacted order
            grp = np.array([m[g * GROUP:(g + 1) * GROUP].any(axis=0) for g in range((x["ne"] + GROUP - 1) // GROUP)])   # [NG, npx]
            for p in range(pix.size):
                gs = np.flatnonzero(grp[:, p])
                run = best = 1
                for a_, b_ in zip(gs[:-1], gs[1:]):
                    run = run + 1 if b_ == a_ + 1 else 1
                    best = max(best, run)
                if best >= 3:
                    c.add("handoff-3")
                if best >= 4:
                    c.add("handoff-4")
                if gs.size >= 2 and (np.diff(gs) > 1).any():
                    c.add("handoff-gap")
                ks = np.flatnonzero(m[:, p])
                if ks.size == 2 and ks[0] % GROUP == GROUP - 1 and ks[1] == ks[0] + 1:
                    c.add("handoff-15-16")
                gp = int(pix[p])
                if d["stop_k"][gp] >= 0 and ks.size and d["n_contrib"][gp] > x["b"] * BUCKET and d["n_contrib"][gp] <= (x["b"] + 1) * BUCKET:
                    if ks[-1] % GROUP == GROUP - 1:
                        c.add("term-slot15")
                    if ks[-1] % GROUP == 0 and ks[-1] >= GROUP:
                        c.add("term-slot16")
    for (b, q), hh in by_bq.items():
        if (hh[0]["npx"] == 0) != (hh[1]["npx"] == 0):
            c.add("half-empty-beside-active")
    for b in {x["b"] for x in H_}:
        act = [any(by_bq[(b, q)][h]["npx"] for h in (0, 1)) for q in range(4)]
        if any(act[i] and not act[i + 1] and any(act[i + 2:]) for i in range(2)):
            c.add("quadrant-gap")
        nes = [max(by_bq[(b, q)][h]["ne"] for h in (0, 1)) for q in range(4)]
        if all(act) and len(set(nes)) == 4:
            c.add("four-ne")
        bs = b * BUCKET
        nv = min(n, bs + BUCKET) - bs
        if nv > 32:
            both = bl[bs + 31] & bl[bs + 32]
            if both.any():
                c.add("seam-both")
            if (bl[bs + 31] & ~bl[bs + 32]).any():
                c.add("seam-31")
            if (~bl[bs + 31] & bl[bs + 32]).any():
                c.add("seam-32")
        un = d["unblended"][b]
        for k, nm in ((0, "0"), (31, "31"), (32, "32"), (nv - 1, "last")):
            if k in un:
                c.add("unblended-" + nm)
        if not un and nv == BUCKET:
            c.add("all-blended")
        nc = d["n_contrib"][d["inimg"]]
        if b >= 1 and (nc > bs).any():
            if (nc == bs).any():
                c.add("nc=bstart")
            if (nc == bs + 1).any():
                c.add("nc=bstart+1")
    if (d["araw"][bl] >= ALPHA_MAX).any():
        c.add("clamp")
    if n and (d["araw"].max(axis=1) < ALPHA_MIN).any():
        c.add("never")
    if n > 2 * BUCKET and n <= 3 * BUCKET and d["max_contrib"] <= BUCKET and (d["stop_k"][d["inimg"]] >= 0).all() and (d["stop_k"] < BUCKET).all():
        c.add("all-terminate-in-bucket-0-of-3")
    rq = d["reach_q"]
    for k in range(n):
        qs = tuple(np.flatnonzero(rq[k]))
        if len(qs) == 1:
            c.add(f"reach-q{qs[0]}")
        if qs in ((0, 1), (2, 3)):
            c.add("reach-one-wave")
        if len(qs) == 2 and (qs[0] < 2) != (qs[1] < 2):
            c.add("reach-both-waves")
    cut_x, cut_y = (~d["inimg"] & (LY == 0)).any(), (~d["inimg"] & (LX == 0)).any()
    if cut_x or cut_y:
        kind = "corner" if cut_x and cut_y else ("x" if cut_x else "y")
        c.add("ragged-" + kind)
        mx, my = d["dx"][:, 0] + d["tx0"] + LX[0], d["dy"][:, 0] + d["ty0"] + LY[0]
        w, h = d["tx0"] + LX[d["inimg"]].max(), d["ty0"] + LY[d["inimg"]].max()
        out = ((mx > w + 0.5) | (my > h + 0.5)) & bl.any(axis=1)
        if out.any():
            c.add(f"ragged-{kind}-mean-outside")
    return c


def coverage(dec):
    """{cell: set of the cases that reach it}"""
    out = {}
    for name, d in dec.items():
        for cell in cells_of(d):
            out.setdefault(cell, set()).add(name)
    return out


# cell -> the case that must reach it
REQUIRED = {
    "ne=1": "ne-small", "ne=15": "ne-small", "ne=16": "ne-small", "ne=17": "ne-small", "ne=31": "ne-31-32", "ne=32": "ne-31-32", "ne=33": "ne-33",
    "ne=47": "ne-47-48-49", "ne=48": "ne-47-48-49", "ne=49": "ne-47-48-49", "ne=63": "ne-63", "ne=64": "ne-64",
    "npx=1": "ne-small", "npx=3": "ne-small", "npx=4": "ne-small", "npx=5": "ne-small", "npx=31": "ne-31-32", "npx=32": "ne-31-32",
    "half-empty-beside-active": "ne-small", "quadrant-gap": "ne-31-32", "four-ne": "ne-small",
    "seam-both": "seam", "seam-31": "seam", "seam-32": "seam",
    "handoff-3": "ne-47-48-49", "handoff-4": "ne-64", "handoff-gap": "handoff", "handoff-15-16": "handoff",
    "clamp": "clamp-reach", "never": "unblended",
    "n=1": "n1", "n=63": "ne-63", "n=64": "ne-64", "n=65": "maxc64", "n=127": "maxc65", "n=128": "handoff", "n=129": "terminate", "n=200": "n200",
    "dead-bucket-1": "maxc64", "bucket-1-live-through-one-entry": "maxc65", "nc=bstart": "n200", "nc=bstart+1": "n200",
    "all-terminate-in-bucket-0-of-3": "terminate", "term-slot15": "term-slots", "term-slot16": "term-slots",
    "unblended-0": "unblended", "unblended-31": "unblended", "unblended-32": "unblended", "unblended-last": "unblended", "all-blended": "ne-64",
    "reach-q0": "ne-small", "reach-q1": "ne-small", "reach-q2": "ne-small", "reach-q3": "ne-small", "reach-one-wave": "clamp-reach",
    "reach-both-waves": "clamp-reach",
    "ragged-x": "ragged-x", "ragged-y": "ragged-y", "ragged-corner": "ragged-corner", "ragged-x-mean-outside": "ragged-x",
    "ragged-y-mean-outside": "ragged-y", "ragged-corner-mean-outside": "ragged-corner",
}


# ------------------------------------------------------------------------------------------------------------------ the scenes
def _design(name, W, H, tx, ty, rng):
    """the entries of one case, its blobs nudged until the analytic decisions keep twice the cut margins"""
    base = CASES[name]()
    for attempt in range(400):
        nudge = {}                                                          # (entries designed equal stay equal)
        for e in base:
            key = (e["x"], e["y"], e["sx"], e["op"])
            if key not in nudge:
                nudge[key] = rng.normal(0, 0.04, 2) if e["jit"] and attempt else np.zeros(2)
        ents = [dict(e, x=e["x"] + nudge[(e["x"], e["y"], e["sx"], e["op"])][0], y=e["y"] + nudge[(e["x"], e["y"], e["sx"], e["op"])][1]) for e in base]
        m2 = np.array([[16 * tx + e["x"], 16 * ty + e["y"]] for e in ents])
        co = np.array([conic_of(e) for e in ents])
        try:
            cut_margins({name: tile_decisions(m2, co, 16 * tx, 16 * ty, W, H)}, 2 * MARGIN)
            return ents
        except AssertionError:
            continue
    raise AssertionError(f"no placement of {name} keeps the cut margins")


_built = {}


def build(which):
    """(raw, sc, camd, cam, plan) of SCENES[which]; plan = dict(W, H, gx, T, tile [P], key [P] depth keys, case [P] index into cases,
    cases [dict(name, tile, n)]).  Built once per process; callers do not modify it."""
    if which in _built:
        return _built[which]
    W, H, where = SCENES[which]
    rng = np.random.default_rng(7 + list(SCENES).index(which))
    gx, gy = (W + 15) // 16, (H + 15) // 16
    cases, ents, tile_s, case_s, z_s = [], [], [], [], []
    for ci, (name, (tx, ty)) in enumerate(where.items()):
        e = _design(name, W, H, tx, ty, rng)
        cases.append(dict(name=name, tile=ty * gx + tx, n=len(e)))
        ents += [dict(v, x=16 * tx + v["x"], y=16 * ty + v["y"]) for v in e]
        tile_s += [ty * gx + tx] * len(e)
        case_s += [ci] * len(e)
        z_s += [2.0 + 0.03125 * k + 0.001 * ci for k in range(len(e))]      # list order = depth order
    P = len(ents)
    rows = rng.permutation(P)                                               # a case's Gaussians are not contiguous rows
    raw, _, camd, cam = make_scene("random", P, W, H, 3, 21)
    z = np.empty(P, np.float32)
    z[rows] = np.array(z_s, np.float32)
    tile, case = np.empty(P, np.int64), np.empty(P, np.int64)
    tile[rows], case[rows] = tile_s, case_s
    f = lambda k: np.array([e[k] for e in ents], np.float64)
    inv = np.empty(P, np.int64)
    inv[rows] = np.arange(P)
    g = lambda k: f(k)[inv]
    zz = z.astype(np.float64)
    fx, fy = float(cam.fx), float(cam.fy)
    xyz = np.stack([(g("x") + 0.5 - float(cam.cx)) / fx * zz, (g("y") + 0.5 - float(cam.cy)) / fy * zz, zz], 1).astype(np.float32)
    assert np.array_equal(xyz[:, 2], z)
    sx, sy = g("sx") * zz / fx, g("sy") * zz / fy
    raw["xyz"] = torch.from_numpy(xyz).contiguous()
    raw["scaling"] = torch.from_numpy(np.log(np.stack([sx, sy, 1e-3 * np.minimum(sx, sy)], 1)).astype(np.float32)).contiguous()
    th = g("th")
    raw["rotation"] = torch.from_numpy(np.stack([np.cos(th / 2), 0 * th, 0 * th, np.sin(th / 2)], 1).astype(np.float32)).contiguous()
    op = g("op")
    raw["opacity"] = torch.from_numpy(np.log(op / (1.0 - op)).astype(np.float32).reshape(P, 1)).contiguous()
    from gaussian_lic_amd.synthetic import activate, to_numpy
    plan = dict(W=W, H=H, gx=gx, T=gx * gy, tile=tile, key=z.view(np.uint32).copy(), case=case, cases=cases)
    _built[which] = (raw, to_numpy(activate(raw)), camd, cam, plan)
    return _built[which]


def expected_case_lists(plan):
    """{case name: its tile's list} by the plain statement of tile_lists.expected_lists: ascending (depth bits, row)"""
    e = tl.expected_lists(plan["tile"], plan["key"], plan["T"])
    return {c["name"]: e["point_list"][int(e["ranges"][c["tile"], 0]):int(e["ranges"][c["tile"], 1])] for c in plan["cases"]}


def isolation(sc_pre, plan):
    """Largest alpha (float64) any Gaussian reaches on a pixel of ANOTHER case's tile, in units of 1 / 255."""
    m2, co = np.asarray(sc_pre["means2D"], np.float64), np.asarray(sc_pre["conic_opacity"], np.float64)
    worst = 0.0
    for ci, c in enumerate(plan["cases"]):
        t = c["tile"]
        px, py = 16.0 * (t % plan["gx"]) + LX, 16.0 * (t // plan["gx"]) + LY
        o = np.flatnonzero(plan["case"] != ci)
        dx, dy = m2[o, 0:1] - px[None], m2[o, 1:2] - py[None]
        power = -0.5 * (co[o, 0:1] * dx * dx + co[o, 2:3] * dy * dy) - co[o, 1:2] * dx * dy
        worst = max(worst, float((co[o, 3:4] * np.exp(np.minimum(power, 0.0))).max()) * 255.0)
    return worst


def pixel_grads(W, H):
    """(dL_dpix [3, H, W], dL_ddepth [H, W]) float32, NON-ZERO on every pixel: a wrongly included pixel shows"""
    g = np.random.default_rng(5)
    s = lambda *shape: (g.uniform(0.25, 1.0, shape) * g.choice([-1.0, 1.0], shape)).astype(np.float32)
    return s(3, H, W), s(H, W)


# ------------------------------------------------------------------------------------------------------------------ the backward, restated
MUTANTS = {   # name -> the case that owns the edge
    "no-handoff": "handoff",            # the state {T, A} is not handed from the 16th to the 17th compacted entry
    "bit32-low-word": "seam",           # the decision of entry 32 read from the low mask word (bit 32 & 31 = 0 of it)
    "pad-last-pixel": "ne-small",       # the last chunk's padding rows read pixel npx - 1 instead of the all-zero record
    "dead-gt": "maxc64",                # liveness off by one (> for >=): the bucket with bstart == max_contrib is worked on, a pixel with
                                        # n_contrib == bstart is active in it; its masks and checkpoints are stale (taken: the bucket's before)
    "edge-active": "ragged-x",          # out-of-image pixels of a cut tile blend and are active (their dL/dpixel: the row-major address)
}


def backward(pre, bins, plan, dL_dpix, tiles=None, mutant=None):
    """The strict blend backward (csrc/render_bwd_scan.hip) restated in float64 numpy in the kernel's own decomposition — live buckets,
    quadrants, halves, compacted entries in groups of GROUP, pixel records in chunks of CHUNK padded with the half's all-zero record, the
    decision taken from the low or the high mask word — over the given tiles (default: every tile with a list).  Returns the reference's
    four blend gradients dict(dL_dmean2D [P, 2], dL_dconic [P, 3], dL_dopacity [P], dL_dcolor [P, 3])."""
    W, H = plan["W"], plan["H"]
    P = pre["means2D"].shape[0]
    out = dict(dL_dmean2D=np.zeros((P, 2)), dL_dconic=np.zeros((P, 3)), dL_dopacity=np.zeros(P), dL_dcolor=np.zeros((P, 3)))
    gflat = np.asarray(dL_dpix, np.float64).reshape(3, -1)
    rng = bins["ranges"].astype(np.int64)
    for t in (np.flatnonzero(rng[:, 1] > rng[:, 0]) if tiles is None else tiles):
        d = _decide(pre, bins, plan, int(t), edge=mutant != "edge-active")
        rows, n = d["rows"], d["n"]
        co = np.asarray(pre["conic_opacity"], np.float64)[rows]
        rgb = np.asarray(pre["rgb"], np.float64)[rows]
        pid = np.clip((d["ty0"] + LY) * W + d["tx0"] + LX, 0, W * H - 1)
        g = np.where(d["inimg"][None], gflat[:, pid], 0.0)                   # [3, 256]
        w_fwd = np.where(d["blended"], d["Tb"] * d["alpha"], 0.0)
        final_C = w_fwd.T @ rgb                                              # [256, 3]
        acc = np.zeros((n, 9))
        nb = (n + BUCKET - 1) // BUCKET
        for b in range(nb):
            bs, be = b * BUCKET, min(n, (b + 1) * BUCKET)
            live = bs <= d["max_contrib"] if mutant == "dead-gt" else bs < d["max_contrib"]
            if not live:
                continue
            src = b - 1 if (mutant == "dead-gt" and bs == d["max_contrib"] and b > 0) else b     # stale masks / checkpoints
            ss, se = src * BUCKET, min(n, (src + 1) * BUCKET)
            mask = np.zeros((BUCKET, 256), bool)
            mask[:se - ss] = d["blended"][ss:se]
            ck_T = d["Tb"][ss]
            ck_C = w_fwd[:ss].T @ rgb[:ss]
            for q in range(4):
                for h in range(2):
                    idx = q * 64 + h * 32 + np.arange(32)
                    nc_ok = d["n_contrib"][idx] >= bs if mutant == "dead-gt" else d["n_contrib"][idx] > bs
                    act = d["inimg"][idx] & nc_ok & mask[:, idx].any(axis=0)
                    pix = idx[act]
                    npx = pix.size
                    if npx == 0:
                        continue
                    ents = np.flatnonzero(mask[:, pix].any(axis=1))
                    ents = ents[ents < be - bs]
                    # pixel records, padded to whole chunks: {T, A} {g} {mask}
                    npad = (npx + CHUNK - 1) // CHUNK * CHUNK
                    rec = np.concatenate([pix, np.full(npad - npx, pix[-1])])
                    real = np.arange(npad) < npx
                    keep = real | (mutant == "pad-last-pixel")
                    Tin = np.where(keep, ck_T[rec], 0.0)
                    gg = np.where(keep[None], g[:, rec], 0.0)
                    Ain = np.where(keep, ((ck_C[rec] - final_C[rec]) * gg.T).sum(axis=1), 0.0)
                    T, A = Tin.copy(), Ain.copy()
                    for k, e in enumerate(ents):
                        if k % GROUP == 0 and k and mutant == "no-handoff":
                            T, A = Tin.copy(), Ain.copy()
                        bit = 0 if (mutant == "bit32-low-word" and e == 32) else e
                        m = np.where(keep, mask[bit, rec], False)
                        j = bs + e
                        ah = np.where(m, d["araw"][j, rec], 0.0)
                        alpha = np.minimum(ah, ALPHA_MAX)
                        Ta = T * alpha
                        cgd = rgb[j] @ gg
                        Ap = A + Ta * cgd
                        wgt = ah * (T * cgd + Ap / (1.0 - alpha))
                        dx, dy = d["dx"][j, rec], d["dy"][j, rec]
                        acc[j] += [(wgt * dx).sum(), (wgt * dy).sum(), (wgt * dx * dx).sum(), (wgt * dx * dy).sum(), (wgt * dy * dy).sum(), wgt.sum(),
                                   (Ta * gg[0]).sum(), (Ta * gg[1]).sum(), (Ta * gg[2]).sum()]
                        T, A = T * (1.0 - alpha), Ap
        A_, B_, C_, op = co[:, 0], co[:, 1], co[:, 2], co[:, 3]
        np.add.at(out["dL_dmean2D"], rows, np.stack([0.5 * W * (-A_ * acc[:, 0] - B_ * acc[:, 1]), 0.5 * H * (-C_ * acc[:, 1] - B_ * acc[:, 0])], 1))
        np.add.at(out["dL_dconic"], rows, -0.5 * acc[:, 2:5])
        np.add.at(out["dL_dopacity"], rows, acc[:, 5] / op)
        np.add.at(out["dL_dcolor"], rows, acc[:, 6:9])
    return out


def oracle_blend_grads(g):
    """the same four tensors out of Oracle.backward's dict"""
    P = g["dL_dopacity"].shape[0]
    con = np.asarray(g["dL_dconic"], np.float64).reshape(P, 4)
    return dict(dL_dmean2D=np.asarray(g["dL_dmean2D"], np.float64)[:, :2], dL_dconic=con[:, [0, 1, 3]],
                dL_dopacity=np.asarray(g["dL_dopacity"], np.float64).reshape(P), dL_dcolor=np.asarray(g["dL_dcolor"], np.float64))


# ------------------------------------------------------------------------------------------------------------------ the comparator
def case_errors(got, ref64, plan, names):
    """{(tensor, case): max |got - ref64| over the case's Gaussians, relative to the case's max-abs of ref64}"""
    out = {}
    P = plan["case"].size
    for k in names:
        a, b = np.asarray(got[k], np.float64).reshape(P, -1), np.asarray(ref64[k], np.float64).reshape(P, -1)
        for ci, c in enumerate(plan["cases"]):
            r = plan["case"] == ci
            scale = float(np.abs(b[r]).max())
            err = float(np.abs(a[r] - b[r]).max())
            out[(k, c["name"])] = (err / scale) if scale > 0 else (0.0 if err == 0 else np.inf)
    return out


def judge(got, ref32, ref64, plan, names, factor, floor):
    """The comparator of the blend-case suites: per tensor and case, the error of `got` against the fp64 reference, relative to the case's
    max-abs, must not exceed factor x max(the fp32 oracle's same figure, floor).  Returns ([failure messages], {(tensor, case): ratio})."""
    eg, er = case_errors(got, ref64, plan, names), case_errors(ref32, ref64, plan, names)
    bad, ratio = [], {}
    for key, e in eg.items():
        bound = max(er[key], floor)
        ratio[key] = e / bound
        if not e <= factor * bound:
            cells = sorted(c for c, owner in REQUIRED.items() if owner == key[1])
            bad.append(f"case {key[1]} ({', '.join(cells) or 'no cell of its own'}): {key[0]} off by {e:.3e} of the case's max-abs, "
                       f"fp32 oracle {er[key]:.3e}, allowed {factor} x {bound:.3e}")
    return bad, ratio


def never_blended_rows(pre, bins, plan):
    """bool [P]: Gaussians no pixel of ANY tile blends (their gradient rows must be exact zeros)"""
    P = pre["means2D"].shape[0]
    hit = np.zeros(P, bool)
    rng = bins["ranges"].astype(np.int64)
    for t in np.flatnonzero(rng[:, 1] > rng[:, 0]):
        d = _decide(pre, bins, plan, int(t))
        hit[d["rows"][d["blended"].any(axis=1)]] = True
    return ~hit
