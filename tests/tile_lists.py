"""Scenes whose per-tile instance lists are DESIGNED: every (length, tie pattern) case gets a tile of its own, so that the per-tile depth sort
(csrc/radix_sort.hip: tile_depth_sort_wave_kernel up to LW_CAP = 1024 instances, tile_depth_sort_kernel in LDS up to LS_CAP = 4096 and in
global scratch beyond) is reached at the exact lengths and tie structures where its paths change, and a plain numpy statement of the lists
the forward must produce.  No GPU, no library: numpy and the scene generator only.

The construction.  Identity pose, so a Gaussian's depth key is the float32 bit pattern of its z.  A Gaussian of tile (tx, ty) sits within
+-2 px of the tile's centre with a scale of 1e-4 and a constant opacity: radius 3, exactly one tile touched, nothing culled — the tile's list
length is the number of Gaussians placed there.  The rows are shuffled across the tiles, so a tile's Gaussians are not contiguous rows; the
LOCAL row order of a tile (its rows, ascending) is what `order` of a pattern refers to.

The tie patterns are stated in sorted positions of the list (E = ceil(n / 64) is the one-wave kernel's run per lane: sorted positions
E-1 and E are the last element of lane 0's run and the first of lane 1's).  Which ROW of two equal keys comes first in the input is not the
pattern's business: the radix path delivers row order, the atomic path arrival order, and a permuted map (tie_rank) whatever its permutation
makes of it — the reversal turns every tied pair and run into descending order of the second key."""
import math

import numpy as np
import torch

from conftest import make_scene

LENGTHS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 960, 961, 1009, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 5121)

# depth keys are uint32 bit patterns of positive float32 z above the near cut of 0.2
Z1, Z30 = 0x3F800000, 0x41F00000              # 1.0 .. 30.0: where the distinct keys of the tie patterns come from
Z_EQUAL = 0x40400000                          # 3.0
Z_NARROW = 0x40A00000                         # 5.0 (+ 0..15)
Z_QUARTER, Z_2P30, Z_2P60 = 0x3E800000, 0x4E800000, 0x5D800000   # 0.25, 2^30 (0.25 + 2^28 in bits), 2^60

PATTERNS = ("distinct-random", "distinct-ascending", "distinct-descending", "all-equal", "pairs-1", "pairs-8", "pairs-9", "run-9", "run-10",
            "narrow", "wide", "wide-low16-zero")


def lane_run(n):
    return (n + 63) // 64


def _distinct(rng, n, lo, hi, step=1):
    """n distinct multiples of `step` in [lo, hi], ascending (uint32)"""
    m = (hi - lo) // step + 1
    assert m >= n
    if m <= 4 * n:
        v = rng.permutation(m)[:n]
    else:
        v = np.unique(rng.integers(0, m, size=2 * n + 16))
        while v.size < n:
            v = np.unique(np.concatenate([v, rng.integers(0, m, size=2 * n + 16)]))
        v = rng.permutation(v)[:n]
    return (np.sort(v).astype(np.uint64) * step + lo).astype(np.uint32)


def _with_duplicates(rng, n, dup):
    """sorted keys of a list whose sorted position p repeats the key of p - 1 where dup[p], all other neighbours distinct"""
    vals = _distinct(rng, int(n - dup.sum()), Z1, Z30)
    return vals[np.cumsum(~dup) - 1]


def pair_positions(n, k):
    """Sorted positions s of k disjoint tied pairs (s, s + 1), or None when they do not fit.  Taken greedily in this order: with three pairs or
    more the head (0, 1) and the tail (n - 2, n - 1) first; then the lane boundaries (m E - 1, m E), m = 1, 2, ... — (E - 1, E) is the last element
    of lane 0's run and the first of lane 1's; with E = 1 it IS the head, and with E = 2 it overlaps the head, so that the boundary pair is
    lane 1 | lane 2's (3, 4) — then whatever position is left, ascending."""
    if n < 2 * k:
        return None
    E = lane_run(n)
    cand = ([0, n - 2] if k >= 3 else []) + [m * E - 1 for m in range(1, 64)] + list(range(n - 1))
    taken = []
    for s in cand:
        if 0 <= s and s + 1 < n and all(abs(s - t) >= 2 for t in taken):
            taken.append(s)
            if len(taken) == k:
                return sorted(taken)
    return None


def run_position(n, L, where):
    """First sorted position of a run of L equal keys, or None when the list is shorter than the run.  "boundary": the run straddles the
    boundary between lane 0's and lane 1's runs (positions E - 1 | E) — it starts L // 2 before E, or at 0 when E is smaller than that."""
    if n < L:
        return None
    if where == "head":
        return 0
    if where == "tail":
        return n - L
    return min(max(lane_run(n) - L // 2, 0), n - L)


def design(n, pattern, where, rng):
    """One tile's case: None when the pattern does not fit n, else dict(keys = the depth keys in the tile's LOCAL ROW order, pairs = equal
    neighbours of the sorted list, lo / hi = the bracket kmax - kmin must lie in (hi exclusive, None = unbounded))."""
    u32 = lambda a: np.asarray(a, np.uint32)
    if pattern.startswith("distinct"):
        keys = _distinct(rng, n, Z1, Z30)
        order = pattern.split("-")[1]
        keys = keys[::-1].copy() if order == "descending" else (rng.permutation(keys) if order == "random" else keys)
        return dict(keys=u32(keys), pairs=0, lo=0, hi=None)
    if pattern == "all-equal":
        return dict(keys=np.full(n, Z_EQUAL, np.uint32), pairs=max(n - 1, 0), lo=0, hi=1)
    if pattern.startswith("pairs-") or pattern.startswith("run-"):
        count = int(pattern.split("-")[1])
        dup = np.zeros(n, bool)
        if pattern.startswith("pairs-"):
            pos = pair_positions(n, count)
            if pos is None:
                return None
            dup[np.asarray(pos, np.int64) + 1] = True
        else:
            s = run_position(n, count, where)
            if s is None:
                return None
            dup[s + 1:s + count] = True
        return dict(keys=u32(rng.permutation(_with_duplicates(rng, n, dup))), pairs=int(dup.sum()), lo=0, hi=None)
    if pattern == "narrow":
        keys = u32(Z_NARROW + rng.integers(0, 16, size=n))
        return dict(keys=keys, pairs=int(n - np.unique(keys).size), lo=0, hi=16)
    if pattern in ("wide", "wide-low16-zero"):
        step, top = (1, Z_2P30) if pattern == "wide" else (1 << 16, Z_2P60)
        keys = _distinct(rng, n, Z_QUARTER, top, step)
        if n >= 2:
            keys[0], keys[-1] = Z_QUARTER, top     # (the span itself: 2^28 in bits at the least)
        return dict(keys=u32(rng.permutation(keys)), pairs=0, lo=(1 << 28) if n >= 2 else 0, hi=None)
    raise ValueError(pattern)


def cases_of(pattern, lengths=LENGTHS):
    """the (n, pattern, where) cases of one scene: every length once; the run patterns at the lane boundary, the head and the tail"""
    wheres = ("boundary", "head", "tail") if pattern.startswith("run-") else ("",)
    return [(n, pattern, w) for w in wheres for n in lengths]


def build(cases, W=320, H=192, seed=0):
    """cases: [(n, pattern, where)].  Every case that fits gets a tile of its own (tiles in a seeded random order).
    Returns (raw, sc, camd, cam, plan): make_scene's four, and plan = dict(T, tile [P] the tile of every row, key [P] its designed depth key
    (uint32), cases [dict(tile, n, pattern, where, pairs, lo, hi)], dropped [(n, pattern, where)] the cases that did not fit)."""
    rng = np.random.default_rng(seed)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    T = gx * gy
    placed, dropped, keys = [], [], []
    for n, pattern, where in cases:
        d = design(n, pattern, where, rng)
        if d is None:
            dropped.append((n, pattern, where))
            continue
        assert d["keys"].shape == (n,) and d["keys"].dtype == np.uint32
        keys.append(d.pop("keys"))
        placed.append(dict(n=n, pattern=pattern, where=where, **d))
    assert len(placed) <= T and W % 16 == 0 and H % 16 == 0
    for c, t in zip(placed, rng.permutation(T)[:len(placed)]):
        c["tile"] = int(t)
    P = int(sum(c["n"] for c in placed))
    # a tile's keys are in its LOCAL row order: its rows are handed out ascending, from a shuffle of all rows
    tile_sorted = np.repeat(np.array([c["tile"] for c in placed], np.int64), [c["n"] for c in placed])
    rows = np.concatenate([np.sort(r) for r in np.split(rng.permutation(P), np.cumsum([c["n"] for c in placed])[:-1])]) if P else np.zeros(0, np.int64)
    tile = np.empty(P, np.int64)
    key = np.empty(P, np.uint32)
    tile[rows] = tile_sorted
    key[rows] = np.concatenate(keys) if P else np.zeros(0, np.uint32)

    raw, _, camd, cam = make_scene("random", P, W, H, 3, seed)
    z = key.view(np.float32).astype(np.float64)
    assert np.all(z > 0.2)
    px = 16.0 * (tile % gx) + 8.0 + rng.uniform(-2.0, 2.0, P) + 0.5     # (the projection puts x fx / z + cx - 1/2 into the image)
    py = 16.0 * (tile // gx) + 8.0 + rng.uniform(-2.0, 2.0, P) + 0.5
    xyz = np.stack([(px - float(cam.cx)) / float(cam.fx) * z, (py - float(cam.cy)) / float(cam.fy) * z, z], 1).astype(np.float32)
    assert np.array_equal(xyz[:, 2].view(np.uint32), key)
    raw["xyz"] = torch.from_numpy(xyz).contiguous()
    raw["scaling"] = torch.full((P, 3), math.log(1e-4), dtype=torch.float32)
    raw["opacity"] = torch.full((P, 1), -3.0, dtype=torch.float32)
    from gaussian_lic_amd.synthetic import activate, to_numpy
    return raw, to_numpy(activate(raw)), camd, cam, dict(T=T, tile=tile, key=key, cases=placed, dropped=dropped)


def scene(pattern, W=320, H=192):
    """the scene of one pattern of PATTERNS (seeded by the pattern's position)"""
    return build(cases_of(pattern), W, H, seed=100 + PATTERNS.index(pattern))


def expected_lists(tile, key, T, tie_rank=None):
    """The lists the forward must produce for rows with the given tile and depth key: per tile, ascending (depth key, original index) —
    the reference's stable sort of an index-ordered emission.  For a permuted map `tile` and `key` are in STORAGE row order and
    tie_rank[row] is the row's original index: the order is by (depth key, tie_rank[row]) and the list holds storage rows.
    Returns dict(R, ranges [T, 2] uint32, keys [R] uint64 = tile << 32 | depth key, point_list [R] uint32)."""
    tile = np.asarray(tile, np.int64)
    key = np.asarray(key, np.uint32)
    second = np.arange(tile.size, dtype=np.int64) if tie_rank is None else np.asarray(tie_rank, np.int64)
    order = np.lexsort((second, key, tile))
    end = np.cumsum(np.bincount(tile, minlength=T))
    ranges = np.stack([end - np.bincount(tile, minlength=T), end], 1)
    ranges[ranges[:, 0] == ranges[:, 1]] = 0        # (an empty tile's range is never written: it stays (0, 0))
    return dict(R=int(tile.size), ranges=ranges.astype(np.uint32), keys=(tile[order].astype(np.uint64) << np.uint64(32)) | key[order].astype(np.uint64),
                point_list=order.astype(np.uint32))


def tile_stats(keys64, ranges):
    """(equal-neighbour pairs, kmax - kmin) per tile of a sorted key array (uint64: tile << 32 | depth) and its ranges"""
    d = (np.asarray(keys64, np.uint64) & np.uint64(0xffffffff)).astype(np.int64)
    pairs, span = np.zeros(len(ranges), np.int64), np.zeros(len(ranges), np.int64)
    for t, (a, b) in enumerate(np.asarray(ranges, np.int64)):
        if b > a:
            pairs[t] = int((d[a + 1:b] == d[a:b - 1]).sum())
            span[t] = int(d[b - 1] - d[a])
    return pairs, span
