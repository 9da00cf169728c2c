"""The designed front-end scenes of tests/footprint_cases.py ARE what they were designed to be, and each edge they reach is one a wrong rule
would show at — checked on the CPU oracle (oracle32 is the authority) and the module's numpy restatements, nothing hard-coded:
  * every rectangle size at every lane, the waves' instance totals, the cnt == 0 class, the exact-value culls, the border clamps, the
    get_rect tie, one visible row per single-r block, a clamped channel on every visible SH row;
  * the sensitivity proof: for each edge the ONE wrong rule it guards against is stated in numpy, and the scene has a row (or, for the
    staging threshold, a wave) whose expected result differs under it —
        `t < 16` read as `t <= 16`             footprint_cases.scheduled_count(lane_tiles=17)
        the sweep stepping 63                  footprint_cases.scheduled_count(sweep_step=63)
        a column predicate without (e + 3) / 45 footprint_cases.lost_floats
        `wcount < KB_CAP`                      footprint_cases.staged(strict=True)
        `+ 15` for `+ 16 - 1`                  footprint_cases.get_rect(plus15=True)
    No broken kernel runs anywhere."""
import math

import numpy as np
import pytest

import footprint_cases as fc

F32 = np.float32


def _grid(cam):
    return (cam.image_width + 15) // 16, (cam.image_height + 15) // 16


_refs = {}


def _ref(name, oracle):
    """(scene, oracle forward, numpy rectangle of every row from the oracle's means2D / radii, its tile count)"""
    if name not in _refs:
        s = fc.scene(name)
        ref = oracle.forward(s["sc"], s["camd"])
        pre = ref["pre"]
        rect = fc.get_rect(pre["means2D"][:, 0], pre["means2D"][:, 1], pre["radii"], *_grid(s["cam"]))
        _refs[name] = (s, ref, rect, np.where(pre["radii"] > 0, fc.rect_tiles(rect), 0))
    return _refs[name]


def _summary(name, ref):
    r = ref["bins"]["ranges"].astype(np.int64)
    print(f"{name}: P = {ref['pre']['radii'].size}, R = {ref['num_rendered']}, longest list = {int((r[:, 1] - r[:, 0]).max())}")


# ------------------------------------------------------------------------------------------------ the restatements themselves
def test_constants_are_the_issue_s():
    assert (fc.SEQ_TILES, fc.SWEEP, fc.KB_CAP, fc.SCAN_TILE) == (16, 64, 1024, 4096)
    assert fc.STRIP_SIZES == (1, 2, 15, 16, 17, 18, 79, 80, 81, 143, 144, 145, 160) and fc.STRIP_LANES == (0, 31, 32, 63)
    assert fc.ROW_COUNTS == (255, 256, 257, 4095, 4096, 4097, 8193)
    assert fc.SH_P == (1, 31, 32, 33, 63, 64, 65, 97, 173) and fc.SH_SINGLE == (0, 1, 2, 3, 30, 31, 32, 33, 62, 63)
    assert fc.SH_LDS == ((1, 15), (2, 15), (3, 15)) and fc.SH_PLAIN == ((0, 15), (0, 0), (1, 3), (2, 8))
    assert len(fc.SH_PATTERNS) == 13


def test_get_rect_restatement_against_the_oracle(oracle32):
    """the numpy get_rect is the oracle's on every designed row (radii as the float64 restatement gives them where the oracle culled),
    and on the documented tie"""
    tie = np.array([0x4357FFFF], np.uint32).view(F32)[0]
    assert float(tie) == 215.99998474121094 and F32(F32(tie + F32(25.0)) + F32(16.0)) == F32(257.0)
    assert [int(v[0]) for v in fc.get_rect([tie], [100.0], [25], 21, 12)] == list(oracle32.get_rect(float(tie), 100.0, 25, 21, 12))
    assert int(fc.get_rect([tie], [100.0], [25], 21, 12)[2][0]) == 16 and int(fc.get_rect([tie], [100.0], [25], 21, 12, plus15=True)[2][0]) == 15
    for name in fc.SCENES:
        s, ref, rect, _ = _ref(name, oracle32)
        pre = ref["pre"]
        gx, gy = _grid(s["cam"])
        for i in range(pre["radii"].size):
            want = oracle32.get_rect(float(pre["means2D"][i, 0]), float(pre["means2D"][i, 1]), int(pre["radii"][i]), gx, gy)
            assert tuple(int(v[i]) for v in rect) == want, (name, i)
    # values beyond the clamps
    big = fc.get_rect([-1e9, 1e9, np.nan, 5.0], [5.0, 5.0, 5.0, -40.0], [3, 3, 3, 20], 21, 12)
    for k, (px, py, r) in enumerate([(-1e9, 5.0, 3), (1e9, 5.0, 3), (5.0, -40.0, 20)]):
        k = k if k < 2 else 3
        assert tuple(int(v[k]) for v in big) == oracle32.get_rect(px, py, r, 21, 12)


def test_schedule_staging_and_column_restatements():
    for n in range(0, 200):
        assert fc.scheduled_count(np.ones(n, bool)) == n
        assert fc.scheduled_count(np.ones(n, bool), lane_tiles=17) == n + (n >= 17)
        assert fc.scheduled_count(np.ones(n, bool), sweep_step=63) == n + (n >= 80) + (n >= 143)
    p = np.zeros(100, bool); p[[3, 16, 79, 80]] = True
    assert (fc.scheduled_count(p), fc.scheduled_count(p, lane_tiles=17), fc.scheduled_count(p, sweep_step=63)) == (4, 5, 5)
    assert fc.staged(1024) and not fc.staged(1025) and fc.staged(1023, strict=True) and not fc.staged(1024, strict=True)
    # one visible row r among invisible ones loses its first (-45 r) mod 4 floats without the second term, and nothing with it
    for r in range(64):
        v = np.zeros(64, bool); v[r] = True
        lost = fc.lost_floats(v, 64)
        assert lost.sum() == (-45 * (r % 32)) % 4 and not lost[r, (-45 * (r % 32)) % 4:].any() and lost[r, :(-45 * (r % 32)) % 4].all()
        assert not fc.lost_floats(v, 64, without_second_term=False).any()
        assert not fc.lost_floats(v, 31).any()                                  # both half-blocks short: the scalar copy
        assert fc.lost_floats(v, 63).sum() == (lost.sum() if r < 32 else 0)     # the second half-block short
    assert not fc.lost_floats(np.ones(64, bool), 64).any()
    assert {(-45 * r) % 4 for r in fc.SH_SINGLE} == {0, 1, 2, 3} and {r // 32 for r in fc.SH_SINGLE} == {0, 1}


# ------------------------------------------------------------------------------------------------ strip
def test_strip_reaches_every_size_at_every_lane(oracle32):
    s, ref, rect, ntiles = _ref("strip", oracle32)
    _summary("strip", ref)
    pre, plan = ref["pre"], s["plan"]
    assert plan["dropped"] == [] and _grid(s["cam"]) == (160, 1)
    tt = pre["tiles_touched"].astype(np.int64)
    vis = pre["radii"] > 0
    np.testing.assert_array_equal(tt[vis], ntiles[vis])                # opacity 0.99: every tile of the rectangle passes
    lane = np.arange(tt.size) % 64
    for n in fc.STRIP_SIZES:
        for l in fc.STRIP_LANES:
            assert ((ntiles == n) & (lane == l) & vis).any(), (n, l)
    assert {(int(ntiles[row]), int(row % 64)) for row, _ in plan["sizes"]} == {(n, l) for n in fc.STRIP_SIZES for l in fc.STRIP_LANES}
    whole = ntiles == 160
    assert whole.any() and (rect[0][whole] == 0).all() and (rect[2][whole] == 160).all()
    # waves: swept rows per wave; a swept row with culled rows on both sides
    swept = ntiles > fc.SEQ_TILES
    per_wave = np.add.reduceat(swept.astype(np.int64), np.arange(0, tt.size, 64))
    assert per_wave[plan["many_swept"]] >= 4 and per_wave.max() >= 4
    row, w = plan["between"]
    assert swept[row] and not vis[row - 1] and not vis[row + 1] and not vis[row - 2] and not vis[row + 2] and row // 64 == w
    assert {s["plan"]["tag"][row + d] for d in (-2, -1, 1, 2)} == {"around-swept"}
    # invisible rows of all three kinds stand between the designed ones
    z, op = s["sc"]["means"][:, 2], s["sc"]["opac"][:, 0]
    assert (z < 0).any() and ((z > 0) & (z <= F32(0.2))).any() and ((z > F32(0.2)) & (op < F32(1.0) / F32(255.0))).any()
    assert tt.size % 64 != 0
    # ---- sensitivity: SEQ_TILES and the sweep's step.  Every tile of these rectangles passes, so the schedule's count is a function of n.
    right = np.array([fc.scheduled_count(np.ones(n, bool)) for n in ntiles])
    np.testing.assert_array_equal(right, tt)
    le16 = np.array([fc.scheduled_count(np.ones(n, bool), lane_tiles=17) for n in ntiles])
    step63 = np.array([fc.scheduled_count(np.ones(n, bool), sweep_step=63) for n in ntiles])
    assert (le16[ntiles == 17] != 17).all() and (le16[ntiles == 16] == 16).all() and (ntiles == 17).any() and (ntiles == 16).any()
    assert (step63[ntiles == 80] != 80).all() and (step63[ntiles == 79] == 79).all() and (step63[ntiles == 81] != 81).all()
    assert (step63[ntiles == 143] == 145).all() and (step63[ntiles == 144] == 146).all() and (step63[ntiles == 145] == 147).all()
    assert (le16 != tt).sum() == int((ntiles >= 17).sum()) and (step63 != tt).sum() == int((ntiles >= 80).sum())


# ------------------------------------------------------------------------------------------------ waves
def test_waves_have_the_designed_totals(oracle32):
    s, ref, rect, ntiles = _ref("waves", oracle32)
    _summary("waves", ref)
    pre, plan = ref["pre"], s["plan"]
    assert plan["dropped"] == []
    tt = pre["tiles_touched"].astype(np.int64)
    np.testing.assert_array_equal(tt, ntiles)
    totals, last = fc.wave_totals(tt)
    by_name = {}
    for w, (name, first, rows, total) in enumerate(plan["waves"]):
        assert first == 64 * w and totals[w] == total, (name, totals[w], total)
        by_name[name] = (w, tt[first:first + rows])
    swept = lambda name: int((by_name[name][1] > fc.SEQ_TILES).sum())
    assert totals[by_name["1024-seqmask"][0]] == 1024 and swept("1024-seqmask") == 0 and (by_name["1024-seqmask"][1] == 16).all()
    assert totals[by_name["1025"][0]] == 1025
    assert totals[by_name["1024-swept"][0]] == 1024 and swept("1024-swept") >= 2
    assert totals[by_name["1023"][0]] == 1023
    big = by_name["thousands"]
    assert totals[big[0]] >= 3000 and swept("thousands") >= 4 and int(((big[1] > 0) & (big[1] <= fc.SEQ_TILES)).sum()) >= 4
    e = by_name["empty"][0]
    assert totals[e] == 0 and totals[e - 1] > 0 and totals[e + 1] > 0
    assert tt.size % 64 != 0 and last[-1] == (tt.size - 1) % 64 < 63 and totals[-1] > 0 and swept("partial") >= 1
    # the staged waves hold both sub-paths, and so do the direct ones
    for name in ("1024-swept", "1025", "thousands"):
        assert swept(name) >= 1 and int(((by_name[name][1] > 0) & (by_name[name][1] <= fc.SEQ_TILES)).sum()) >= 1
    # a staged 1025 would spill into the LDS of the next wave of its workgroup: the 1025 wave is not the last of its four
    assert by_name["1025"][0] % 4 != 3
    # ---- sensitivity: `wcount < KB_CAP`.  The rule decides a wave's PATH (both paths write the same lists): the waves of exactly 1024 change it
    flips = np.nonzero(fc.staged(totals) != fc.staged(totals, strict=True))[0]
    assert sorted(flips.tolist()) == sorted([by_name["1024-seqmask"][0], by_name["1024-swept"][0]])
    assert fc.staged(totals).tolist() == [True, False, True, True, False, True, True]


@pytest.mark.parametrize("P", fc.ROW_COUNTS)
def test_row_counts_tile_the_waves(oracle32, P):
    s = fc.row_counts(P)
    ref = oracle32.forward(s["sc"], s["camd"])
    _summary(f"row_counts({P})", ref)
    base = _ref("waves", oracle32)[1]["pre"]["tiles_touched"]
    tt = ref["pre"]["tiles_touched"]
    assert tt.size == P and s["sc"]["shs"].shape[1] == 0 and s["sc"]["D"] == 0
    np.testing.assert_array_equal(tt, base[np.arange(P) % base.size])
    assert ref["num_rendered"] <= 200000
    totals, _ = fc.wave_totals(tt)
    assert (totals > fc.KB_CAP).any() and ((totals > 0) & (totals <= fc.KB_CAP)).any()
    # the 256-thread block edge and the one-tile | chained edge of the scan over P
    assert P in (255, 256, 257) or abs(P - fc.SCAN_TILE) <= 1 or P > 2 * fc.SCAN_TILE


# ------------------------------------------------------------------------------------------------ border
def _f64_rect(s, i):
    """float64 radius and the rectangle it gives around the float32 restatement of the mean: (3 sqrt(lambda_1), det, rectangle)"""
    cam, sc = s["cam"], s["sc"]
    three_sigma, det = fc.radius64(cam, sc["means"][i].astype(np.float64), sc["scales"][i].astype(np.float64), sc["rots"][i].astype(np.float64))
    mx, my = fc.project32(cam, sc["means"][i:i + 1])
    return three_sigma, det, fc.get_rect(mx, my, [math.ceil(three_sigma)], *_grid(cam))


def test_border_reaches_the_clamps_the_empty_classes_and_the_tie(oracle32):
    s, ref, rect, ntiles = _ref("border", oracle32)
    _summary("border", ref)
    pre, plan, cam = ref["pre"], s["plan"], s["cam"]
    W, H = cam.image_width, cam.image_height
    gx, gy = _grid(cam)
    assert (W, H, gx, gy) == (333, 190, 21, 12) and plan["dropped"] == []
    m, vis, tt = pre["means2D"], pre["radii"] > 0, pre["tiles_touched"].astype(np.int64)
    out_x = np.where(m[:, 0] < 0, -1, np.where(m[:, 0] > W - 1, 1, 0))
    out_y = np.where(m[:, 1] < 0, -1, np.where(m[:, 1] > H - 1, 1, 0))
    sign = dict(left=(-1, 0), right=(1, 0), top=(0, -1), bottom=(0, 1), topleft=(-1, -1), topright=(1, -1), bottomleft=(-1, 1), bottomright=(1, 1))
    assert set(plan["sides"]) == set(sign)
    for name, rows in plan["sides"].items():
        rows = np.asarray(rows)
        sx, sy = sign[name]
        outside = (out_x[rows] == sx) & (out_y[rows] == sy)
        assert (outside & vis[rows]).any(), name                          # a mean outside this side still reaches the image
        assert (~outside & vis[rows] & (out_x[rows] == 0) & (out_y[rows] == 0)).any(), name
        near = lambda v, e: np.abs(v - e) < 1e-3                           # (the mean is a float32 result: on the edge pixel's centre to 1e-3)
        on_edge = (near(m[rows, 0], 0 if sx < 0 else W - 1) if sx else True) & (near(m[rows, 1], 0 if sy < 0 else H - 1) if sy else True)
        assert np.any(on_edge & vis[rows]), name
        r = pre["radii"][rows].astype(np.float64)
        dx = np.maximum(np.where(sx < 0, -m[rows, 0], m[rows, 0] - (W - 1)), 0) if sx else np.zeros(rows.size)
        dy = np.maximum(np.where(sy < 0, -m[rows, 1], m[rows, 1] - (H - 1)), 0) if sy else np.zeros(rows.size)
        far = np.hypot(dx, dy)[vis[rows]]
        assert (far <= r[vis[rows]]).all() and (far >= 0.9 * r[vis[rows]]).any(), name    # up to a radius outside
        # the rectangle is cut by the clamp on this side
        if sx:
            assert ((rect[0][rows] == 0) & (m[rows, 0] - r < 0) if sx < 0 else (rect[2][rows] == gx) & (m[rows, 0] + r >= 16 * gx))[vis[rows]].any(), name
        if sy:
            assert ((rect[1][rows] == 0) & (m[rows, 1] - r < 0) if sy < 0 else (rect[3][rows] == gy) & (m[rows, 1] + r >= 16 * gy))[vis[rows]].any(), name
    # clamped to nothing: the float64 radius is positive, the rectangle has no tile
    assert len(plan["zero"]) == 4
    for i in plan["zero"]:
        three_sigma, det, r64 = _f64_rect(s, i)
        assert pre["radii"][i] == 0 and three_sigma > 1 and det > 0 and int(fc.rect_tiles(r64)[0]) == 0, i
        assert s["sc"]["means"][i, 2] > F32(0.2) and s["sc"]["opac"][i, 0] >= F32(1.0) / F32(255.0)
    # slanted: the exact test rejects tiles of the rectangle, on the lane's side of SEQ_TILES and on the sweep's
    sl = np.asarray(plan["slanted"])
    assert vis[sl].all() and (tt[sl] < ntiles[sl]).all() and (ntiles[sl] <= fc.SEQ_TILES).sum() >= 2 and (ntiles[sl] > fc.SEQ_TILES).sum() >= 3
    assert (ntiles[sl] > fc.SEQ_TILES + fc.SWEEP).any()                   # (... one of them over two sweep steps)
    # cnt == 0: a non-empty rectangle, neither cull applies, no tile passes
    none = [i for i in range(tt.size) if not vis[i] and s["sc"]["means"][i, 2] > F32(0.2) and s["sc"]["opac"][i, 0] >= F32(1.0) / F32(255.0)
            and _f64_rect(s, i)[1] > 0 and int(fc.rect_tiles(_f64_rect(s, i)[2])[0]) > 0]
    assert set(plan["none_passes"]) <= set(none) and len(plan["none_passes"]) >= 3
    for i in none:
        assert pre["radii"][i] == 0 and tt[i] == 0
    print("cnt == 0 rows:", none, "(designed:", plan["none_passes"], ")")
    # ---- the tie, and its sensitivity: `+ 15` for `+ 16 - 1`
    tie = np.asarray(plan["tie"])
    np.testing.assert_array_equal(m[tie, 0].view(np.uint32), np.asarray(plan["tie_x"], F32).view(np.uint32))
    assert m[tie[0], 0] == F32(215.99998) and pre["radii"][tie[0]] == 25 and vis[tie].all()
    wrong = fc.get_rect(m[:, 0], m[:, 1], pre["radii"], gx, gy, plus15=True)
    assert (rect[2][tie] == 16).all() and (wrong[2][tie] == 15).all()           # x1 is the larger value
    differs = np.nonzero(vis & ((wrong[2] != rect[2]) | (wrong[3] != rect[3])))[0]
    assert sorted(differs.tolist()) == sorted(tie.tolist())
    # the column the wrong rule loses holds tiles that pass (the oracle's lists have the row in tile column 15): tiles_touched, R and the
    # lists themselves would differ
    tiles = (ref["bins"]["keys"] >> np.uint64(32)).astype(np.int64)
    for i in tie:
        assert (tiles[ref["bins"]["point_list"] == i] % gx == 15).any(), i


# ------------------------------------------------------------------------------------------------ culls
def test_exact_value_culls_fall_on_their_side(oracle32):
    s, ref, rect, ntiles = _ref("culls", oracle32)
    _summary("culls", ref)
    pre, rows, sc, cam = ref["pre"], s["plan"]["rows"], s["sc"], s["cam"]
    assert s["plan"]["dropped"] == []
    near, one = F32(0.2), F32(1.0) / F32(255.0)
    z, op = sc["means"][:, 2], sc["opac"][:, 0]
    assert z[rows["z=0.2"][0]] == near and z[rows["z=next(0.2)"][0]] == np.nextafter(near, F32(1.0))
    assert op[rows["op=1/255"][0]] == one and op[rows["op=prev(1/255)"][0]] == np.nextafter(one, F32(0.0))
    assert z[rows["behind"][0]] < 0
    np.testing.assert_array_equal(s["act"]["means"].numpy(), sc["means"])
    for name, (i, kept) in rows.items():
        assert (pre["radii"][i] > 0) == kept and (pre["tiles_touched"][i] > 0) == kept, name
    assert pre["tiles_touched"][rows["op=1/255"][0]] == 1           # cull threshold log(1) = 0: only the tile that holds the mean
    # the two invisible exact-value rows are invisible BY that value: their neighbour across the threshold has the same geometry
    for a, b in (("z=0.2", "z=next(0.2)"), ("op=1/255", "op=prev(1/255)")):
        np.testing.assert_allclose(sc["means"][rows[a][0], :2], sc["means"][rows[b][0], :2], rtol=1e-5)
        np.testing.assert_allclose(sc["scales"][rows[a][0]], sc["scales"][rows[b][0]], rtol=1e-5)
    i = rows["jacobian-clamped"][0]
    assert sc["means"][i, 0] / sc["means"][i, 2] < cam.limx_neg and pre["radii"][i] > 0
    from conftest import clamp_masked_visible
    assert clamp_masked_visible(sc, s["camd"], pre["radii"]) >= 1


# ------------------------------------------------------------------------------------------------ sh_blocks
def test_sh_blocks_grid(oracle32):
    """every (P, pattern): the oracle's visibility is the designed one; every single-r block has exactly one visible row, at r; every visible
    row has a clamped channel (whatever D, M); the patterns that design nothing are the ones a rule predicts"""
    dropped = []
    for P in fc.SH_P:
        for pattern in fc.SH_PATTERNS:
            for D, M in ((3, 15), (0, 15), (1, 3)) if pattern in ("all", "alternate") else ((3, 15),):
                s = fc.sh_blocks(D, M, P, pattern)
                pre = oracle32.preprocess(s["sc"], s["camd"])
                vis = pre["radii"] > 0
                np.testing.assert_array_equal(vis, s["plan"]["visible"], err_msg=f"{P} {pattern}")
                assert s["sc"]["shs"].shape == (P, M, 3) and s["sc"]["D"] == D
                if vis.any():
                    assert (pre["clamped"][vis].sum(1) >= 1).all() and (pre["clamped"][vis].sum(1) < 3).any() or vis.sum() < 3, (P, pattern, D, M)
                    assert pre["clamped"][vis, 1 + np.nonzero(vis)[0] % 2].all()
                assert not pre["clamped"][~vis].any()
            dropped += s["plan"]["dropped"]
            if pattern.startswith("single-"):
                r = int(pattern.split("-")[1])
                for b in range(0, P, 64):
                    rows = min(P - b, 64)
                    assert np.nonzero(vis[b:b + rows])[0].tolist() == ([r] if r < rows else []), (P, pattern, b)
            if pattern == "alternate":
                assert vis[::2].all() and not vis[1::2].any()
            # invisible by both culls
            if pattern == "none" and P > 1:
                z, op = s["sc"]["means"][:, 2], s["sc"]["opac"][:, 0]
                assert (z <= F32(0.2)).any() and ((z > F32(0.2)) & (op < F32(1.0) / F32(255.0))).any()
    assert dropped == [(P, f"single-{r}") for P in fc.SH_P for r in fc.SH_SINGLE if P <= r]
    # the last block's rows and both half-blocks take every branch: full, short (scalar copy), absent
    halves = {(min(max(P - b - 32 * h, 0), 32)) for P in fc.SH_P for b in range(0, P, 64) for h in range(2)}
    assert {0, 1, 31, 32}.issubset(halves) and any(0 < v < 32 for v in halves)
    assert {min(P - b, 64) for P in fc.SH_P for b in range(0, P, 64)} >= {1, 31, 32, 33, 63, 64, 45}


def test_sh_clamps_on_every_degree(oracle32):
    for D, M in fc.SH_LDS + fc.SH_PLAIN:
        s = fc.sh_blocks(D, M, 173, "all")
        ref = oracle32.forward(s["sc"], s["camd"])
        if (D, M) == (3, 15):
            _summary("sh_blocks(3, 15, 173, all)", ref)
        c = ref["pre"]["clamped"]
        # channel 0 never clamps (a row's first SH float shows in it), channels 1 and 2 clamp on some rows and survive on others
        assert not c[:, 0].any() and c[:, 1:].any(0).all() and (~c[:, 1:]).any(0).all(), (D, M)
        d = s["sc"]["means"] - s["camd"]["campos"]
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
        # no direction along an axis (at least two components alive on every row, all three on nine in ten): every basis function counts
        assert (np.abs(d).min(1) > 0.02).all()


def test_column_predicate_sensitivity(oracle32):
    """Without the (e + 3) / 45 term a visible row whose first float4 column begins in an invisible neighbour's row loses its first floats.
    For every LDS scene of the grid the lost floats are stated by footprint_cases.lost_floats; zeroing them in the oracle's input changes the
    row's rgb — on every alignment 45 r mod 4 != 0, in both half-blocks, and never where the half-block takes the scalar copy."""
    seen = set()
    for D, M in fc.SH_LDS:
        for P in fc.SH_P:
            for pattern in fc.SH_PATTERNS:
                s = fc.sh_blocks(D, M, P, pattern)
                vis = s["plan"]["visible"]
                lost = np.zeros((P, 45), bool)
                for b in range(0, P, 64):
                    rows = min(P - b, 64)
                    v = np.zeros(64, bool); v[:rows] = vis[b:b + rows]
                    assert not fc.lost_floats(v, rows, without_second_term=False).any()
                    lost[b:b + rows] = fc.lost_floats(v, rows)[:rows]
                if pattern == "all":
                    assert not lost.any()
                if not lost.any():
                    continue
                sc = dict(s["sc"])
                sc["shs"] = np.where(lost.reshape(P, 15, 3), F32(0), s["sc"]["shs"])
                a, b_ = oracle32.preprocess(s["sc"], s["camd"])["rgb"], oracle32.preprocess(sc, s["camd"])["rgb"]
                hit = np.nonzero(lost.any(1))[0]
                changed = np.abs(a[hit] - b_[hit]).max(1)
                # (1e-4: a hundred times the 1e-6 the GPU test holds rgb to.  A lone visible row shows it always; of the alternate pattern's
                # many rows those whose direction has y near 0 — the first SH term's factor — may not, most do)
                assert (changed > 1e-4).all() if pattern.startswith("single-") else (changed > 1e-4).mean() > 0.75, (D, P, pattern, hit[changed <= 1e-4])
                same = np.setdiff1d(np.arange(P), hit)
                np.testing.assert_array_equal(a[same], b_[same])
                for r in hit:
                    seen.add((D, int(lost[r].sum()), int(r % 64) // 32, pattern.split("-")[0]))
    for D, _ in fc.SH_LDS:
        for n in (1, 2, 3):
            for h in (0, 1):
                assert (D, n, h, "single") in seen, (D, n, h)
