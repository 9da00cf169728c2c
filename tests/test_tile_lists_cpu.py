"""The designed tile-list scenes of tests/tile_lists.py ARE what they were designed to be — checked on the CPU oracle with no allowance:
one tile per Gaussian, the designed list length per tile, depth key = the bits of z, the designed number of equal neighbours and key span
per tile, and the oracle's lists equal to the plain numpy statement of them (tile_lists.expected_lists), also for a permuted map."""
import numpy as np
import pytest

import tile_lists as tl

# what the builder drops, by rule (tile_lists.pair_positions / run_position): k disjoint pairs need 2 k elements, a run of L needs L
DROPPED = {
    "pairs-1": [(0, "pairs-1", ""), (1, "pairs-1", "")],
    "pairs-8": [(n, "pairs-8", "") for n in (0, 1, 2, 3)],
    "pairs-9": [(n, "pairs-9", "") for n in (0, 1, 2, 3)],
    "run-9": [(n, "run-9", w) for w in ("boundary", "head", "tail") for n in (0, 1, 2, 3)],
    "run-10": [(n, "run-10", w) for w in ("boundary", "head", "tail") for n in (0, 1, 2, 3)],
}


def test_lengths_are_the_issue_s():
    assert tl.LENGTHS == (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 960, 961, 1009, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 5121)
    assert len(tl.PATTERNS) == 12


@pytest.mark.parametrize("n,k,want", [
    (2, 1, [0]), (3, 1, [0]), (65, 1, [1]), (1024, 1, [15]),
    (16, 8, [0, 2, 4, 6, 8, 10, 12, 14]),
    (1024, 8, [0, 15, 31, 47, 63, 79, 95, 1022]),
    (1024, 9, [0, 15, 31, 47, 63, 79, 95, 111, 1022]),
    (65, 8, [0, 3, 5, 7, 9, 11, 13, 63]),
    (3, 8, None), (1, 1, None),
])
def test_pair_positions(n, k, want):
    assert tl.pair_positions(n, k) == want


@pytest.mark.parametrize("n,L,where,want", [
    (1024, 9, "boundary", 12), (1024, 10, "boundary", 11), (1024, 9, "head", 0), (1024, 9, "tail", 1015), (63, 9, "boundary", 0),
    (9, 9, "boundary", 0), (9, 9, "tail", 0), (3, 9, "head", None), (5121, 10, "boundary", 76),
])
def test_run_position(n, L, where, want):
    s = tl.run_position(n, L, where)
    assert s == want
    if s is not None and where == "boundary" and n > L:
        E = tl.lane_run(n)
        assert s <= E - 1 and s + L - 1 >= E       # lane 0's last element and lane 1's first are both inside the run


def test_expected_lists_on_a_hand_case():
    tile = np.array([2, 0, 2, 2, 0])
    key = np.array([7, 5, 7, 3, 5], np.uint32)
    e = tl.expected_lists(tile, key, 4)
    assert e["point_list"].tolist() == [1, 4, 3, 0, 2] and e["ranges"].tolist() == [[0, 2], [0, 0], [2, 5], [0, 0]]
    assert e["keys"].tolist() == [5, 5, (2 << 32) | 3, (2 << 32) | 7, (2 << 32) | 7]
    # the same rows stored in reverse (storage row s = original row 4 - s): the ties follow the ORIGINAL index, the list holds storage rows
    perm = np.arange(5)[::-1]
    p = tl.expected_lists(tile[perm], key[perm], 4, tie_rank=perm)
    assert perm[p["point_list"]].tolist() == e["point_list"].tolist() and p["point_list"].tolist() == [3, 0, 1, 4, 2]


@pytest.fixture(scope="module")
def built():
    cache = {}

    def get(pattern, oracle):
        if pattern not in cache:
            raw, sc, camd, cam, plan = tl.scene(pattern)
            cache[pattern] = (sc, plan, oracle.forward(sc, camd))
        return cache[pattern]
    return get


@pytest.mark.parametrize("pattern", tl.PATTERNS)
def test_scene_is_what_was_designed(oracle32, built, pattern):
    sc, plan, ref = built(pattern, oracle32)
    assert plan["dropped"] == DROPPED.get(pattern, [])
    assert sorted({c["n"] for c in plan["cases"]} | {d[0] for d in plan["dropped"]}) == list(tl.LENGTHS)
    P, T = plan["tile"].size, plan["T"]
    pre, bins = ref["pre"], ref["bins"]
    assert (pre["radii"] > 0).all() and (pre["tiles_touched"] == 1).all()
    assert ref["num_rendered"] == P
    r = bins["ranges"].astype(np.int64)
    length = r[:, 1] - r[:, 0]
    want = np.zeros(T, np.int64)
    for c in plan["cases"]:
        want[c["tile"]] = c["n"]
    np.testing.assert_array_equal(length, want)
    np.testing.assert_array_equal(np.bincount(plan["tile"], minlength=T), want)
    # the rows of a tile are not contiguous
    big = next(c for c in plan["cases"] if c["n"] == 1024)
    assert np.ptp(np.nonzero(plan["tile"] == big["tile"])[0]) > 4 * 1024
    # depth key = the bits of z
    np.testing.assert_array_equal(pre["depths"].view(np.uint32), plan["key"])
    np.testing.assert_array_equal(sc["means"][:, 2].view(np.uint32), plan["key"])
    np.testing.assert_array_equal((bins["keys"] & np.uint64(0xffffffff)).astype(np.uint32), plan["key"][bins["point_list"]])
    # the oracle's lists = the plain statement of them
    exp = tl.expected_lists(plan["tile"], plan["key"], T)
    assert exp["R"] == ref["num_rendered"]
    np.testing.assert_array_equal(bins["ranges"], exp["ranges"])
    np.testing.assert_array_equal(bins["keys"], exp["keys"])
    np.testing.assert_array_equal(bins["point_list"], exp["point_list"])
    np.testing.assert_array_equal(bins["point_list"], np.lexsort((np.arange(P), plan["key"], plan["tile"])).astype(np.uint32))
    # ties and key span per tile, as designed
    pairs, span = tl.tile_stats(bins["keys"], bins["ranges"])
    for c in plan["cases"]:
        t = c["tile"]
        assert pairs[t] == c["pairs"], c
        assert span[t] >= c["lo"] and (c["hi"] is None or span[t] < c["hi"]), (c, span[t])


@pytest.mark.parametrize("pattern,count,bracket", [
    ("distinct-random", lambda n: 0, None), ("distinct-ascending", lambda n: 0, None), ("distinct-descending", lambda n: 0, None),
    ("all-equal", lambda n: max(n - 1, 0), "zero"), ("pairs-1", lambda n: 1, None), ("pairs-8", lambda n: 8, None), ("pairs-9", lambda n: 9, None),
    ("run-9", lambda n: 8, None), ("run-10", lambda n: 9, None), ("narrow", None, "narrow"), ("wide", lambda n: 0, "wide"),
    ("wide-low16-zero", lambda n: 0, "wide"),
])
def test_designed_counts_are_the_issue_s(pattern, count, bracket):
    """the plan's own figures (which the oracle's lists are held to above) against the numbers written here"""
    rng = np.random.default_rng(5)
    for n, _, where in tl.cases_of(pattern):
        d = tl.design(n, pattern, where, rng)
        if d is None:
            continue
        k = np.sort(d["keys"]).astype(np.int64)
        if count is not None:
            assert d["pairs"] == count(n), (pattern, n)
        assert int((k[1:] == k[:-1]).sum()) == d["pairs"]
        span = int(k[-1] - k[0]) if n else 0
        if bracket == "zero":
            assert (d["lo"], d["hi"]) == (0, 1) and span == 0
        elif bracket == "narrow":
            assert (d["lo"], d["hi"]) == (0, 16) and span < 16 and (n < 960 or np.unique(k).size == 16)
        elif bracket == "wide":
            assert d["lo"] == ((1 << 28) if n >= 2 else 0) and d["hi"] is None and span >= d["lo"]
        if pattern == "wide-low16-zero":
            assert not (k & 0xffff).any()
        if pattern == "distinct-ascending":
            assert (np.diff(d["keys"].astype(np.int64)) > 0).all()
        if pattern == "distinct-descending":
            assert (np.diff(d["keys"].astype(np.int64)) < 0).all()
        if pattern.startswith("pairs-"):
            pos = tl.pair_positions(n, d["pairs"])
            E = tl.lane_run(n)
            assert np.array_equal(np.nonzero(k[1:] == k[:-1])[0], pos)
            assert (3 if E == 2 and d["pairs"] >= 8 else E - 1) in pos and (d["pairs"] < 8 or (0 in pos and n - 2 in pos))
        if pattern.startswith("run-"):
            s = tl.run_position(n, d["pairs"] + 1, where)
            assert np.array_equal(np.nonzero(k[1:] == k[:-1])[0], np.arange(s, s + d["pairs"]))
