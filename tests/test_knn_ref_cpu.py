"""tests/knn_ref.py against the CPU oracle's k-NN (oracle/gs_oracle.c: orc_knn), and what its directed clouds are made of.  No GPU."""
import numpy as np
import pytest

import knn_ref


@pytest.mark.parametrize("P", [4, 5, 1025])
def test_brute_force_is_the_oracle_s(oracle32, oracle64, P):
    pts = knn_ref.cloud("gaussian", P)
    r32, r64 = knn_ref.mean_dist2_f32(pts), knn_ref.mean_dist2_f64(pts)
    assert r32.dtype == np.float32 and r64.dtype == np.float64
    # the same operations in the same order, every one rounded to float32 (the oracle is built without contraction): the same bits
    np.testing.assert_array_equal(r32, oracle32.knn(pts))
    np.testing.assert_array_equal(r64, oracle64.knn(pts))
    # float32 against float64: a difference carries 1 rounding, its square 1 more, the two sums 2, the mean 3 — under 6e-7 in all
    assert (np.abs(r32.astype(np.float64) - r64) <= 1e-6 * r64).all()


def test_self_is_excluded_by_index_not_by_value():
    pts = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3]], np.float32)
    for f, t in ((knn_ref.mean_dist2_f32, np.float32), (knn_ref.mean_dist2_f64, np.float64)):
        np.testing.assert_array_equal(f(pts), np.array([0 + 1 + 4, 0 + 1 + 4, 1 + 1 + 5, 4 + 4 + 5, 9 + 9 + 10], t) / t(3))


@pytest.mark.parametrize("P", knn_ref.SIZES)
def test_clouds_are_what_they_are_called(P):
    c = {k: knn_ref.cloud(k, P) for k in knn_ref.CLOUDS}
    assert all(v.shape == (P, 3) and v.dtype == np.float32 and np.isfinite(v).all() for v in c.values())
    g = c["gaussian"]
    assert P < 1023 or ((g.min(0) < 0).all() and (g.max(0) > 0).all())                    # straddles the origin on every axis
    assert (c["shifted-positive"] > 0).all() and (c["shifted-negative"] < 0).all()
    assert np.abs(c["shifted-positive"] - (g + np.array([100, 50, 20], np.float32))).max() < 1e-4
    assert (c["plane-z0"][:, 2] == 0).all() and (c["plane-z5"][:, 2] == 5).all() and (c["line-x"][:, 1:] == 0).all()
    count = lambda a: np.unique(a, axis=0, return_counts=True)[1]
    assert count(c["twice"]).min() >= 2 and count(c["four-times"]).min() >= 4 and count(g).max() == 1
    assert (knn_ref.mean_dist2_f32(c["four-times"]) == 0).all()
    x = c["two-clusters"][:, 0]
    n0 = int((x < 500).sum())
    assert n0 == 3 * P // 8 + 1 and (P < 1024 or (n0 % 1024 and (P - n0) % 1024)) and x[x >= 500].min() - x[x < 500].max() > 800
    lat = c["lattice"]
    assert (lat == np.round(lat)).all() and count(lat).max() == 1 and (P < 1023 or (knn_ref.mean_dist2_f32(lat) <= 2).all())
