"""The stratified per-Gaussian gradient check (tests/rowwise.py) itself, oracle only — no GPU: the fp32 oracle passes it, three mutants of
the fp32 oracle's gradients that the tensor-max-abs bar of 1e-4 accepts or barely notices are rejected, and the geometry of row_strata."""
import numpy as np
import pytest

import rowwise as rw
from conftest import rel_err

TOL = 1e-4     # the first bar
_cache = {}


def _case(name, oracle32, oracle64):
    if name not in _cache:
        from gaussian_lic_amd.synthetic import pixel_grad
        raw, sc, camd, cam, P, W, H = rw.build_case(name)
        dL = pixel_grad(H, W, seed=1).numpy()
        f32, f64 = oracle32.forward(sc, camd), oracle64.forward(sc, camd)
        vis = (f32["pre"]["radii"] > 0) & (f64["pre"]["radii"] > 0)
        _cache[name] = dict(sc=sc, camd=camd, P=P, raw={k: raw[k].numpy() for k in ("opacity", "scaling", "rotation")}, dL=dL, f32=f32, vis=vis, g32=oracle32.backward(sc, camd, f32, dL),
                            g64=oracle64.backward(sc, camd, f64, dL))
    return _cache[name]


def _failed_tensors(bad):
    return {line.split(":")[0].split()[-1].split(".")[0] for line in bad}


def test_factor_is_within_what_the_mutants_allow():
    assert 1 <= rw.FACTOR <= rw.MAX_FACTOR and 1 <= rw.FACTOR_FAST_MEDIAN <= rw.MAX_FACTOR


@pytest.mark.parametrize("name", list(rw.CASES))
def test_fp32_oracle_passes_and_uses_at_most_half_the_outlier_cap(oracle32, oracle64, name):
    """Self-check on every case of tests/test_rowwise_gradients_gpu.py: the yardstick passes its own bar, and the outlier cap is a condition
    the reference's arithmetic meets with a factor of two to spare — for the colour, the depth and the raw-parameter gradients."""
    import torch
    from test_depth_gpu import oracle_backward_depth
    c = _case(name, oracle32, oracle64)
    cmp = rw.assert_rowwise(c["g32"], c["g32"], c["g64"], c["vis"], c["P"], rw.FACTOR, what=name)
    print("\n" + rw.format_table(cmp, f"{name}: fp32 oracle against the fp64 oracle"))
    assert {label for label, _, _ in cmp} >= {"dL_dmean3D", "dL_dopacity", "dL_dscale"}
    H, W = c["dL"].shape[1:]
    gD = torch.randn(H, W, generator=torch.Generator().manual_seed(11)).float().numpy()
    f64 = oracle64.forward(c["sc"], c["camd"])
    d32, d64 = (oracle_backward_depth(o, c["sc"], c["camd"], f, c["dL"], gD) for o, f in ((oracle32, c["f32"]), (oracle64, f64)))
    r32, r64 = rw.raw_chain(c["g32"], c["raw"], np.float32), rw.raw_chain(c["g64"], c["raw"], np.float64)
    names = tuple(k for k in rw.GRADS if (name, k) not in rw.RAW_EXCLUDED)
    for path, cm in (("colour", cmp), ("depth", rw.compare(d32, d32, d64, c["vis"], c["P"])), ("raw", rw.compare(r32, r32, r64, c["vis"], c["P"], names))):
        for label, sg, _ in cm:
            assert sg["outliers"] <= 0.5 * rw.OUTLIER_SHARE * sg["rows"], (path, label, sg["outliers"], sg["rows"], rw.worst_rows(sg))


@pytest.mark.parametrize("name", rw.CPU_CASES)
def test_mutant_a_one_percent_below_1e3_of_max(oracle32, oracle64, name):
    """Every element below 1e-3 of its tensor's max-abs multiplied by 1.01: invisible to the first bar, rejected by the second."""
    c = _case(name, oracle32, oracle64)
    mut = {}
    for k in rw.GRADS:
        a = c["g32"][k].copy()
        small = np.abs(a) < 1e-3 * np.abs(a).max()
        a[small] *= a.dtype.type(1.01)
        mut[k] = a
        assert rel_err(a, c["g64"][k]) < TOL, k          # the point: the old bar accepts the mutant
    bad = rw.failures(rw.compare(mut, c["g32"], c["g64"], c["vis"], c["P"]), rw.FACTOR, what=name)
    assert _failed_tensors(bad) >= {"dL_dmean3D", "dL_dopacity", "dL_dsh", "dL_dscale"}, "\n".join(bad)


@pytest.mark.parametrize("name", rw.CPU_CASES)
def test_mutant_b_dropped_tail(oracle32, oracle64, name):
    """The fp32 oracle's backward with n_contrib clipped to 64 per pixel: every contribution after the first bucket of a list is lost.
    Both cases already fail the first bar (lists of several buckets carry large gradients too: see the printed figures), so only the second
    bar is asserted: every per-Gaussian tensor the blend feeds is rejected."""
    c = _case(name, oracle32, oracle64)
    f = dict(c["f32"])
    f["n_contrib"] = np.minimum(c["f32"]["n_contrib"], 64).astype(c["f32"]["n_contrib"].dtype)
    assert int((f["n_contrib"] != c["f32"]["n_contrib"]).sum()) > 0
    mut = oracle32.backward(c["sc"], c["camd"], f, c["dL"])
    print("\n" + name + " first bar on the dropped tail: " + "  ".join(f"{k} {rel_err(mut[k], c['g64'][k]):.1e}" for k in rw.GRADS if mut[k].size))
    bad = rw.failures(rw.compare(mut, c["g32"], c["g64"], c["vis"], c["P"]), rw.FACTOR, what=name)
    assert _failed_tensors(bad) >= {"dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmean3D", "dL_dcov3D", "dL_ddc", "dL_dsh", "dL_dscale", "dL_drot"}, "\n".join(bad)


@pytest.mark.parametrize("name", rw.CPU_CASES)
def test_mutant_c_lost_partial_rows(oracle32, oracle64, name):
    """The rows of 1 % of the visible Gaussians, chosen among those below 1e-2 of the tensor's max-abs, set to zero (a lost partial row):
    the quantiles do not move, the outlier cap catches it."""
    c = _case(name, oracle32, oracle64)
    P, vis = c["P"], c["vis"]
    rng = np.random.default_rng(0)
    mut, hit = {}, []
    for k in rw.GRADS:
        a = c["g32"][k].copy()
        s = rw.row_strata(a, c["g64"][k], vis, P)
        if s["rows"]:
            pool = s["idx"][s["scale"] < 1e-2 * s["tmax"]]
            n = int(round(0.01 * s["rows"]))
            if len(pool) >= n > 0:
                a.reshape(P, -1)[rng.choice(pool, n, replace=False)] = 0
                hit.append(k)
                assert rel_err(a, c["g64"][k]) <= 1e-2, k
        mut[k] = a
    assert set(hit) >= {"dL_dmean3D", "dL_dopacity", "dL_dsh", "dL_dscale"}
    bad = rw.failures(rw.compare(mut, c["g32"], c["g64"], vis, P), rw.FACTOR, what=name)
    capped = _failed_tensors([b for b in bad if "outlier cap" in b])
    assert capped >= set(hit), "\n".join(bad)


# ------------------------------------------------------------------------------------------------------------------ geometry of row_strata
def test_zero_rows_and_invisible_rows_are_left_out():
    P = 200
    ref = np.ones((P, 3))
    ref[:10] = 0                                   # zero rows
    vis = np.ones(P, bool)
    vis[10:30] = False
    got = ref * (1 + 1e-3)
    got[:30] = 7.0                                 # whatever stands in a zero or an invisible row does not count here
    s = rw.row_strata(got, ref, vis, P)
    assert s["rows"] == P - 30 and np.array_equal(s["idx"], np.arange(30, P))
    assert s["n"].tolist() == [P - 30] + [0] * 6   # a single stratum
    assert s["median"][0] == pytest.approx(1e-3) and s["p90"][0] == pytest.approx(1e-3) and s["outliers"] == 0
    assert np.isnan(s["median"][1])


def test_strata_are_decades_of_the_row_scale_clipped_at_six():
    P = 90
    scale = np.repeat(10.0 ** -np.arange(9), 10) * 0.5           # 0.5, 0.05, ... 0.5e-8: ten rows each
    ref = np.zeros((P, 2))
    ref[:, 1] = -scale
    ref[0, 0] = 1.0                                              # the tensor's max-abs
    s = rw.row_strata(ref * 1.5, ref, np.ones(P, bool), P)
    assert s["tmax"] == 1.0
    assert s["n"].tolist() == [10, 10, 10, 10, 10, 10, 30]
    assert np.allclose(s["err"], 0.5) and s["outliers"] == P
    # the row error is the row's max-abs difference over the row's max-abs reference
    s = rw.row_strata(np.array([[1.0, 0.1 + 0.3]]), np.array([[1.0, 0.1]]), np.ones(1, bool), 1)
    assert s["err"][0] == pytest.approx(0.3)


@pytest.mark.parametrize("M", [0, 3, 8, 15])
def test_sh_rows_split_by_band(M):
    P = 60
    rng = np.random.default_rng(M)
    a = rng.standard_normal((P, M, 3))
    v = rw.views("dL_dsh", a, P)
    want = {0: [], 3: ["band1"], 8: ["band1", "band2"], 15: ["band1", "band2", "band3"]}[M]
    assert [label for label, _ in v] == ["dL_dsh"] + ["dL_dsh." + b for b in want]
    assert [x.shape[1] for _, x in v[1:]] == [9, 15, 21][:len(want)]
    if M == 15:
        np.testing.assert_array_equal(v[2][1], a[:, 3:8].reshape(P, -1))
    # a band that is small next to band 1 is judged on its own scale: an error confined to band 3 disappears in the whole row, not in its band
    if M == 15:
        ref = a.copy()
        ref[:, 8:] *= 1e-4
        got = ref.copy()
        got[:, 8:] *= 1.5
        cmp = dict((label, sg) for label, sg, _ in rw.compare({"dL_dsh": got}, {"dL_dsh": ref}, {"dL_dsh": ref}, np.ones(P, bool), P, names=("dL_dsh",)))
        assert cmp["dL_dsh"]["err"].max() < 1e-3 and cmp["dL_dsh.band3"]["err"].min() == pytest.approx(0.5)
    assert rw.views("dL_dmean3D", np.zeros((P, 3)), P)[0][1].shape == (P, 3) and len(rw.views("dL_dmean3D", np.zeros((P, 3)), P)) == 1


def test_all_zero_and_empty_references_are_skipped():
    P = 100
    z = np.zeros((P, 4))
    s = rw.row_strata(np.ones((P, 4)), z, np.ones(P, bool), P)
    assert s["rows"] == 0 and s["n"].sum() == 0
    got = {"dL_drot": np.ones((P, 4)), "dL_dsh": np.zeros((P, 0, 3)), "dL_dopacity": np.ones((P, 1))}
    ref = {"dL_drot": z, "dL_dsh": np.zeros((P, 0, 3)), "dL_dopacity": np.ones((P, 1))}
    cmp = rw.assert_rowwise(got, ref, ref, np.ones(P, bool), P, rw.FACTOR, names=("dL_drot", "dL_dsh", "dL_dopacity"))
    assert [label for label, _, _ in cmp] == ["dL_dopacity"]
    assert "dL_dopacity" in rw.format_table(cmp) and rw.worst_line(cmp).startswith("dL_dopacity")


def test_small_strata_are_reported_not_judged_and_the_message_names_everything():
    P = 400
    ref = np.ones((P, 1))
    ref[:40] = 1e-3                                # 40 rows in stratum 3: below MIN_ROWS
    got = ref.copy()
    got[:40] *= 1.05                               # wrong by 5 %, under the outlier threshold, in a stratum that is not judged
    r = {"x": ref}
    assert rw.failures(rw.compare({"x": got}, r, r, np.ones(P, bool), P, names=("x",)), rw.FACTOR) == []
    ref[:60] = 1e-3
    got = ref.copy()
    got[:60] *= 1.05
    bad = rw.failures(rw.compare({"x": got}, r, r, np.ones(P, bool), P, names=("x",)), rw.FACTOR, what="case")
    assert len(bad) == 2 and all("case x: stratum 1e-3 of max (60 rows)" in b for b in bad)
    assert "median 5.000e-02" in bad[0] and "p90" in bad[1]
    with pytest.raises(AssertionError, match="stratum 1e-3"):
        rw.assert_rowwise({"x": got}, r, r, np.ones(P, bool), P, rw.FACTOR, names=("x",))
    # NaN never passes
    got[0] = np.nan
    got[60:] = np.nan
    assert rw.failures(rw.compare({"x": got}, r, r, np.ones(P, bool), P, names=("x",)), rw.FACTOR)


def test_raw_chain_matches_autograd():
    import torch
    rng = np.random.default_rng(3)
    P = 50
    raw = dict(opacity=rng.standard_normal((P, 1)) * 2, scaling=rng.standard_normal((P, 3)), rotation=rng.standard_normal((P, 4)))
    g = dict(dL_dopacity=rng.standard_normal((P, 1)), dL_dscale=rng.standard_normal((P, 3)), dL_drot=rng.standard_normal((P, 4)))
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in raw.items()}
    loss = ((torch.sigmoid(t["opacity"]) * torch.tensor(g["dL_dopacity"])).sum() + (torch.exp(t["scaling"]) * torch.tensor(g["dL_dscale"])).sum()
            + (torch.nn.functional.normalize(t["rotation"]) * torch.tensor(g["dL_drot"])).sum())
    loss.backward()
    out = rw.raw_chain(g, raw, np.float64)
    for k, n in (("dL_dopacity", "opacity"), ("dL_dscale", "scaling"), ("dL_drot", "rotation")):
        np.testing.assert_allclose(out[k], t[n].grad.numpy(), rtol=1e-12, atol=1e-14)
    assert rw.raw_chain({k: v.astype(np.float32) for k, v in g.items()}, raw, np.float32)["dL_drot"].dtype == np.float32
