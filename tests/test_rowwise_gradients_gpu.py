"""-m gpu: the backward kernels' per-Gaussian gradients under the stratified row-wise bar of tests/rowwise.py (second bar).

Every other gradient comparison of the suite divides by the tensor's max-abs and so cannot see the faint, far, late-in-the-list and
border Gaussians — a third to a half of the rows.  Here each row is measured against its own magnitude, by decade of magnitude, and held
against the fp32 oracle's own error in the same decade (both against the fp64 oracle).  Paths: gslic_rasterize_backward and
gslic_rasterize_backward_depth in both arithmetic modes, and the raw-parameter path (activations inside the kernels) that bench.py times.
tests/rowwise_report.py prints the same comparisons as the table committed in profiles/rowwise_gradient_strata.txt."""
import numpy as np
import pytest
import torch

import rowwise as rw
from test_depth_gpu import POSE, _mode, bwd, fwd_depth, fwd_plain, oracle_backward_depth

pytestmark = pytest.mark.gpu

PATHS = ("colour-strict", "colour-fast", "depth-strict", "depth-fast", "raw-strict")
_refs = {}


def references(name, oracle32, oracle64):
    """Scene, upstream gradients and both oracles' forward / colour backward of one case (kept for the module: five paths share them)."""
    if name not in _refs:
        from gaussian_lic_amd.synthetic import pixel_grad
        assert rw.POSE == POSE
        raw, sc, camd, cam, P, W, H = rw.build_case(name)
        dL = pixel_grad(H, W, seed=1)
        gD = torch.randn(H, W, generator=torch.Generator().manual_seed(11)).float()    # pixel_grad-like noise of the depth image's shape
        f32, f64 = oracle32.forward(sc, camd), oracle64.forward(sc, camd)
        _refs[name] = dict(raw=raw, sc=sc, camd=camd, cam=cam, P=P, dL=dL, gD=gD, f32=f32, f64=f64,
                           vis=(f32["pre"]["radii"] > 0) & (f64["pre"]["radii"] > 0),
                           g32=oracle32.backward(sc, camd, f32, dL.numpy()), g64=oracle64.backward(sc, camd, f64, dL.numpy()))
    return _refs[name]


def run_path(name, path, oracle32, oracle64):
    """One case through one path: dict(cmp = comparison against the fp64 oracle with the fp32 oracle as yardstick, cmp32 = the same rows against
    the fp32 oracle directly (strict colour only, informative), got, n_contrib_mismatch (strict colour only), names, strict)."""
    from gpu_helpers import hip_backward, hip_forward, npy
    c = references(name, oracle32, oracle64)
    kind, strict = path.split("-")[0], path.endswith("strict")
    raw, cam, P, dL, gD = c["raw"], c["cam"], c["P"], c["dL"], c["gD"]
    out = dict(strict=strict, names=rw.GRADS)
    if kind == "colour":
        with _mode(strict):
            f = hip_forward(raw, cam, export=("n_contrib",))
            got = hip_backward(f, dL)
        ref32, ref64 = c["g32"], c["g64"]
        if strict:
            out["n_contrib_mismatch"] = int((npy(f["dbg"]["n_contrib"]).astype(np.int64) != c["f32"]["n_contrib"].astype(np.int64)).sum())
            out["cmp32"] = rw.compare(got, ref32, ref32, c["vis"], P)
    elif kind == "depth":
        with _mode(strict):
            got = bwd(fwd_depth(raw, cam), dL, gD)
        if "d32" not in c:
            c["d32"], c["d64"] = (oracle_backward_depth(o, c["sc"], c["camd"], f, dL.numpy(), gD.numpy())
                                  for o, f in ((oracle32, c["f32"]), (oracle64, c["f64"])))
        ref32, ref64 = c["d32"], c["d64"]
    else:
        with _mode(True):
            got = bwd(fwd_plain(raw, cam, raw_params=True), dL)
        rawnp = {k: raw[k].numpy() for k in ("opacity", "scaling", "rotation")}
        ref32, ref64 = rw.raw_chain(c["g32"], rawnp, np.float32), rw.raw_chain(c["g64"], rawnp, np.float64)
        out["names"] = tuple(k for k in rw.GRADS if (name, k) not in rw.RAW_EXCLUDED)
    out["got"], out["cmp"] = got, rw.compare(got, ref32, ref64, c["vis"], P, out["names"])
    return out


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(rw.CASES))
def test_rowwise_gradients(oracle32, oracle64, name, path):
    r = run_path(name, path, oracle32, oracle64)
    c = references(name, oracle32, oracle64)
    print("\n" + rw.format_table(r["cmp"], f"{name} {path}: HIP and the fp32 oracle against the fp64 oracle"))
    print("worst judged ratio: " + rw.worst_line(r["cmp"]))
    labels = {label for label, _, _ in r["cmp"]}
    assert labels >= {"dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmean3D", "dL_dcov3D", "dL_dscale"}, labels
    if c["sc"]["shs"].size:     # (M = 0: the reference skips the whole SH backward, backward.cu:352 — dL_ddc is all zero there and skipped by rule)
        assert labels >= {"dL_ddc", "dL_dsh", "dL_dsh.band1"}, labels
    if "cmp32" in r:
        print(rw.format_table(r["cmp32"], f"{name} {path}: HIP against the fp32 oracle directly (informative: summation order only; ratios are to the 4-ulp floor)"))
        print(f"n_contrib differs from the fp32 oracle's in {r['n_contrib_mismatch']} pixels")
        assert r["n_contrib_mismatch"] == 0      # cut decisions are shared with the yardstick
    if r["strict"]:
        bad = rw.failures(r["cmp"], rw.FACTOR, what=f"{name} {path}")
    else:
        # fast arithmetic: medians only — threshold flips live in the tails (p90 and the outlier share are in the table above); the cap holds
        bad = rw.failures(r["cmp"], rw.FACTOR_FAST_MEDIAN, quantiles=("median",), what=f"{name} {path}")
    for label, sg, _ in r["cmp"]:
        if any(b.split(":")[0].endswith(" " + label) for b in bad):
            print(f"worst rows of {label} (Gaussian id, row scale / max, rel err): {rw.worst_rows(sg, 8)}")
    assert not bad, "\n".join(bad)
    if path == "raw-strict":
        for case, k in rw.RAW_EXCLUDED:
            if case == name:
                # the excluded tensor: mathematically zero rows, held to zero within the first bar's measure for this tensor (the magnitude of the
                # cancelling terms, as tests/test_parity_gpu.py takes it), through the 1 / |q| of the normalisation's backward
                q = np.linalg.norm(c["raw"]["rotation"].numpy().astype(np.float64), axis=1)
                scale = max(float(np.abs(c["g64"]["dL_drot"]).max()), float(np.abs(c["g64"]["dL_dscale"]).max() * c["sc"]["scales"].max())) / float(q.min())
                e = float(np.abs(r["got"][k]).max()) / scale
                print(f"{name} {k} (excluded by name, reference mathematically zero): max |got| = {e:.2e} of the cancelling terms")
                assert e < 1e-4, (k, e)
