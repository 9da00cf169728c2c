"""-m gpu: the C++ host (gslic::FusedStep, shim/include/gslic_fused.h) carrying BOTH statistics objects at once — a gslic::ContributionStats with its
error and free-space arrays and the attached gslic::GradientStats — through all four row changes (densify, extend, prune, resort), held against the
Python model with a trainer.ContributionStats and a trainer.GradientStats attached.  What the single-feature C++-host tests leave out: gradient
statistics through extend(), the free-space arrays through densify(), and the two objects side by side.  Every comparison is on the bits."""
import functools

import numpy as np
import pytest
import torch

import fused_check_io as fio
import gradstats_ref as gr

pytestmark = pytest.mark.gpu


def _flat_bits(t):   # (detached, on the host and flat, as fio.read gives the files: not gpu_helpers.bits, which keeps device and shape)
    return t.detach().contiguous().view(torch.int32).cpu().reshape(-1)


def test_fused_rows_cpp_host(tmp_path, monkeypatch):
    """shim/fused_rows_check.cpp and this function run the same scenario on a 600-row map that starts in insertion order, 2 steps between events:
    gradient statistics attached, steps; one view accumulated with an error image and one with a near-bound image; densify by the gradient grow mask
    (split scale at the median) with the contribution statistics, steps; the first sort and the re-sort fraction, then extend() with a LiDAR frame
    whose tail passes the fraction (the rule re-sorts), steps; one more free-space view; prune by big_mask; resort, steps.  The 19 row arrays, the six
    contribution arrays and the three gradient arrays over [0, size()), the three permutations and the printed counts agree bit for bit."""
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.rasterizer import render
    from gaussian_lic_amd.synthetic import gt_image, lidar_scene
    exe = fio.build("fused_rows")
    monkeypatch.delenv("GSLIC_RESORT", raising=False)
    dev = torch.device("cuda:0")
    W, H, P0, iters, seed, fraction, n_pts, w_min = gr.W, gr.H, 600, 2, 11, 0.05, 400, trainer.ContributionStats.W_MIN
    cam = synthetic_camera(W, H).to_device(dev)
    gt, bg = gt_image(H, W, seed=5).to(dev), torch.zeros(3, device=dev)
    m = trainer.GaussianModel(gr.scene(P0, 3), dev)
    m.training_setup()
    d = str(tmp_path)
    # the LiDAR frame inputs of tests/test_resort_gpu.py
    frame = lidar_scene(n_pts, W, H, sh_degree=3, seed=77)
    pts, rsp = frame["xyz"].to(dev), frame["xyz"][:, 2].contiguous().to(dev)
    col = (frame["features_dc"].reshape(-1, 3) * 0.28209479177387814 + 0.5).to(dev)
    Rcw, tcw = torch.from_numpy(cam.world_view_transform[:3, :3].T.copy()), torch.from_numpy(cam.world_view_transform[3, :3].copy())
    intr = (float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy))
    g = torch.Generator().manual_seed(7)                                # a bound image that splits the map's depth range, a quarter unmeasured
    near = 1.0 + 29.0 * torch.rand(H, W, generator=g)
    near[torch.rand(H, W, generator=g) < 0.25] = 0.0
    near = near.to(dev)
    fio.write_inputs(d, m, cam, scalars_extra=intr, gt=gt, pts=pts, col=col, rsp=rsp, Rcw=Rcw, tcw=tcw, near=near)

    gst = trainer.GradientStats(m)

    def steps():
        for _ in range(iters):
            trainer.training_step_fused(m, cam, gt, bg, grad_stats=gst)
    steps()
    with torch.no_grad():
        err = (render(cam, m, bg)[0] - gt).abs().mean(0).contiguous()
    fio.write(d, "err", err)
    st = trainer.ContributionStats(m)
    st.accumulate(cam, w_min=w_min, error=err)
    st.accumulate(cam, w_min=w_min, free_space=near)
    # thresholds from the model's own statistics: about half of the seen rows grow, about half of those split
    grad_above = float(np.float32(gst.mean_gradient()[gst.n_seen() > 0].median().item()))
    split_scale = float(torch.exp(m.scaling.detach().double()).max(1).values.median())
    k, n_split, _parents = m.densify(gst.grow_mask(grad_above), split_scale, seed=seed)
    print(f"[fused rows] densify: {k} new rows, {n_split} from splits")
    assert 0 < n_split < k < P0
    steps()
    perm0 = m.to_morton_order(resort_fraction=fraction)                 # the first sort, from insertion order: from here on the re-sort rule applies
    seen, resort = [], m.resort
    m.resort = lambda: seen.append(resort()) or seen[-1]                # (extend() does not return the permutation of the re-sort it triggers)
    k2 = m.extend(cam, pts, col, rsp, Rcw, tcw, intr)
    del m.resort
    print(f"[fused rows] extend: {k2} rows inserted into {P0 + k}, re-sorts {len(seen)}")
    assert k2 > fraction * (P0 + k + k2) and len(seen) == 1 and m._sorted_P == m.P == P0 + k + k2           # the rule re-sorted, once
    steps()
    st.accumulate(cam, w_min=w_min, free_space=near)
    rlim = int(gst.max_radius()[gst.n_seen() > 0].float().median())     # about half of the seen rows are "big"
    removed, _kept = m.prune(drop=gst.big_mask(rlim))
    print(f"[fused rows] prune: {removed} rows removed, {m.P} left")
    assert 0 < removed and m.P > 0
    perm2 = m.resort()
    steps()
    P = m.P
    assert bool(st.free_fixed().any()) and bool(st.error_fixed().any()) and st.views == 3
    assert int(gst.n_seen().max()) == 4 * iters                         # a row of the initial map that every step saw and no event reset

    r = fio.run(exe, d, str(P0), str(W), str(H), "3", str(iters), str(n_pts), repr(fraction), repr(w_min), repr(grad_above), repr(split_scale),
                str(seed), str(rlim))
    assert f"rows densified {k} splits {n_split} extended {k2} resorts 2 pruned {removed} size {P} views 3" in r.stdout, r.stdout[-500:]
    torch.cuda.synchronize()
    rd = functools.partial(fio.read, d)
    for n, f in (("xyz", "xyz"), ("features_dc", "dc"), ("features_rest", "rest"), ("opacity", "opacity"), ("scaling", "scaling"), ("rotation", "rotation")):
        for pre, src in (("", m._buf), ("m_", m._m), ("v_", m._v)):
            assert torch.equal(rd(pre + f + ".f32", np.int32), _flat_bits(src[n][:P])), pre + f
    assert torch.equal(rd("tie.i32", np.int32), m.tie_rank.cpu())
    assert torch.equal(rd("max_w.i32", np.int32), st._max[:P].cpu()) and torch.equal(rd("n_pix.i32", np.int32), st._npix[:P].cpu())
    assert torch.equal(rd("sum_w.i64", np.int64), st.sum_fixed().cpu()) and torch.equal(rd("err_sum.i64", np.int64), st.error_fixed().cpu())
    assert torch.equal(rd("free_sum.i64", np.int64), st.free_fixed().cpu()) and torch.equal(rd("meas_sum.i64", np.int64), st.measured_fixed().cpu())
    assert torch.equal(rd("grad_sum.f32", np.int32), _flat_bits(gst.grad_sum())) and bool((gst.grad_sum() > 0).any())
    assert torch.equal(rd("n_seen.i32", np.int32), gst._seen_n[:P].cpu()) and torch.equal(rd("max_radius.i32", np.int32), gst.max_radius().cpu())
    assert torch.equal(rd("perm0.i64", np.int64), perm0.cpu()) and perm0.numel() == P0 + k
    assert torch.equal(rd("perm1.i64", np.int64), seen[0].cpu()) and seen[0].numel() == P0 + k + k2
    assert torch.equal(rd("perm2.i64", np.int64), perm2.cpu()) and perm2.numel() == P
