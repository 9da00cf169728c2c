"""-m gpu: the C++ LibTorch shim (reference L2 signatures) and the reference's own host code on top of it."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import fused_check_io as fio
from conftest import make_scene, rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "gaussian-lic_amd", "libgslic_torch_shim.so")
CHECK = os.path.join(ROOT, "gaussian-lic_amd", "dropin_check")
CHECK_GROUPS = os.path.join(ROOT, "gaussian-lic_amd", "dropin_check_groups")
CHECK_DIST = os.path.join(ROOT, "gaussian-lic_amd", "dropin_check_dist")
CHECK_FUSED = os.path.join(ROOT, "gaussian-lic_amd", "fused_check")


def _load_shim():
    if not os.path.exists(SHIM):
        pytest.skip("libgslic_torch_shim.so not built")
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    _lib.lib()
    torch.ops.load_library(SHIM)


def test_shim_ops_equal_ctypes_path():
    """torch.ops.gslic.* (C++ shim, reference signatures) gives bit-identical results to the Python front-end."""
    _load_shim()
    from gpu_helpers import hip_backward, hip_forward, settings_from
    from gaussian_lic_amd.synthetic import activate, pixel_grad
    raw, sc, camd, cam = make_scene("random", 20000, 320, 240, 3, 31)
    dev = torch.device("cuda:0")
    act = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in activate(raw).items()}
    rs = settings_from(cam, 3, dev)
    e = torch.empty(0, device=dev)
    R, B, color, final_T, radii, geom, binning, img, sample = torch.ops.gslic.RasterizeGaussiansCUDA(
        rs.bg, act["means"], e, act["opac"], act["scales"], act["rots"], 1.0, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy,
        rs.image_height, rs.image_width, rs.limx_neg, rs.limx_pos, rs.limy_neg, rs.limy_pos, act["dc"], act["shs"], 3, rs.campos, False,
        False, False)
    ref = hip_forward(raw, cam)
    assert (R, B) == (ref["R"], ref["B"])
    assert torch.equal(color, ref["color"]) and torch.equal(final_T, ref["final_T"]) and torch.equal(radii, ref["radii"])
    dL = pixel_grad(240, 320).to(dev)
    g = torch.ops.gslic.RasterizeGaussiansBackwardCUDA(
        rs.bg, act["means"], radii, e, act["scales"], act["rots"], 1.0, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy,
        rs.limx_neg, rs.limx_pos, rs.limy_neg, rs.limy_pos, dL, act["dc"], act["shs"], 3, rs.campos, geom, R, binning, img, B, sample,
        0.0, False)
    gref = hip_backward(ref, dL)
    names = ["dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmean3D", "dL_dcov3D", "dL_ddc", "dL_dsh", "dL_dscale", "dL_drot"]
    for n, t in zip(names, g):
        np.testing.assert_array_equal(t.cpu().numpy(), gref[n])
    with pytest.raises(RuntimeError, match="means3D must have dimensions"):   # rasterize_points.cu:77-80
        torch.ops.gslic.RasterizeGaussiansCUDA(rs.bg, act["means"].reshape(-1), e, act["opac"], act["scales"], act["rots"], 1.0, e,
                                               rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, 240, 320, -1.0, 1.0, -1.0, 1.0,
                                               act["dc"], act["shs"], 3, rs.campos, False, False, False)
    d = torch.ops.gslic.distCUDA2(act["means"])
    from gaussian_lic_amd import knn
    assert torch.equal(d, knn.distCUDA2(act["means"]))


def test_reference_host_code_drives_the_hip_kernels(tmp_path):
    """dropin_check = the reference's rasterizer.cpp / loss_utils.h / optim_utils.h (compiled unmodified) running three
    iterations of the optimize() loop body on our kernels; must agree with the Python mirror of the same loop."""
    if not os.path.exists(CHECK):
        pytest.skip("dropin_check not built (needs /root/reference at build time)")
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.synthetic import gt_image
    P, W, H, iters = 30000, 320, 240, 3
    raw, sc, camd, cam = make_scene("random", P, W, H, 3, 41)
    d = str(tmp_path)
    gt = gt_image(H, W)
    fio.write_inputs(d, raw, cam, gt=gt)
    fio.run(CHECK, d, str(P), str(W), str(H), "3", str(iters))
    dev = torch.device("cuda:0")
    model = trainer.GaussianModel(raw, dev)
    model.training_setup()
    cam.to_device(dev)
    bg = torch.zeros(3, device=dev)
    for _ in range(iters):
        trainer.training_step(model, cam, gt.to(dev), bg, raw_render=False)   # (the C++ program runs renderer.cpp as written)
    rd = lambda name, shape: fio.read(d, name + ".f32", np.float32).numpy().reshape(shape)
    for name, t in (("xyz", model.xyz), ("scaling", model.scaling), ("rotation", model.rotation), ("opacity", model.opacity),
                    ("dc", model.features_dc), ("rest", model.features_rest)):
        got = rd(name, tuple(t.shape))
        assert rel_err(got, t.detach().cpu().numpy()) < 1e-5, name
    # the same program compiled against this repo's optim_utils.h (one Adam launch per step through adamUpdateGroups, no
    # grad.clone()) instead of the reference's (six adamUpdate launches): bit-identical parameters and image
    if os.path.exists(CHECK_GROUPS):
        first = {n: rd(n, (-1,)).copy() for n in ("image", "xyz", "scaling", "rotation", "opacity", "dc", "rest")}
        fio.run(CHECK_GROUPS, d, str(P), str(W), str(H), "3", str(iters))
        for n, a in first.items():
            np.testing.assert_array_equal(rd(n, (-1,)), a, err_msg=n)
        # and with the N > 1 exchange step compiled in (shim/include/gslic_dist.h: c10d ProcessGroupNCCL = RCCL, all-reduce of the
        # gradients and of the visibility mask between loss.backward() and step(), gaussian.cpp:697-707) in a group of ONE rank: the
        # sums are the identity, dense and visible-rows-only alike, so the outputs stay bit-identical
        if os.path.exists(CHECK_DIST):
            for sparse, port in (("0", "29601"), ("1", "29603")):
                env = dict(os.environ, RANK="0", WORLD_SIZE="1", MASTER_PORT=port, GSLIC_SPARSE_EXCHANGE=sparse, HSA_ENABLE_IPC_MODE_LEGACY="0")
                fio.run(CHECK_DIST, d, str(P), str(W), str(H), "3", str(iters), env=env)
                for n, a in first.items():
                    np.testing.assert_array_equal(rd(n, (-1,)), a, err_msg=f"{n} (dist, sparse={sparse})")
            # rank-1 exchange (gslic_dist.h exchange_gradients_rank1: 11 floats all-reduced, dL_ddc all-gathered, dL_ddc / dL_dsh rebuilt by
            # gslic_sh_grad_from_rgb from what was gathered): this host ships dL_ddc, so dRGB is recovered to 1 ulp — not bit-identical to the
            # autograd rows it replaces, equal to fp32 rounding (Adam's normalised update turns a last-bit change of a near-zero gradient into a
            # visible change of that element's step, hence 1e-4 of max-abs after three steps rather than 1e-6)
            env = dict(os.environ, RANK="0", WORLD_SIZE="1", MASTER_PORT="29605", GSLIC_EXCHANGE="rank1", HSA_ENABLE_IPC_MODE_LEGACY="0")
            fio.run(CHECK_DIST, d, str(P), str(W), str(H), "3", str(iters), env=env)
            for n, a in first.items():
                assert rel_err(rd(n, (-1,)), a) < 1e-4, f"{n} (dist, rank1)"


@pytest.mark.parametrize("deg", [3, 0])
def test_fused_cpp_host(tmp_path, deg):
    """fused_check = the fused training step written in C++ against the C-ABI (shim/include/gslic_fused.h: raw-parameter forward, loss
    kernels, backward with the Adam update inside; no autograd graph).  It issues the same C-ABI calls as trainer.training_step_fused,
    so image and parameters after four steps are bit-identical to the Python host's; SH degree 0 exercises the empty features_rest group."""
    if not os.path.exists(CHECK_FUSED):
        pytest.skip("fused_check not built")
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.synthetic import gt_image
    P, W, H, iters = 30000, 320, 240, 4
    raw, sc, camd, cam = make_scene("random", P, W, H, deg, 43)
    d = str(tmp_path)
    gt = gt_image(H, W)
    fio.write_inputs(d, raw, cam, gt=gt)
    r = fio.run(CHECK_FUSED, d, str(P), str(W), str(H), str(deg), str(iters))
    dev = torch.device("cuda:0")
    model = trainer.GaussianModel(raw, dev)
    model.training_setup()
    cam.to_device(dev)
    bg = torch.zeros(3, device=dev)
    losses = []
    for _ in range(iters):
        terms, _vis = trainer.training_step_fused(model, cam, gt.to(dev), bg)
        losses.append(float(0.8 * terms[0] + 0.2 * (1.0 - terms[1])))
    rd = lambda name, shape: fio.read(d, name + ".f32", np.float32).numpy().reshape(shape)
    names = [("xyz", model.xyz), ("scaling", model.scaling), ("rotation", model.rotation), ("opacity", model.opacity), ("dc", model.features_dc)]
    if deg > 0:
        names.append(("rest", model.features_rest))
    for name, t in names:
        np.testing.assert_array_equal(rd(name, tuple(t.shape)), t.detach().cpu().numpy(), err_msg=name)
    printed = [float(l.split()[3]) for l in r.stdout.splitlines() if l.startswith("iter ")]
    assert len(printed) == iters and np.allclose(printed, losses, rtol=1e-5)


def test_fused_cpp_host_extend(tmp_path):
    """extend() from C++ (gslic::FusedStep::extend: transmittance render, device-side point selection, in-place append with capacity
    doubling, zero moments) inside the fused training loop — three steps, one LiDAR frame appended, three more steps — against the
    Python host doing the same (trainer.GaussianModel.extend + training_step_fused): same number of Gaussians inserted, bit-identical
    parameters afterwards."""
    if not os.path.exists(CHECK_FUSED):
        pytest.skip("fused_check not built")
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.synthetic import gt_image, lidar_scene
    P, W, H, iters, deg = 20000, 320, 240, 3, 3
    raw, sc, camd, cam = make_scene("random", P, W, H, deg, 47)
    u_pix = raw["xyz"][:, 0] * (0.675 * W) / raw["xyz"][:, 2].abs().clamp_min(0.2) + 0.4857 * W     # leave the right 30 % of the image uncovered
    keep = u_pix < 0.7 * W
    raw = {k: (v[keep].contiguous() if torch.is_tensor(v) else v) for k, v in raw.items()}
    P = int(raw["xyz"].shape[0])
    d = str(tmp_path)
    gt = gt_image(H, W)
    frame = lidar_scene(4000, W, H, sh_degree=3, seed=101)
    f_pts = frame["xyz"].contiguous()
    f_col = (frame["features_dc"].reshape(-1, 3) * 0.28209479177387814 + 0.5).contiguous()
    f_rsp = frame["xyz"][:, 2].contiguous()
    Rcw = np.ascontiguousarray(cam.world_view_transform[:3, :3].T, np.float32)
    tcw = np.ascontiguousarray(cam.world_view_transform[3, :3], np.float32)
    intr = np.array([cam.fx, cam.fy, cam.cx, cam.cy], np.float32)
    fio.write_inputs(d, raw, cam, gt=gt, frame_pts=f_pts, frame_col=f_col, frame_rsp=f_rsp,
                     frame_pose=np.concatenate([Rcw.reshape(-1), tcw.reshape(-1), intr]), frame_n=np.array([f_pts.shape[0]], np.float32))
    r = fio.run(CHECK_FUSED, d, str(P), str(W), str(H), str(deg), str(iters))
    ins = [l for l in r.stdout.splitlines() if l.startswith("extend inserted")]
    assert ins, r.stdout[-1000:]
    k_cpp, size_cpp = int(ins[0].split()[2]), int(ins[0].split()[4])
    dev = torch.device("cuda:0")
    model = trainer.GaussianModel(raw, dev)
    model.training_setup()
    cam.to_device(dev)
    bg = torch.zeros(3, device=dev)
    for _ in range(iters):
        trainer.training_step_fused(model, cam, gt.to(dev), bg)
    k_py = model.extend(cam, f_pts.to(dev), f_col.to(dev), f_rsp.to(dev), torch.from_numpy(Rcw), torch.from_numpy(tcw), tuple(float(v) for v in intr))
    for _ in range(iters):
        trainer.training_step_fused(model, cam, gt.to(dev), bg)
    assert k_cpp == k_py and k_py > 100 and size_cpp == model.P
    rd = lambda name, shape: fio.read(d, name + ".f32", np.float32).numpy().reshape(shape)
    for name, t in (("xyz", model.xyz), ("scaling", model.scaling), ("rotation", model.rotation), ("opacity", model.opacity),
                    ("dc", model.features_dc), ("rest", model.features_rest)):
        np.testing.assert_array_equal(rd(name, tuple(t.shape)), t.detach().cpu().numpy(), err_msg=name)


def test_shim_adam_rejects_noncontiguous_state():
    """adamUpdate works in place on param / exp_avg / exp_avg_sq: a strided view must be refused, not silently updated in a temporary
    copy (the reference takes data_ptr of whatever it is given, rasterize_points.cu:262-272)."""
    _load_shim()
    dev = torch.device("cuda:0")
    N, M = 64, 3
    base = torch.randn(N, 2 * M, device=dev)
    param = base[:, :M]                       # non-contiguous view
    g, m, v = torch.randn(N, M, device=dev), torch.zeros(N, M, device=dev), torch.zeros(N, M, device=dev)
    vis = torch.ones(N, dtype=torch.bool, device=dev)
    with pytest.raises(RuntimeError, match="must be contiguous"):
        torch.ops.gslic.adamUpdate(param, g, m, v, vis, 1e-3, 0.9, 0.999, 1e-15, N, M)
    # a non-contiguous GRADIENT is only read: accepted, same result as its contiguous copy
    p1, p2 = torch.randn(N, M, device=dev), None
    p2 = p1.clone()
    gbase = torch.randn(N, 2 * M, device=dev)
    m1, v1, m2, v2 = (torch.zeros(N, M, device=dev) for _ in range(4))
    torch.ops.gslic.adamUpdate(p1, gbase[:, :M], m1, v1, vis, 1e-3, 0.9, 0.999, 1e-15, N, M)
    torch.ops.gslic.adamUpdate(p2, gbase[:, :M].contiguous(), m2, v2, vis, 1e-3, 0.9, 0.999, 1e-15, N, M)
    assert torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(v1, v2)


def test_reference_host_two_ranks_rccl(tmp_path):
    """The reference's C++ host loop with the exchange step on TWO GPUs (one process per GPU over RCCL, rank k renders view k): the
    parameters after three steps equal a single-process restatement (gradients of the two views summed, masks OR-ed, one Adam).
    Skipped on a one-GPU box."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    if not os.path.exists(CHECK_DIST):
        pytest.skip("dropin_check_dist not built (needs /root/reference at build time)")
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import gt_image
    P, W, H, iters = 30000, 320, 240, 3
    raw, sc, camd, cam = make_scene("random", P, W, H, 3, 41)
    d = str(tmp_path)
    w = functools.partial(fio.write, d)   # (per-rank files view_<k> / gt_<k> and no untagged camera: not fio.write_inputs' layout)
    for k, n in fio.GROUPS:
        w(n, raw[k])
    cams, gts = [synthetic_camera(W, H, k) for k in range(2)], [gt_image(H, W, seed=2 + k) for k in range(2)]
    for k in range(2):
        w(f"view_{k}", cams[k].world_view_transform); w(f"proj_{k}", cams[k].full_proj_transform); w(f"campos_{k}", cams[k].camera_center)
        w(f"gt_{k}", gts[k].numpy())
    w("scalars", np.array([cam.tanfovx, cam.tanfovy, cam.limx_neg, cam.limx_pos, cam.limy_neg, cam.limy_pos], np.float32))
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", MASTER_PORT="29611", HIP_VISIBLE_DEVICES=str(rank), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([CHECK_DIST, d, str(P), str(W), str(H), "3", str(iters)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    for p in procs:
        so, se = p.communicate(timeout=600)
        assert p.returncode == 0, so[-2000:] + se[-2000:]
    dev = torch.device("cuda:0")
    model = trainer.GaussianModel(raw, dev)
    model.training_setup()
    bg = torch.zeros(3, device=dev)
    for c in cams:
        c.to_device(dev)
    for _ in range(iters):
        acc, vis = None, None
        for k in range(2):
            _loss, v = trainer.training_step(model, cams[k], gts[k].to(dev), bg, do_step=False, raw_render=False)
            g = [p.grad.clone() if p.grad is not None else torch.zeros_like(p) for p in model.parameters()]
            model.optimizer.zero_grad(True)
            acc = g if acc is None else [a + b for a, b in zip(acc, g)]
            vis = v if vis is None else (vis | v)
        model.optimizer.set_visibility_and_N(vis, model.P)
        model.optimizer.step(acc)
    rd = lambda name, shape: fio.read(d, name + ".f32", np.float32).numpy().reshape(shape)
    for name, t in (("xyz", model.xyz), ("scaling", model.scaling), ("rotation", model.rotation), ("opacity", model.opacity),
                    ("dc", model.features_dc), ("rest", model.features_rest)):
        assert rel_err(rd(name, tuple(t.shape)), t.detach().cpu().numpy()) < 1e-5, name


def test_dropin_renderer_cpp(tmp_path):
    """shim/renderer.cpp — the drop-in replacement for the reference's src/rasterizer/renderer.cpp (same render() signature; the model's raw
    parameters go to one autograd node whose kernels apply sigmoid / exp / normalize) — against the REFERENCE's renderer.cpp itself.  Both are
    compiled with the reference's renderer.h, rasterizer.{h,cpp}, loss_utils.h and the host lines of gaussian.cpp:683-707 (dropin_check.cpp with
    -DGSLIC_CHECK_RENDER; Camera / GaussianModel are the stand-ins of shim/standin, the reference's need Eigen / OpenCV / PCL), linked once with
    each renderer, and run three optimisation steps on the same inputs.  Same image after three steps (1e-5), same parameters up to what Adam's
    sign-like first steps do to last-bit gradient differences of near-zero elements (the bar of test_fused_training_tracks_dropin_training);
    a third build adds the optional one-node loss (loss_utils_fused.h)."""
    exe_ref = os.path.join(ROOT, "gaussian-lic_amd", "dropin_check_render_ref")
    exe_new = os.path.join(ROOT, "gaussian-lic_amd", "dropin_check_render")
    exe_loss = os.path.join(ROOT, "gaussian-lic_amd", "dropin_check_render_loss")
    if not (os.path.exists(exe_ref) and os.path.exists(exe_new)):
        pytest.skip("dropin_check_render(_ref) not built (needs /root/reference at build time)")
    from gaussian_lic_amd.synthetic import gt_image
    P, W, H, iters = 30000, 320, 240, 3
    raw, sc, camd, cam = make_scene("random", P, W, H, 3, 43)
    d = str(tmp_path)
    fio.write_inputs(d, raw, cam, gt=gt_image(H, W))
    names = ("image", "xyz", "scaling", "rotation", "opacity", "dc", "rest")
    rd = lambda name: fio.read(d, name + ".f32", np.float32).numpy()
    lrs = dict(xyz=1.6e-4, dc=2.5e-3, rest=2.5e-3 / 20.0, opacity=5e-2, scaling=5e-3, rotation=1e-3)

    def run(exe):
        r = fio.run(exe, d, str(P), str(W), str(H), "3", str(iters))
        losses = [float(l.split()[3]) for l in r.stdout.splitlines() if l.startswith("iter ")]
        return {n: rd(n).copy() for n in names}, losses

    ref, loss_ref = run(exe_ref)
    for exe in (exe_new, exe_loss):
        if not os.path.exists(exe):
            continue
        got, loss_got = run(exe)
        np.testing.assert_allclose(loss_got, loss_ref, rtol=2e-5)
        assert rel_err(got["image"], ref["image"]) < 2e-4, os.path.basename(exe)      # (the image after three Adam steps: see the parameter bar)
        for n in names[1:]:
            dlt = np.abs(got[n] - ref[n])
            # (measured: 0.6 % of the opacities, whose rate is the largest, 5e-2 per step; every other group below 0.2 %)
            assert (dlt > 1e-5 * np.abs(ref[n]).max()).mean() < 1e-2, (os.path.basename(exe), n, float((dlt > 1e-5 * np.abs(ref[n]).max()).mean()))
            assert np.median(dlt) <= 2e-7 * max(1.0, float(np.abs(ref[n]).max())), (os.path.basename(exe), n)
            assert dlt.max() <= 2 * iters * lrs[n] * 1.01, (os.path.basename(exe), n, float(dlt.max()))


def test_fused_cpp_host_pose_gradient(tmp_path):
    """gslic::FusedStep::pose_gradient (C++: forward, loss kernels, gslic_rasterize_backward_camera, the se(3) chain on the host) at a rotated
    pose with clamp-masked Gaussians against trainer.pose_gradient (the same calls from Python + Camera.pose_gradient): the six numbers agree."""
    if not os.path.exists(CHECK_FUSED):
        pytest.skip("fused_check not built")
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import gt_image
    P, W, H, deg = 20000, 320, 240, 3
    raw, sc, camd, _cam = make_scene("random", P, W, H, deg, 49)
    cam = synthetic_camera(W, H, 7)
    d = str(tmp_path)
    gt = gt_image(H, W)
    fio.write_inputs(d, raw, cam, gt=gt)
    r = fio.run(CHECK_FUSED, d, str(P), str(W), str(H), str(deg), "1", env=dict(os.environ, GSLIC_CHECK_POSE="1"))   # (the gradient is printed before the one step)
    got = np.array([float(v) for v in [l for l in r.stdout.splitlines() if l.startswith("pose_gradient")][-1].split()[1:]])
    dev = torch.device("cuda:0")
    model = trainer.GaussianModel(raw, dev)
    cam.to_device(dev)
    want, _terms = trainer.pose_gradient(model, cam, gt.to(dev), torch.zeros(3, device=dev))
    assert float(np.abs(got - want).max()) <= 1e-5 * max(float(np.abs(want).max()), 1e-30), (got, want)
