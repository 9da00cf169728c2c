"""RCCL smoke test of the N > 1 step on a single-GPU box: a process group of ONE rank with GSLIC_FORCE_DIST=1 takes exactly the code
path every rank takes at N > 1 (gradients to the flat slab -> all_reduce(SUM) on the slab + all_reduce(MAX) on the visibility bytes
through torch.distributed's nccl (= RCCL) backend -> masked Adam).  With one rank the sum is the identity, so the trajectory must
equal the single-process split-Adam path bit for bit.  (World size 2 is covered on CPU with gloo, tests/test_distributed_cpu.py.)"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SNIPPET = r"""
import os, sys, torch
sys.path.insert(0, {root!r})
import gaussian_lic_amd
from gaussian_lic_amd import trainer
from gaussian_lic_amd.camera import synthetic_camera
from gaussian_lic_amd.synthetic import random_scene, gt_image
dev = torch.device("cuda", 0); torch.cuda.set_device(dev)
forced = os.environ.get("GSLIC_FORCE_DIST") == "1"
if forced:
    torch.distributed.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
W, H, P = 320, 192, 30000
model = trainer.GaussianModel(random_scene(P, W, H, 3, 5), dev); model.training_setup()
cam = synthetic_camera(W, H).to_device(dev); gt = gt_image(H, W).to(dev); bg = torch.zeros(3, device=dev)
for _ in range(3):
    loss = trainer.training_step_fused(model, cam, gt, bg, adam_in_backward=False)[0]
torch.cuda.synchronize()
import hashlib
h = hashlib.sha256()
for t in (model.xyz, model.features_dc, model.features_rest, model.opacity, model.scaling, model.rotation):
    h.update(t.detach().cpu().numpy().tobytes())
print("DIGEST", h.hexdigest(), float(torch.as_tensor(loss).double().sum()))
if forced:
    torch.distributed.destroy_process_group()
"""


def _run(force):
    env = dict(os.environ)
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", HSA_ENABLE_IPC_MODE_LEGACY="0")
    if force:
        env["GSLIC_FORCE_DIST"] = "1"
    else:
        env.pop("GSLIC_FORCE_DIST", None)
    r = subprocess.run([sys.executable, "-c", SNIPPET.format(root=ROOT)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("DIGEST")][-1].split()
    return line[1], float(line[2])


@pytest.mark.gpu
def test_rccl_exchange_path_world1_matches_local_path():
    d_local, l_local = _run(False)
    d_dist, l_dist = _run(True)
    assert l_local == l_dist
    assert d_local == d_dist


@pytest.mark.gpu
def test_bench_under_torchrun_one_rank():
    """bench.py launched the way the driver launches it (torch.distributed.run, RANK / WORLD_SIZE from the environment) prints one
    JSON line with the contract's keys."""
    env = dict(os.environ)
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", GSLIC_FORCE_DIST="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", "29541", os.path.join(ROOT, "bench.py"), "--full", "--gpus", "1", "--steps", "3", "--warmup", "2", "--gaussians", "100000",
           "--width", "640", "--height", "360", "--no-cpu-baseline"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["value"] > 0


@pytest.mark.gpu
def test_bench_gpus_2_launches_itself():
    """`python bench.py --gpus 2` with no launcher and no WORLD_SIZE — the shape of the driver's N = 1 command — spawns its two ranks itself and prints
    ONE JSON line from rank 0 carrying the N > 1 fields.  On a one-GPU box the two ranks share the device (RCCL refuses that: the collectives go
    through gloo on device tensors and the line says so); on a box with two GPUs the same command runs over RCCL and `rccl_ranks` is 2."""
    import torch
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "GSLIC_FORCE_DIST")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", GSLIC_DIST_PRIME_STEPS="3")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "3", "--warmup", "2", "--gaussians", "100000",
           "--width", "640", "--height", "360", "--no-cpu-baseline"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.count("\n") == 1 and r.stdout.startswith("{"), "stdout must hold the ONE JSON line and nothing else: " + r.stdout[:400]
    d = json.loads(r.stdout)
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["value"] > 0 and d["scaling"] == "weak"
    assert d["launch"]["ranks"] == 2 and d["launch"]["ranks_reached_by_all_reduce"] == 2 and d["launch"]["self_launched"] is True
    assert len(d["per_rank_ms_per_step"]) == 2 and all(v > 0 for v in d["per_rank_ms_per_step"])
    assert d["exchange"]["world"] == 2 and d["exchange"]["collectives_per_step"] == 3
    mb = d["rccl_microbench"]
    for k in ("all_gather_payload", "all_reduce_xyz", "all_reduce_opacity_scaling_rotation", "all_reduce_dense_slab", "three_collectives_of_the_step_together"):
        assert mb[k]["ms"] > 0, (k, mb)
    if torch.cuda.device_count() >= 2:
        assert d["rccl_ranks"] == 2 and d["launch"]["backend"].startswith("nccl")
    else:
        assert d["rccl_ranks"] is None and d["launch"]["backend"].startswith("gloo")


TWO_RANK_SNIPPET = r"""
import os, sys, hashlib, torch
sys.path.insert(0, {root!r})
import gaussian_lic_amd
from gaussian_lic_amd import trainer
from gaussian_lic_amd.camera import synthetic_camera
from gaussian_lic_amd.synthetic import random_scene, gt_image
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dev = torch.device("cuda", 0); torch.cuda.set_device(dev)
W, H, P, STEPS = 320, 192, 30000, 3
def digest(model):
    h = hashlib.sha256()
    for t in (model.xyz, model.features_dc, model.features_rest, model.opacity, model.scaling, model.rotation):
        h.update(t.detach().cpu().numpy().tobytes())
    return h.hexdigest()
bg = torch.zeros(3, device=dev)
if world > 1:
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)   # both ranks share the one GPU of the box
    model = trainer.GaussianModel(random_scene(P, W, H, 3, 5), dev); model.training_setup()
    cam = synthetic_camera(W, H, rank).to_device(dev); gt = gt_image(H, W, seed=2 + rank).to(dev)
    for _ in range(STEPS):
        trainer.training_step_fused(model, cam, gt, bg)
    torch.cuda.synchronize()
    print("DIGEST", rank, digest(model))
    torch.distributed.barrier(); torch.distributed.destroy_process_group()
else:
    # single-process restatement of the same two-view step: gradients of view 0 and view 1 summed, masks OR-ed, one masked Adam
    model = trainer.GaussianModel(random_scene(P, W, H, 3, 5), dev); model.training_setup()
    cams = [synthetic_camera(W, H, k).to_device(dev) for k in range(2)]
    gts = [gt_image(H, W, seed=2 + k).to(dev) for k in range(2)]
    for _ in range(STEPS):
        flats, vis = [], []
        for k in range(2):
            _, v = trainer.training_step_fused(model, cams[k], gts[k], bg, do_step=False, adam_in_backward=False)
            flats.append(model._grad_slab.flat.clone()); vis.append(v.clone())
        model._grad_slab.flat.copy_(flats[0] + flats[1])
        model.optimizer.set_visibility_and_N(vis[0] | vis[1], model.P)
        model.optimizer.step(model._grad_slab.grads(model))
    torch.cuda.synchronize()
    print("DIGEST", 0, digest(model))
"""


@pytest.mark.gpu
def test_two_ranks_sharing_one_gpu_match_the_summed_gradient_step():
    """The complete N = 2 step on real kernels: two processes (gloo backend on device tensors, both on the box's one GPU), rank k
    renders view k, pipelined slab exchange, masked Adam.  Both replicas must end bit-identical to each other and to a
    single-process restatement (gradients of the two views summed, masks OR-ed, one Adam)."""
    port = "29561"
    def run(rank, world):
        env = dict(os.environ)
        env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
        env.pop("GSLIC_FORCE_DIST", None)
        return subprocess.Popen([sys.executable, "-c", TWO_RANK_SNIPPET.format(root=ROOT)], env=env, stdout=subprocess.PIPE,
                                stderr=subprocess.PIPE, text=True)
    procs = [run(0, 2), run(1, 2)]
    outs = [p.communicate(timeout=600) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-2000:]
    d = [[l for l in so.splitlines() if l.startswith("DIGEST")][-1].split()[2] for so, _ in outs]
    assert d[0] == d[1]
    ref = run(0, 1)
    so, se = ref.communicate(timeout=600)
    assert ref.returncode == 0, se[-2000:]
    dref = [l for l in so.splitlines() if l.startswith("DIGEST")][-1].split()[2]
    assert d[0] == dref


@pytest.mark.gpu
def test_two_ranks_sparse_exchange_equals_dense():
    """The visible-rows-only exchange (GSLIC_SPARSE_EXCHANGE=1: OR the masks, all-reduce the compacted rows, scatter back) on the
    complete N = 2 step, two processes sharing the GPU: the replicas end bit-identical to the dense-slab trajectory."""
    def run(rank, sparse, port):
        env = dict(os.environ)
        env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
        env.pop("GSLIC_FORCE_DIST", None)
        env.pop("GSLIC_SPARSE_EXCHANGE", None)
        env["GSLIC_EXCHANGE"] = "sparse" if sparse else "dense"
        return subprocess.Popen([sys.executable, "-c", TWO_RANK_SNIPPET.format(root=ROOT)], env=env, stdout=subprocess.PIPE,
                                stderr=subprocess.PIPE, text=True)
    digests = []
    for sparse, port in ((False, "29571"), (True, "29573")):
        procs = [run(0, sparse, port), run(1, sparse, port)]
        outs = [p.communicate(timeout=600) for p in procs]
        for p, (so, se) in zip(procs, outs):
            assert p.returncode == 0, se[-2000:]
        d = [[l for l in so.splitlines() if l.startswith("DIGEST")][-1].split()[2] for so, _ in outs]
        assert d[0] == d[1]
        digests.append(d[0])
    assert digests[0] == digests[1]


@pytest.mark.gpu
def test_two_ranks_rank1_exchange_equals_dense():
    """The default N > 1 exchange (rank-1: 11 floats all-reduced, the 3-float colour gradients all-gathered, SH rows rebuilt locally)
    against GSLIC_EXCHANGE=dense (the whole slab all-reduced) on the complete N = 2 step, two processes sharing the GPU: the same bits."""
    def run(rank, mode, port):
        env = dict(os.environ)
        env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE="2", HSA_ENABLE_IPC_MODE_LEGACY="0", GSLIC_EXCHANGE=mode)
        env.pop("GSLIC_FORCE_DIST", None); env.pop("GSLIC_SPARSE_EXCHANGE", None)
        return subprocess.Popen([sys.executable, "-c", TWO_RANK_SNIPPET.format(root=ROOT)], env=env, stdout=subprocess.PIPE,
                                stderr=subprocess.PIPE, text=True)
    digests = []
    # ... and GSLIC_EXCHANGE=single (round 6: north_star's "single all-reduce" to the letter — slab and mask in ONE collective): the same bits again
    for mode, port in (("dense", "29575"), ("rank1", "29577"), ("single", "29579")):
        procs = [run(0, mode, port), run(1, mode, port)]
        outs = [p.communicate(timeout=600) for p in procs]
        for p, (so, se) in zip(procs, outs):
            assert p.returncode == 0, se[-2000:]
        d = [[l for l in so.splitlines() if l.startswith("DIGEST")][-1].split()[2] for so, _ in outs]
        assert d[0] == d[1]
        digests.append(d[0])
    assert digests[0] == digests[1] == digests[2]


RCCL2_SNIPPET = r"""
import os, sys, hashlib, torch
sys.path.insert(0, {root!r})
import gaussian_lic_amd
from gaussian_lic_amd import trainer
from gaussian_lic_amd.camera import synthetic_camera
from gaussian_lic_amd.synthetic import random_scene, gt_image
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dev = torch.device("cuda", rank); torch.cuda.set_device(dev)
torch.distributed.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
W, H, P = 320, 192, 30000
model = trainer.GaussianModel(random_scene(P, W, H, 3, 5), dev); model.training_setup()
cam = synthetic_camera(W, H, rank).to_device(dev); gt = gt_image(H, W, seed=2 + rank).to(dev); bg = torch.zeros(3, device=dev)
for _ in range(3):
    trainer.training_step_fused(model, cam, gt, bg)
torch.cuda.synchronize()
h = hashlib.sha256()
for t in (model.xyz, model.features_dc, model.features_rest, model.opacity, model.scaling, model.rotation):
    h.update(t.detach().cpu().numpy().tobytes())
print("DIGEST", rank, h.hexdigest())
torch.distributed.barrier(); torch.distributed.destroy_process_group()
"""


@pytest.mark.gpu
def test_rccl_two_ranks_two_gpus():
    """The N = 2 step over RCCL proper (one process per GPU, backend nccl).  Needs two devices: skipped on the one-GPU test box, runs
    wherever the driver has a multi-GPU node.  Both replicas must end bit-identical, and equal to the two-processes-one-GPU gloo run."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs (RCCL refuses two ranks on one device)")
    procs = []
    for rank in range(2):
        env = dict(os.environ)
        env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29581", RANK=str(rank), WORLD_SIZE="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
        env.pop("GSLIC_FORCE_DIST", None)
        procs.append(subprocess.Popen([sys.executable, "-c", RCCL2_SNIPPET.format(root=ROOT)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=900) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-2000:]
    d = [[l for l in so.splitlines() if l.startswith("DIGEST")][-1].split()[2] for so, _ in outs]
    assert d[0] == d[1]


# ---------------------------------------------------------------------------------------------------------------------------------------
# N = 4 and N = 8 (one view per rank, ONE exchange per optimiser step), every rank a process of its own sharing the box's
# one GPU, gloo on device tensors.  What can be proven without the 8-GPU node: (1) the exchanged gradients equal the sum over the views
# of the single-GPU gradients (1e-5 of the group's max-abs; the reduction order is the backend's) and the mask is the OR of the views'
# masks, exactly; (2) after three complete steps every replica holds the same bits, for the rank-1 and the dense exchange.
N_RANK_SNIPPET = r"""
import os, sys, hashlib, numpy as np, torch
sys.path.insert(0, {root!r})
import gaussian_lic_amd
from gaussian_lic_amd import trainer
from gaussian_lic_amd.camera import synthetic_camera
from gaussian_lic_amd.synthetic import random_scene, gt_image
rank, world, task, out = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), os.environ["GSLIC_TEST_TASK"], os.environ["GSLIC_TEST_OUT"]
nviews = int(os.environ.get("GSLIC_TEST_VIEWS", world))
dev = torch.device("cuda", 0); torch.cuda.set_device(dev)
W, H, P = (int(os.environ.get(k, d)) for k, d in (("GSLIC_TEST_W", 320), ("GSLIC_TEST_H", 192), ("GSLIC_TEST_P", 30000)))
bg = torch.zeros(3, device=dev)
model = trainer.GaussianModel(random_scene(P, W, H, 3, 5), dev); model.training_setup()
def digest(m):
    h = hashlib.sha256()
    for t in (m.xyz, m.features_dc, m.features_rest, m.opacity, m.scaling, m.rotation):
        h.update(t.detach().cpu().numpy().tobytes())
    return h.hexdigest()
if task == "reference":      # one process: the per-view gradients of views 0..nviews-1, summed in float64, masks OR-ed
    acc, vis = None, None
    for k in range(nviews):
        cam = synthetic_camera(W, H, k).to_device(dev); gt = gt_image(H, W, seed=2 + k).to(dev)
        _, v = trainer.training_step_fused(model, cam, gt, bg, do_step=False, adam_in_backward=False)
        f = model._grad_slab.flat.double().cpu().numpy()
        acc = f if acc is None else acc + f
        vis = v.cpu().numpy() if vis is None else (vis | v.cpu().numpy())
    np.savez(out, flat=acc, vis=vis, sizes=np.array([model._grad_slab.views[n].numel() for n in model.NAMES]))
else:
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    cam = synthetic_camera(W, H, rank).to_device(dev); gt = gt_image(H, W, seed=2 + rank).to(dev)
    if task == "grads":      # one exchange, no optimiser: what the ranks agree on
        model.optimizer.step = lambda *a, **k: None
        if hasattr(model.optimizer, "step_sh_from_rgb"):
            model.optimizer.step_sh_from_rgb = lambda *a, **k: None
        _, v = trainer.training_step_fused(model, cam, gt, bg)
        torch.cuda.synchronize()
        if rank == 0:
            np.savez(out, flat=model._grad_slab.flat.cpu().numpy(), vis=v.cpu().numpy())
    else:                    # three complete steps
        for _ in range(3):
            trainer.training_step_fused(model, cam, gt, bg)
        torch.cuda.synchronize()
        print("DIGEST", rank, digest(model))
    torch.distributed.barrier(); torch.distributed.destroy_process_group()
"""


def _spawn_ranks(world, task, mode, port, out, extra_env=None):
    procs = []
    for rank in range(world):
        env = dict(os.environ)
        env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0",
                   GSLIC_EXCHANGE=mode, GSLIC_TEST_TASK=task, GSLIC_TEST_OUT=out)
        env.update(extra_env or {})
        env.pop("GSLIC_FORCE_DIST", None); env.pop("GSLIC_SPARSE_EXCHANGE", None)
        procs.append(subprocess.Popen([sys.executable, "-c", N_RANK_SNIPPET.format(root=ROOT)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=1200) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-2000:]
    return [so for so, _ in outs]


@pytest.mark.gpu
@pytest.mark.parametrize("world", [4, 8])
def test_n_ranks_exchanged_gradients_equal_the_sum_over_views(world, tmp_path):
    import numpy as np
    ref_file = str(tmp_path / "ref.npz")
    _spawn_ranks(1, "reference", "dense", 29601 + world, ref_file, {"GSLIC_TEST_VIEWS": str(world)})
    ref = np.load(ref_file)
    offs = np.concatenate([[0], np.cumsum(ref["sizes"])])
    for mode, port in (("dense", 29611 + world), ("rank1", 29621 + world)):
        got_file = str(tmp_path / f"got_{mode}.npz")
        # rank-1: rebuild the SH rows into the slab (the fused rebuild + Adam kernel never materialises them)
        _spawn_ranks(world, "grads", mode, port, got_file, {"GSLIC_RANK1_SPLIT_ADAM": "1"})
        got = np.load(got_file)
        np.testing.assert_array_equal(got["vis"], ref["vis"], err_msg=f"{mode}: mask != OR of the views' masks")
        for g in range(6):
            a, b = got["flat"][offs[g]:offs[g + 1]], ref["flat"][offs[g]:offs[g + 1]]
            scale = max(float(np.abs(b).max()), 1e-30)
            assert float(np.abs(a - b).max()) / scale < 1e-5, (mode, g, float(np.abs(a - b).max()) / scale)


@pytest.mark.gpu
def test_config4_full_size_eight_views_gradient_sum(tmp_path):
    """BASELINE config 4 at its own size: 2 000 000 Gaussians, 1920x1080, eight views k = 0..7 (yaw (k - 3.5) 4 deg, x = (k - 3.5) 0.25 m),
    one per rank — eight processes sharing the box's one GPU, gloo on device tensors.  The exchanged gradient slab equals sum_k grad(view k) of
    the single-GPU path (1e-5 of each group's max-abs) and the mask equals OR_k visible_k exactly, for the rank-1 exchange (default: dRGB
    all-gathered, SH rows rebuilt) and for the dense slab all-reduce."""
    import numpy as np
    size = {"GSLIC_TEST_W": "1920", "GSLIC_TEST_H": "1080", "GSLIC_TEST_P": "2000000"}
    ref_file = str(tmp_path / "ref.npz")
    _spawn_ranks(1, "reference", "dense", 29801, ref_file, dict(size, GSLIC_TEST_VIEWS="8"))
    ref = np.load(ref_file)
    rflat, rvis = ref["flat"], ref["vis"]
    offs = np.concatenate([[0], np.cumsum(ref["sizes"])])
    assert int(rvis.sum()) > 1_000_000 and rflat.size == 59 * 2_000_000
    for mode, port in (("rank1", 29811), ("dense", 29821)):
        got_file = str(tmp_path / f"got_{mode}.npz")
        _spawn_ranks(8, "grads", mode, port, got_file, dict(size, GSLIC_RANK1_SPLIT_ADAM="1"))
        got = np.load(got_file)
        np.testing.assert_array_equal(got["vis"], rvis, err_msg=f"{mode}: mask != OR of the eight views' masks")
        gflat = got["flat"]
        for g in range(6):
            a, b = gflat[offs[g]:offs[g + 1]], rflat[offs[g]:offs[g + 1]]
            scale = max(float(np.abs(b).max()), 1e-30)
            err = float(np.abs(a - b).max()) / scale
            print(f"config 4 full size, {mode}, group {g}: max |exchanged - sum of views| / max-abs = {err:.2e}")
            assert err < 1e-5, (mode, g, err)
        del got, gflat
        os.remove(got_file)


@pytest.mark.gpu
@pytest.mark.parametrize("world", [4, 8])
@pytest.mark.parametrize("mode", ["rank1", "dense"])
def test_n_ranks_replicas_stay_bit_identical(world, mode):
    outs = _spawn_ranks(world, "steps", mode, 29640 + world + (0 if mode == "rank1" else 20), "unused")
    d = [[l for l in so.splitlines() if l.startswith("DIGEST")][-1].split()[2] for so in outs]
    assert len(set(d)) == 1, d


@pytest.mark.gpu
def test_chunked_exchange_equals_unchunked():
    """GSLIC_EXCHANGE_CHUNKS=4: the per-Gaussian backward in four row chunks, a chunk's all-gather + all-reduce on the wire while the next
    chunk is computed, Adam per chunk.  Per Gaussian the arithmetic is the unchunked step's: at N = 2 (two addends) the replicas end with the
    SAME BITS as without chunking; at N = 4 all replicas agree with each other."""
    d1 = _spawn_ranks(2, "steps", "rank1", 29701, "unused")
    d4 = _spawn_ranks(2, "steps", "rank1", 29703, "unused", {"GSLIC_EXCHANGE_CHUNKS": "4"})
    g = lambda outs: [[l for l in so.splitlines() if l.startswith("DIGEST")][-1].split()[2] for so in outs]
    a, b = g(d1), g(d4)
    assert len(set(a)) == 1 and len(set(b)) == 1 and a[0] == b[0], (a, b)
    c = g(_spawn_ranks(4, "steps", "rank1", 29705, "unused", {"GSLIC_EXCHANGE_CHUNKS": "3"}))
    assert len(set(c)) == 1, c
