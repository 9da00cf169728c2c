"""-m gpu: the launch switches of the blend kernels that no other suite sets (csrc/render.hip: launch_render_fwd_t, launch_render_bwd) —
GSLIC_FWD_SPLIT = 1 | 4 (render_fwd_kernel<*, 1 | 4>: one and four waves per tile), GSLIC_BWD_XCD_RUN = 0 | 1 | 4 | 2048 (no blockIdx remap;
units of 8 and 32 buckets; a grid padded far past B) and GSLIC_BWD_SCAN = 0 (the pipeline kernel in the strict mode too).  The first two
change which wave or workgroup does a piece of work and nothing else: image, final_T, n_contrib, radii, every gradient of a colour and a
depth backward and the Adam state after two fused steps must be the default process's BITS, in both arithmetic modes, on the designed
ragged scene of tests/blend_cases.py and on a random one.  GSLIC_BWD_SCAN = 0 changes the association of the strict backward's sums: its
forward and its whole fast mode keep the bits, its strict gradients are held to the fp64 oracle with the rule and FACTOR of
tests/test_blend_cases_gpu.py (see test_pipeline_kernel_in_the_strict_mode).
Each switch is read once per process, so every setting runs in a fresh child process (as tests/test_fwd_tail_gpu.py), one after another."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TENSORS = ("dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dcov3D")

PROBE = r"""
import hashlib, json, os, sys
import numpy as np, torch
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import gaussian_lic_amd
from gaussian_lic_amd import trainer, _lib
from gaussian_lic_amd.synthetic import gt_image, pixel_grad
import blend_cases as bc
from conftest import make_scene
from gpu_helpers import hip_forward, hip_backward, npy
from test_depth_gpu import bwd, fwd_depth
save = sys.argv[1]
dev = torch.device("cuda:0")
def dig(a):
    return hashlib.sha256(np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a).tobytes()).hexdigest()
raw_d, _, _, cam_d, plan = bc.build("ragged")
dL_d, gD_d = (torch.from_numpy(a) for a in bc.pixel_grads(plan["W"], plan["H"]))
raw_r, _, _, cam_r = make_scene("random", 20000, 200, 120, 3, 11)
dL_r, gD_r = pixel_grad(120, 200, seed=2), torch.randn(120, 200, generator=torch.Generator().manual_seed(3)).float()
out, keep = {}, {}
for mode in ("strict", "fast"):
    _lib.set_math_mode(mode == "strict")
    for name, raw, cam, dL, gD in (("designed", raw_d, cam_d, dL_d, gD_d), ("random", raw_r, cam_r, dL_r, gD_r)):
        o = {}
        f = hip_forward(raw, cam, export=("n_contrib",))
        fd = fwd_depth(raw, cam)
        for k in ("color", "final_T", "radii"):
            o[k] = dig(f[k])
        o["n_contrib"], o["depth"] = dig(f["dbg"]["n_contrib"]), dig(fd["depth"])
        gc, gd = hip_backward(f, dL), bwd(fd, dL, gD)
        grads = {"colour " + k: v for k, v in gc.items()}
        grads.update({"depth " + k: v for k, v in gd.items()})
        for k, v in grads.items():
            o["grad " + k] = dig(v)
        if mode == "strict" and name == "designed":
            keep = grads
        if mode == "fast":      # the strict backward behind a fast forward: the pipeline's fallback, the fast backward's bits
            _lib.set_math_mode(True)
            fc, fdp = hip_backward(f, dL), bwd(fd, dL, gD)
            _lib.set_math_mode(False)
            o["fallback is the fast backward"] = str(all(np.array_equal(fc[k], gc[k]) and np.array_equal(fdp[k], gd[k]) for k in gc))
        model = trainer.GaussianModel({k: (v.clone() if torch.is_tensor(v) else v) for k, v in raw.items()}, dev)
        model.training_setup()
        H, W = cam.image_height, cam.image_width
        gt, bg, camd = gt_image(H, W, seed=3).to(dev), torch.zeros(3, device=dev), cam.to_device(dev)
        for _ in range(2):
            trainer.training_step_fused(model, camd, gt, bg)
        torch.cuda.synchronize()
        for n in model.NAMES:
            o["adam p " + n], o["adam m " + n], o["adam v " + n] = dig(getattr(model, n)), dig(model._m[n][:model.P]), dig(model._v[n][:model.P])
        out[mode + " " + name] = o
np.savez(save, **keep)
print("DIGESTS " + json.dumps(out))
""" % (ROOT, ROOT)

_default = {}
_stopped = []      # the first child that did not end well (exit status, time limit, no digests): none is started after it
# A child's time limit: the slowest measured child took 2.8 s on an MI355X (profiles/blend_cases_factors.txt, "child processes"), most of it
# the interpreter's and the library's start; twenty times that leaves room for a cold start on a loaded machine and still ends a hung
# child within a minute.
CHILD_TIMEOUT = 60
# distinct digests every section of a child's report must hold at the least: 5 forward items + the 9 gradients of one backward + parameter and
# two moments of one group (the depth backward repeats the colour's bits in the tensors depth does not reach, and zero moments can coincide)
MIN_DIGESTS = 5 + 9 + 3


def _run(env_set, tmp_path, tag):
    """One child.  Whatever goes wrong with it — exit status, time limit, any other failure to run it, no DIGESTS line — is recorded, and no
    further child is started in this session: what faulted or hung on the card is not followed by more work on it."""
    env = dict(os.environ)
    for k in ("GSLIC_FWD_SPLIT", "GSLIC_BWD_XCD_RUN", "GSLIC_BWD_SCAN"):
        env.pop(k, None)
    env.update(env_set)
    save = str(tmp_path / f"{tag}.npz")
    assert not _stopped, f"no further child is started: {_stopped[0]}"
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, "-c", PROBE, save], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except BaseException as e:      # TimeoutExpired (the child has been killed by then) and anything else
        _stopped.append(f"the child with {env_set} did not finish: {type(e).__name__}")
        raise
    print(f"\n[child {env_set or 'default'}] {time.perf_counter() - t0:.1f} s of {CHILD_TIMEOUT} s")
    lines = [l for l in r.stdout.splitlines() if l.startswith("DIGESTS ")]
    if r.returncode != 0 or not lines:
        _stopped.append(f"the child with {env_set} exited {r.returncode}" + ("" if lines else " without its digests"))
    assert r.returncode == 0, f"{env_set}: the child exited {r.returncode}\n{r.stderr[-2000:]}"
    assert lines, f"{env_set}: the child printed no digests\n{r.stdout[-1000:]}\n{r.stderr[-1000:]}"
    return json.loads(lines[-1][len("DIGESTS "):]), save


def _reference(tmp_path_factory):
    """the default process's digests: one child, shared (a default child that did not end well is not started again: _run refuses)"""
    if not _default:
        d, npz = _run({}, tmp_path_factory.mktemp("blend_variants"), "default")
        for section in d.values():
            # digests of different things: a probe that hashed one buffer again and again would pass every equality below
            assert len(set(section.values())) >= MIN_DIGESTS, sorted(section)
        _default["d"], _default["npz"] = d, npz
    return _default["d"]


@pytest.mark.parametrize("var,value", [("GSLIC_FWD_SPLIT", 1), ("GSLIC_FWD_SPLIT", 4), ("GSLIC_BWD_XCD_RUN", 0), ("GSLIC_BWD_XCD_RUN", 1),
                                       ("GSLIC_BWD_XCD_RUN", 4), ("GSLIC_BWD_XCD_RUN", 2048)])
def test_launch_switch_changes_no_bit(tmp_path_factory, tmp_path, var, value):
    ref = _reference(tmp_path_factory)
    got, _ = _run({var: str(value)}, tmp_path, "variant")
    for section in ref:
        diff = [k for k in ref[section] if ref[section][k] != got[section][k]]
        assert not diff, f"{var}={value}, {section}: {diff} differ from the default launch"
        if section.startswith("fast"):
            assert got[section]["fallback is the fast backward"] == "True", (var, value, section)


def test_pipeline_kernel_in_the_strict_mode(tmp_path_factory, tmp_path, oracle32, oracle64):
    """GSLIC_BWD_SCAN=0: render_bwd_kernel<true, *> behind a strict forward.  "Within the tolerance of the scan kernel's gradients" is read
    as: held to the fp64 oracle by the same per-case rule and FACTOR as the scan kernel in tests/test_blend_cases_gpu.py (two results
    inside that bound are within twice it of each other), plus the proof that another kernel ran (some gradient bit moved).  Bit equality
    with the in-process fallback — the strict backward behind a FAST forward — cannot hold for this child's strict run and is not asserted:
    the fallback replays the fast forward's checkpoints, this run the strict forward's, and the two forwards differ in their bits.  What is
    asserted is that inside this child, as inside every other, the fallback equals the fast backward bit for bit."""
    import blend_cases as bc
    import rowwise as rw
    from test_blend_cases_gpu import _check_grads, _world
    ref = _reference(tmp_path_factory)
    got, save = _run({"GSLIC_BWD_SCAN": "0"}, tmp_path, "pipeline")
    for section in ref:
        moved = [k for k in ref[section] if ref[section][k] != got[section][k]]
        if section.startswith("strict"):       # the sums' association differs: gradients, hence the Adam state, may move; the forward may not
            assert not [k for k in moved if not (k.startswith("grad ") or k.startswith("adam "))], (section, moved)
        else:
            assert not moved, (section, moved)
            assert got[section]["fallback is the fast backward"] == "True", section
    w = _world("ragged", oracle32, oracle64)
    g = np.load(save)
    for kind, tag in (("colour", "gc"), ("depth", "gd")):
        _check_grads({k: g[f"{kind} {k}"] for k in TENSORS}, w, tag, f"ragged strict pipeline {kind}")
    # ... and it is a different kernel: some gradient bit moved against the scan kernel's
    assert any(k.startswith("grad ") and ref["strict designed"][k] != got["strict designed"][k] for k in ref["strict designed"])
