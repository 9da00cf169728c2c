"""Measures the free-space launch beside the plain and the error-weighted one at the config-3 shape, in one process, alternating, median of five
rounds.

    timeout -k 10 600 python tools/freespace_probe.py [--P 2000000] [--width 1920] [--height 1080] [--rounds 5] [--log profiles/freespace_config3.log]

gslic_contribution_accumulate, gslic_contribution_accumulate_error and gslic_contribution_accumulate_free_space on the same forward of the bench
scene (Morton-ordered map, identity camera, strict arithmetic; a seeded error image in [0, 2]; a seeded near bound: a quarter of the pixels
unmeasured, the rest uniform over the scene's depth range 1 .. 30), each between two device events on fresh zero accumulators, the three in turn
within every round.  The process is the one GPU step: run it under a time limit as above.  Before anything is timed the free-space launch's three
base statistics are compared with the plain launch's on the bits, so that a wrong run does not pass as a fast one.  Prints one JSON line and
appends it to --log."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=2_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--log", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "freespace_config3.log"))
    a = ap.parse_args()
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd import rasterizer as rz
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import random_scene
    assert torch.cuda.is_available(), "freespace_probe needs a GPU: a time taken anywhere else says nothing"
    dev = torch.device("cuda:0")
    P, W, H = a.P, a.width, a.height
    med = statistics.median

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    model = trainer.GaussianModel(random_scene(P, W, H, sh_degree=3, seed=0), dev, order="morton")
    cam = synthetic_camera(W, H).to_device(dev)
    fwd = trainer._RawRaster(model, cam, torch.zeros(3, device=dev))
    g = torch.Generator(device=dev).manual_seed(1)
    err = 2.0 * torch.rand(H, W, device=dev, generator=g)
    near = 1.0 + 29.0 * torch.rand(H, W, device=dev, generator=g)
    near[torch.rand(H, W, device=dev, generator=g) < 0.25] = 0.0
    z32, z64 = (lambda: torch.zeros(P, dtype=torch.int32, device=dev)), (lambda: torch.zeros(P, dtype=torch.int64, device=dev))
    acc = [z32(), z32(), z64(), z64(), z64(), z64()]   # max_w, n_pix, sum_w, err_sum, free_sum, meas_sum
    with torch.no_grad():
        fwd.forward()
    R, B, _radii, geom, binning, img, _sample = fwd.state
    plain = lambda: rz.contribution_accumulate(P, H, W, R, B, geom, binning, img, 0.05, *acc[:3])
    weighted = lambda: rz.contribution_accumulate(P, H, W, R, B, geom, binning, img, 0.05, *acc[:3], error=err, err_sum=acc[3])
    free = lambda: rz.contribution_accumulate(P, H, W, R, B, geom, binning, img, 0.05, *acc[:3], near_bound=near, free_sum=acc[4], meas_sum=acc[5])

    def zero():
        for t in acc:
            t.zero_()
    zero(); plain(); torch.cuda.synchronize()
    want = [t.clone() for t in acc[:3]]
    zero(); free(); torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(want, acc[:3])), "the free-space launch changed the base statistics"
    assert bool((acc[4] <= acc[5]).all()) and bool((acc[5] <= acc[2]).all()) and bool(acc[4].any())
    zero(); weighted()
    ms = {"plain": [], "error": [], "free_space": []}
    for _ in range(a.rounds):
        for name, fn in (("plain", plain), ("error", weighted), ("free_space", free)):
            zero()
            ms[name].append(timed(fn))
    out = dict(P=P, W=W, H=H, R=R, rounds=a.rounds, device=torch.cuda.get_device_name(0))
    for name, v in ms.items():
        out[f"contribution_{name}_event_ms"] = [round(x, 4) for x in v]
        out[f"contribution_{name}_event_ms_median"] = round(med(v), 4)
    out.update(error_over_plain=round(med(ms["error"]) / med(ms["plain"]), 3), free_space_over_plain=round(med(ms["free_space"]) / med(ms["plain"]), 3),
               sum_w=round(float(trainer.fixed_to_weight(acc[2]).sum()), 3), free_sum=round(float(trainer.fixed_to_weight(acc[4]).sum()), 3),
               meas_sum=round(float(trainer.fixed_to_weight(acc[5]).sum()), 3))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    with open(a.log, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
