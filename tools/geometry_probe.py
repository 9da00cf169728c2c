"""Times gslic_geometry_images (all seven outputs) at the config-3 shape against gslic_contribution_accumulate on the same forward, in the same
process, alternating.

    python tools/geometry_probe.py [--P 2000000] [--width 1920] [--height 1080] [--rounds 5]

The bench scene (synthetic.random_scene, seed 0, SH degree 3) in a Morton-ordered map, identity camera, strict arithmetic, ONE raw-parameter
forward.  Per round: the contribution launch on fresh zero accumulators between two device events, then the geometry launch between two device
events.  Both walk the same lists; the contribution launch adds the reductions and atomics, the geometry launch the seven stores per pixel.  Prints
one JSON line with the five times of each, their medians, the ratio, and what the view gave (sum of the opacity image against the covered pixels
and against the contribution launch's sum of weights, pixels with an owner, pixels that reach the median) so that a wrong run does not pass as a
fast one."""
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
    ap.add_argument("--a-min", type=float, default=0.05)
    a = ap.parse_args()
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd import rasterizer as rz
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import random_scene
    assert torch.cuda.is_available(), "geometry_probe needs a GPU: a time taken anywhere else says nothing"
    dev = torch.device("cuda:0")
    P, W, H = a.P, a.width, a.height
    model = trainer.GaussianModel(random_scene(P, W, H, sh_degree=3, seed=0), dev, order="morton")
    cam = synthetic_camera(W, H).to_device(dev)
    fwd = trainer._RawRaster(model, cam, torch.zeros(3, device=dev))
    acc = [torch.zeros(P, dtype=torch.int32, device=dev), torch.zeros(P, dtype=torch.int32, device=dev), torch.zeros(P, dtype=torch.int64, device=dev)]
    out = {n: torch.empty(H, W, dtype=torch.int32 if n == "top_row" else torch.float32, device=dev) for n in rz.GEOMETRY_IMAGES}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    with torch.no_grad():
        fwd.forward()
        R, B, _radii, geom, binning, img, _sample = fwd.state
        contribution = lambda: rz.contribution_accumulate(P, H, W, R, B, geom, binning, img, 0.05, *acc)
        geometry = lambda: rz.geometry_images(P, H, W, R, B, geom, binning, img, a.a_min, out)
        for _ in range(2):   # warm both at the timed shape
            contribution()
            geometry()
        torch.cuda.synchronize()
        contrib_ms, geom_ms = [], []
        for _ in range(a.rounds):
            for t in acc:
                t.zero_()
            torch.cuda.synchronize()
            contrib_ms.append(timed(contribution))
            geom_ms.append(timed(geometry))
    med = statistics.median
    res = dict(P=P, W=W, H=H, R=R, rounds=a.rounds, a_min=a.a_min,
               contribution_event_ms=[round(x, 4) for x in contrib_ms], contribution_event_ms_median=round(med(contrib_ms), 4),
               geometry_event_ms=[round(x, 4) for x in geom_ms], geometry_event_ms_median=round(med(geom_ms), 4),
               ratio_to_contribution=round(med(geom_ms) / med(contrib_ms), 2),
               sum_opacity=round(float(out["opacity"].double().sum()), 3), covered=round(float((1.0 - out["transmittance"].double()).sum()), 3),
               sum_w=round(float(trainer.fixed_to_weight(acc[2]).sum()), 3), owned_pixels=int((out["top_row"] >= 0).sum()),
               median_pixels=int((out["depth_median"] > 0).sum()), normalised_pixels=int((out["depth_norm"] > 0).sum()),
               device=torch.cuda.get_device_name(0))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
