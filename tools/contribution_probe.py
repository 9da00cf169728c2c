"""Times gslic_contribution_accumulate at the config-3 shape against the forward blend of the same view, in the same process.

    python tools/contribution_probe.py [--P 2000000] [--width 1920] [--height 1080] [--rounds 5]

The bench scene (synthetic.random_scene, seed 0, SH degree 3) in a Morton-ordered map, identity camera, strict arithmetic.  Per round: one
raw-parameter forward with the library profiler on render_fwd (kernel time between two events on the stream), then the contribution kernel on
that forward's buffers between two device events, on fresh zero accumulators.  Both kernels walk the same lists.  Prints one JSON line with the
five times of each, their medians, the ratio, and what the view accumulated (contributing Gaussians, counted pairs, sum of the weights against
the covered pixels) so that a wrong run does not pass as a fast one."""
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
    ap.add_argument("--w-min", type=float, default=0.05)
    a = ap.parse_args()
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib, trainer
    from gaussian_lic_amd import rasterizer as rz
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import random_scene
    assert torch.cuda.is_available(), "contribution_probe needs a GPU: a time taken anywhere else says nothing"
    dev = torch.device("cuda:0")
    P, W, H = a.P, a.width, a.height
    model = trainer.GaussianModel(random_scene(P, W, H, sh_degree=3, seed=0), dev, order="morton")
    cam = synthetic_camera(W, H).to_device(dev)
    bg = torch.zeros(3, device=dev)
    fwd = trainer._RawRaster(model, cam, bg)
    acc = [torch.zeros(P, dtype=torch.int32, device=dev), torch.zeros(P, dtype=torch.int32, device=dev), torch.zeros(P, dtype=torch.int64, device=dev)]

    def kernel():
        R, B, _radii, geom, binning, img, _sample = fwd.state
        rz.contribution_accumulate(P, H, W, R, B, geom, binning, img, a.w_min, *acc)

    with torch.no_grad():
        for _ in range(2):   # warm both at the timed shape
            fwd.forward()
            kernel()
        torch.cuda.synchronize()
        blend_ms, contrib_ms = [], []
        _lib.profile_enable(True, only=["render_fwd"])
        for _ in range(a.rounds):
            for t in acc:
                t.zero_()
            _lib.profile_reset()
            image, _d, _r = fwd.forward()
            ms, launches = _lib.profile_collect()["render_fwd"]
            assert launches == 1
            blend_ms.append(ms)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            kernel()
            e1.record()
            torch.cuda.synchronize()
            contrib_ms.append(e0.elapsed_time(e1))
        _lib.profile_enable(False)
        final_T = rz.render(cam, model, bg)[1]
    med = statistics.median
    sum_w = float(trainer.fixed_to_weight(acc[2]).sum())
    out = dict(P=P, W=W, H=H, R=fwd.state[0], rounds=a.rounds, w_min=a.w_min,
               render_fwd_profiler_ms=[round(x, 4) for x in blend_ms], render_fwd_profiler_ms_median=round(med(blend_ms), 4),
               contribution_event_ms=[round(x, 4) for x in contrib_ms], contribution_event_ms_median=round(med(contrib_ms), 4),
               ratio_to_blend=round(med(contrib_ms) / med(blend_ms), 2),
               contributing_gaussians=int((acc[0] != 0).sum()), counted_pairs=int((acc[1].long() & 0xffffffff).sum()),
               sum_w=round(sum_w, 3), covered=round(float((1.0 - final_T.double()).sum()), 3), device=torch.cuda.get_device_name(0))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
