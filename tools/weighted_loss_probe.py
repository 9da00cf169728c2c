#!/usr/bin/env python
"""Timing probe: the weighted L1 + SSIM loss against the unweighted one at the config-3 image (3 x 1080 x 1920), loss launches only.
In one process, after warm-up, the variants are timed in alternating rounds with device events (ms per call, median of the rounds):
  unweighted     gslic_l1_ssim_loss_forward_backward              (two launches: forward, backward with the reduction on its first workgroup)
  weighted_ones  gslic_l1_ssim_loss_weighted_forward_backward, w == 1     (three launches: forward, reduction, backward)
  weighted_mask  the same with a random 0/1 mask that keeps half of the pixels
  fusedloss_mask FusedLoss.forward_backward(weight=mask): the three launches and the 8-byte copy into terms3
then prints the library profiler's table (ms per call and launches per call of the K_SSIM_FWD / K_SSIM_BWD classes) of each variant, which
splits a call into forward (+ reduction) and backward.
    python tools/weighted_loss_probe.py [W H rounds calls_per_round]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_lic_amd  # noqa: F401,E402
from gaussian_lic_amd import _lib, loss  # noqa: E402
from gaussian_lic_amd.synthetic import gt_image  # noqa: E402

W, H, ROUNDS, N = (int(v) for v in (sys.argv[1:5] + ["1920", "1080", "5", "200"][len(sys.argv) - 1:]))
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
gt = gt_image(H, W, seed=2).to(dev)
img = (gt + 0.05 * torch.randn(3, H, W, generator=g).to(dev)).clamp(0, 1).contiguous()
ones = torch.ones(H, W, device=dev)
mask = (torch.rand(H, W, generator=g) < 0.5).float().to(dev)
L, p = _lib.lib(), _lib.ptr
d = [torch.empty_like(img) for _ in range(4)]
partials = torch.empty(int(L.gslic_loss_partials_count(1, 3, H, W)), device=dev)
wpartials = torch.empty(int(L.gslic_l1_ssim_loss_weighted_partials_count(3, H, W)), device=dev)
terms = torch.zeros(3, device=dev)
fl = loss.FusedLoss(0.2)
print(f"W={W} H={H} rounds={ROUNDS} calls/round={N} mask keeps {float(mask.mean()):.4f} of the pixels", flush=True)


def unweighted():
    _lib.check(L.gslic_l1_ssim_loss_forward_backward(1, 3, H, W, loss.C1, loss.C2, 0.2, p(img), p(gt), p(d[0]), p(d[1]), p(d[2]), p(partials), p(terms),
                                                     p(d[3]), _lib.current_stream_ptr()))


def weighted(w):
    _lib.check(L.gslic_l1_ssim_loss_weighted_forward_backward(3, H, W, loss.C1, loss.C2, 0.2, p(img), p(gt), p(w), p(d[0]), p(d[1]), p(d[2]), p(wpartials),
                                                              p(terms), p(d[3]), _lib.current_stream_ptr()))


variants = {
    "unweighted": unweighted,
    "weighted_ones": lambda: weighted(ones),
    "weighted_mask": lambda: weighted(mask),
    "fusedloss_mask": lambda: fl.forward_backward(img, gt, mask),
}


def clock(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


for fn in variants.values():
    clock(fn, 20)
times = {k: [] for k in variants}
for r in range(ROUNDS):
    for name, fn in variants.items():
        times[name].append(clock(fn, N))
    print("round", r, " ".join(f"{k}={v[-1]:.4f}" for k, v in times.items()), flush=True)
med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
print("median ms/call:", " ".join(f"{k}={v:.4f}" for k, v in med.items()), flush=True)
print("min    ms/call:", " ".join(f"{k}={min(v):.4f}" for k, v in times.items()), flush=True)
print("weighted / unweighted (medians):", " ".join(f"{k}={med[k] / med['unweighted']:.3f}" for k in variants if k != "unweighted"), flush=True)

for name, fn in variants.items():
    clock(fn, 3)
    _lib.profile_reset()
    _lib.profile_enable(True)
    clock(fn, N)
    k = _lib.profile_collect()
    _lib.profile_enable(False)
    print(f"kernels {name} (ms/call, launches/call):", " ".join(f"{kn} {ms / N:.4f} {nl / N:.1f}" for kn, (ms, nl) in sorted(k.items()) if nl), flush=True)
