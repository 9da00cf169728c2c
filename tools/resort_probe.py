"""Measures GaussianModel.resort() on the library route (gslic_morton_order + gslic_permute_rows) against the LibTorch route it replaces
(GSLIC_RESORT=torch: ~10 elementwise int64 kernels, torch.sort, 19 index + copy round trips) on the same map, same process, same device,
alternating, median of five rounds (DESIGN.md sections 3 and 8).

    python tools/resort_probe.py [--P 2000000] [--tail 0.1] [--rounds 5]

The map: P rows at SH degree 3 — 6 groups x {parameter, exp_avg, exp_avg_sq} + tie_rank = 19 arrays, 712 B per row — of which the first
P / (1 + tail) are in Morton order and the rest an appended tail in insertion order (what extend() leaves behind between two re-sorts).  Every
timed resort() starts from that same storage (restored from a snapshot outside the timed region).  Prints one JSON line: per route the device
events around resort() and the wall time the model records in sort_ms (both include the sampled box and the routes' synchronisations); the
library route a second time with the copy back as one launch instead of 19 hipMemcpyAsync (GSLIC_PERMUTE_COPY=kernel); the three parts of the library route timed
separately by device events — the sampled box (torch), gslic_morton_order, gslic_permute_rows — and the permute's achieved TB/s against the
4 x 712 B x P it moves (gather: read + write, copy back: read + write); and how many keys and permutation entries differ between the library's
exact rule and torch's device arithmetic of morton_order_device on this map (recorded, not asserted)."""
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
    ap.add_argument("--tail", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.synthetic import lidar_scene, random_scene
    assert torch.cuda.is_available(), "resort_probe needs a GPU: a time taken anywhere else says nothing"
    dev = torch.device("cuda:0")
    P, W, H = a.P, 1920, 1080
    P0 = int(round(P / (1.0 + a.tail)))
    model = trainer.GaussianModel(random_scene(P0, W, H, sh_degree=3, seed=0), dev, capacity=P, order="morton", resort_fraction=None)
    tail = lidar_scene(P - P0, W, H, sh_degree=3, seed=100)
    for n in model.NAMES:
        model._buf[n][P0:P].copy_(tail[n].to(dev).float().reshape(model._buf[n][P0:P].shape))
    model._tie[P0:P].copy_(torch.arange(P0, P, dtype=torch.int32, device=dev))
    model._rows_appended(P0, P - P0, bump_layout=False)
    g = torch.Generator(device=dev).manual_seed(0)
    for d in (model._m, model._v):          # moments with content (zeros would move as fast, but a map in training has none)
        for n in model.NAMES:
            d[n][:P].copy_(torch.randn(d[n][:P].shape, device=dev, generator=g))
    arrays = [(t, w) for _d, _n, t, w, _z in model._row_arrays()]
    row_bytes = 4 * sum(w for _t, w in arrays)
    assert row_bytes == 712 and model.P == P
    snap = [t[:P].clone() for t, _w in arrays]

    def restore():
        for (t, _w), s in zip(arrays, snap):
            t[:P].copy_(s)
        model._sorted_P = P0
        torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def resort(route, copy="memcpy"):
        os.environ["GSLIC_RESORT"] = route
        os.environ["GSLIC_PERMUTE_COPY"] = copy
        restore()
        ms, perm = timed(model.resort)
        return ms, model.sort_ms[-1], perm

    routes = {"torch": ("torch", "memcpy"), "library": ("library", "memcpy"), "library_kernel_back": ("library", "kernel")}
    results = {}
    for name, (route, copy) in routes.items():      # warm every path at the timed shape, and the results agree before anything is timed
        resort(route, copy)
        _ms, _wall, perm = resort(route, copy)
        results[name] = [t[:P].clone() for t, _w in arrays[:1]] + [arrays[-1][0][:P].clone(), perm]
    same_storage = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(results["library"][:2], results["library_kernel_back"][:2]))
    assert same_storage, "the two copy-back variants disagree"
    perm_rows_differ = int((results["library"][2] != results["torch"][2]).sum())
    ev = {k: [] for k in routes}
    wall = {k: [] for k in routes}
    for _ in range(a.rounds):
        for name, (route, copy) in routes.items():
            ms, w, _perm = resort(route, copy)
            ev[name].append(ms)
            wall[name].append(w)
    # the three parts of the library route, each between two device events
    os.environ["GSLIC_PERMUTE_COPY"] = "memcpy"
    box_ms, order_ms, permute_ms = [], [], []
    for _ in range(a.rounds):
        restore()
        xyz = model._buf["xyz"][:P]
        ms, box = timed(lambda: trainer.morton_box(xyz))
        box_ms.append(ms)
        ms, (perm32, keys) = timed(lambda: trainer.morton_order_library(xyz, box, keys=True))
        order_ms.append(ms)
        ms, _none = timed(lambda: trainer._permute_in_place(arrays, perm32, P))
        permute_ms.append(ms)
    # the library's exact rule against torch's device arithmetic (morton_order_device's expression) on the unsorted map: recorded, not asserted
    restore()
    xyz = model._buf["xyz"][:P]
    box = trainer.morton_box(xyz)
    perm32, keys = trainer.morton_order_library(xyz, box, keys=True)
    u = (((xyz - box[:3]) / (box[3:] - box[:3]).clamp_min(1e-30)).clamp(0.0, 1.0) * 1023).to(torch.int64)

    def spread(v):
        v = (v | (v << 16)) & 0x030000FF
        v = (v | (v << 8)) & 0x0300F00F
        v = (v | (v << 4)) & 0x030C30C3
        v = (v | (v << 2)) & 0x09249249
        return v
    code = spread(u[:, 0]) | (spread(u[:, 1]) << 1) | (spread(u[:, 2]) << 2)
    keys_differ = int((code[perm32.long()] != keys.long()).sum())
    med = statistics.median
    r4 = lambda xs: [round(x, 4) for x in xs]
    moved = 4.0 * row_bytes * P
    out = dict(P=P, sorted_rows=P0, tail_rows=P - P0, row_bytes=row_bytes, rounds=a.rounds,
               resort_torch_event_ms=r4(ev["torch"]), resort_torch_event_ms_median=round(med(ev["torch"]), 4),
               resort_torch_sort_ms=wall["torch"], resort_torch_sort_ms_median=med(wall["torch"]),
               resort_library_event_ms=r4(ev["library"]), resort_library_event_ms_median=round(med(ev["library"]), 4),
               resort_library_sort_ms=wall["library"], resort_library_sort_ms_median=med(wall["library"]),
               resort_library_kernel_back_event_ms=r4(ev["library_kernel_back"]),
               resort_library_kernel_back_event_ms_median=round(med(ev["library_kernel_back"]), 4),
               speedup_vs_torch=round(med(ev["torch"]) / med(ev["library"]), 2),
               box_event_ms=r4(box_ms), box_event_ms_median=round(med(box_ms), 4),
               morton_order_event_ms=r4(order_ms), morton_order_event_ms_median=round(med(order_ms), 4),
               permute_rows_event_ms=r4(permute_ms), permute_rows_event_ms_median=round(med(permute_ms), 4),
               permute_rows_moved_GB=round(moved / 1e9, 3), permute_rows_TBps=round(moved / (1e9 * med(permute_ms)), 3),
               keys_differ_from_torch_device_arithmetic=keys_differ, perm_entries_differ_from_torch_route=perm_rows_differ,
               device=torch.cuda.get_device_name(0))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
