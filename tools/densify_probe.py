"""Measures the two densification costs at the config-3 shape, in one process, alternating, median of five rounds.

    python tools/densify_probe.py [--P 2000000] [--width 1920] [--height 1080] [--grown 0.1] [--rounds 5]

(a) gslic_contribution_accumulate_error beside gslic_contribution_accumulate on the same forward of the bench scene (Morton-ordered map, identity
    camera, strict arithmetic, a seeded error image in [0, 2]), each between two device events on fresh zero accumulators.
(b) densify = gslic_densify_select + gslic_densify_emit with `grown` of the rows selected, half of them splits, against the same result built with
    torch: the selection (nonzero of the mask, the split comparison — one host synchronisation on either side), then indexing and cat over the 18
    parameter and moment tensors and the rewrite of the split parents.  Both sides are timed as ONE device-event pair around selection plus
    emission; the emission alone (library) and the index + cat alone with the selection hoisted out (torch) are reported beside it.  The torch side
    copies all P rows into fresh storage, the library writes into spare capacity — what each host really does when capacity is left.
Prints one JSON line; the two results of (b) are compared before anything is timed so that a wrong run does not pass as a fast one."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=2_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--grown", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib, trainer
    from gaussian_lic_amd import rasterizer as rz
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import random_scene
    assert torch.cuda.is_available(), "densify_probe needs a GPU: a time taken anywhere else says nothing"
    L, p = _lib.lib(), _lib.ptr
    dev = torch.device("cuda:0")
    P, W, H, M = a.P, a.width, a.height, 15
    med = statistics.median

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        del out
        return e0.elapsed_time(e1)

    # ---------------------------------------------------------------- (a) the error-weighted launch beside the plain one
    model = trainer.GaussianModel(random_scene(P, W, H, sh_degree=3, seed=0), dev, order="morton")
    cam = synthetic_camera(W, H).to_device(dev)
    fwd = trainer._RawRaster(model, cam, torch.zeros(3, device=dev))
    err = 2.0 * torch.rand(H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    acc = [torch.zeros(P, dtype=torch.int32, device=dev), torch.zeros(P, dtype=torch.int32, device=dev), torch.zeros(P, dtype=torch.int64, device=dev),
           torch.zeros(P, dtype=torch.int64, device=dev)]
    with torch.no_grad():
        fwd.forward()
    R, B, _radii, geom, binning, img, _sample = fwd.state
    plain = lambda: rz.contribution_accumulate(P, H, W, R, B, geom, binning, img, 0.05, *acc[:3])
    weighted = lambda: rz.contribution_accumulate(P, H, W, R, B, geom, binning, img, 0.05, *acc[:3], error=err, err_sum=acc[3])
    for _ in range(2):
        plain(); weighted()
    plain_ms, err_ms = [], []
    for _ in range(a.rounds):
        for t in acc:
            t.zero_()
        plain_ms.append(timed(plain))
        for t in acc:
            t.zero_()
        err_ms.append(timed(weighted))
    out = dict(P=P, W=W, H=H, R=R, rounds=a.rounds,
               contribution_event_ms=[round(x, 4) for x in plain_ms], contribution_event_ms_median=round(med(plain_ms), 4),
               contribution_error_event_ms=[round(x, 4) for x in err_ms], contribution_error_event_ms_median=round(med(err_ms), 4),
               error_over_plain=round(med(err_ms) / med(plain_ms), 3),
               sum_w=round(float(trainer.fixed_to_weight(acc[2]).sum()), 3), err_sum=round(float(trainer.fixed_to_weight(acc[3]).sum()), 3))
    del model, fwd, acc, geom, binning, img, _sample
    torch.cuda.empty_cache()

    # ---------------------------------------------------------------- (b) densify against torch indexing + cat
    g = torch.Generator(device=dev).manual_seed(0)
    widths = [3, 3, 3 * M, 1, 3, 4]
    base = [[torch.randn(P, w, device=dev, generator=g) for w in widths] for _ in range(3)]   # parameters, exp_avg, exp_avg_sq
    grow = torch.rand(P, device=dev, generator=g) < a.grown
    thr = float(base[0][4][grow].max(1).values.median())          # half of the grown rows have a component above it
    grow8 = grow.to(torch.uint8)
    parent = torch.empty(P, dtype=torch.int32, device=dev)
    count, n_split = ctypes.c_int32(0), ctypes.c_int32(0)
    stream = _lib.current_stream_ptr()

    def select():
        scratch = _lib.TensorAllocator(dev)
        _lib.check(L.gslic_densify_select(P, p(base[0][0]), p(base[0][1]), p(base[0][3]), p(base[0][4]), p(base[0][5]), p(grow8), None, None, thr,
                                          scratch.cb, None, p(parent), ctypes.byref(count), ctypes.byref(n_split), stream))
    select()
    k = count.value
    store = [[torch.empty(P + k, w, device=dev) for w in widths] for _ in range(3)]
    six = lambda d: (ctypes.c_void_p * 6)(*[t.data_ptr() for t in d])

    def refill():
        for d, s in zip(store, base):
            for t, b in zip(d, s):
                t[:P].copy_(b)

    def emit():
        _lib.check(L.gslic_densify_emit(P, k, p(parent), M, six(store[0]), six(store[1]), six(store[2]), None, thr, 7, stream))

    def torch_select():
        par = grow.nonzero().squeeze(1)
        is_split = (base[0][4][par] > thr).any(1)
        return par, is_split, par[is_split]

    def torch_way(sel=None):
        """The same map with torch ops: the selection (unless handed in), index + cat over 18 tensors and the parent rewrite (the children's positions are
        not built: the noise is not what is being timed)."""
        par, is_split, sp = sel if sel is not None else torch_select()
        res = []
        for gi, s in enumerate(base):
            grp = []
            for t in s:
                n = torch.cat([t, t[par] if gi == 0 else torch.zeros(par.numel(), t.shape[1], device=dev)])
                if gi:
                    n[sp] = 0
                grp.append(n)
            res.append(grp)
        res[0][4][sp] -= 0.4700036292457356
        res[0][4][P:][is_split] -= 0.4700036292457356
        return res

    def densify():
        select()
        emit()

    refill(); emit(); torch.cuda.synchronize()
    ref = torch_way()
    for gi in range(3):
        for wi in range(6):
            if gi == 0 and wi == 0:
                continue   # xyz: the split children's positions
            assert torch.equal(store[gi][wi].view(torch.int32), ref[gi][wi].view(torch.int32)), (gi, wi)
    del ref
    emit_ms, torch_ms, sel_ms, both_ms, torch_cat_ms = [], [], [], [], []
    hoisted = torch_select()
    for _ in range(a.rounds):
        refill()
        torch.cuda.synchronize()
        both_ms.append(timed(densify))
        torch_ms.append(timed(torch_way))
        refill()
        torch.cuda.synchronize()
        emit_ms.append(timed(emit))
        torch_cat_ms.append(timed(lambda: torch_way(hoisted)))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        select()
        sel_ms.append(1e3 * (time.perf_counter() - t0))
    out.update(densify_rows=k, densify_splits=n_split.value, grown_share=round(k / P, 4),
               densify_select_plus_emit_event_ms=[round(x, 4) for x in both_ms], densify_select_plus_emit_event_ms_median=round(med(both_ms), 4),
               densify_emit_event_ms=[round(x, 4) for x in emit_ms], densify_emit_event_ms_median=round(med(emit_ms), 4),
               densify_select_wall_ms=[round(x, 3) for x in sel_ms], densify_select_wall_ms_median=round(med(sel_ms), 3),
               torch_select_index_cat_18_event_ms=[round(x, 4) for x in torch_ms], torch_select_index_cat_18_event_ms_median=round(med(torch_ms), 4),
               torch_index_cat_18_only_event_ms=[round(x, 4) for x in torch_cat_ms], torch_index_cat_18_only_event_ms_median=round(med(torch_cat_ms), 4),
               speedup_select_plus_emit_vs_torch=round(med(torch_ms) / med(both_ms), 2),
               speedup_emit_only_vs_torch_index_cat_only=round(med(torch_cat_ms) / med(emit_ms), 2), device=torch.cuda.get_device_name(0))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
