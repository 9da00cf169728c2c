"""Measures gslic_gather_rows against the LibTorch way of pruning a map (19 boolean-index operations) on the same tensors, same process, same
device, alternating, median of five rounds.

    python tools/prune_probe.py [--P 2000000] [--removed 0.1] [--rounds 5]

The map: P rows at SH degree 3 — 6 groups x {parameter, exp_avg, exp_avg_sq} + tie_rank = 19 arrays, 712 B per row — with a random `removed`
share of the rows dropped (an ascending kept-index list, as gslic_prune_select writes it).  Prints one JSON line: the gather's time from the
library profiler (kernel time between two events on the stream) and from device events around the call, the achieved GB/s against the
2 x 712 B x P' it moves, the same for the 19 boolean-index operations (device events around all 19), and gslic_prune_select's wall time."""
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
    ap.add_argument("--removed", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    assert torch.cuda.is_available(), "prune_probe needs a GPU: a time taken anywhere else says nothing"
    L = _lib.lib()
    dev = torch.device("cuda:0")
    P, M = a.P, 15
    g = torch.Generator(device=dev).manual_seed(0)
    widths = [3, 3, 3 * M, 1, 3, 4] * 3
    srcs = [torch.randn(P, w, device=dev, generator=g) for w in widths] + [torch.randperm(P, device=dev, generator=g).to(torch.int32).reshape(P, 1)]
    row_bytes = 4 * sum(s.shape[1] for s in srcs)
    assert row_bytes == 712
    mask = torch.rand(P, device=dev, generator=g) >= a.removed
    index = mask.nonzero().squeeze(1).to(torch.int32).contiguous()
    n = int(index.numel())
    dsts = [torch.empty_like(s) for s in srcs]
    arr = (_lib.RowArray * len(srcs))(*[_lib.RowArray(s.data_ptr(), d.data_ptr(), s.shape[1]) for s, d in zip(srcs, dsts)])
    stream = _lib.current_stream_ptr()

    def gather():
        _lib.check(L.gslic_gather_rows(arr, len(srcs), _lib.ptr(index), n, stream))

    def torch_index():
        return [s[mask] for s in srcs]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        del out
        return e0.elapsed_time(e1)

    for _ in range(2):      # warm both paths at the timed shape
        gather(); torch_index()
    torch.cuda.synchronize()
    # the results agree before anything is timed
    gather()
    for s, d in zip(srcs, dsts):
        assert torch.equal(d[:n].view(torch.int32), s[mask].view(torch.int32))
    ev_gather, ev_torch, prof_gather = [], [], []
    for _ in range(a.rounds):
        ev_gather.append(timed(gather))
        ev_torch.append(timed(torch_index))
    _lib.profile_enable(True)
    for _ in range(a.rounds):
        _lib.profile_reset()
        gather()
        ms, launches = _lib.profile_collect()["gather_rows"]
        assert launches == 1
        prof_gather.append(ms)
        torch_index()
        torch.cuda.synchronize()
    _lib.profile_enable(False)
    # the selection, for the record: thresholds that remove about the same share, wall time including its one synchronisation
    t = dict(xyz=srcs[0], dc=srcs[1], opacity=srcs[3].reshape(P), scaling=srcs[4], rotation=srcs[5])
    kept = torch.empty(P, dtype=torch.int32, device=dev)
    new_tie = torch.empty(P, dtype=torch.int32, device=dev)
    count, below = ctypes.c_int32(0), ctypes.c_int32(0)
    sel = []
    for _ in range(a.rounds + 1):
        scratch = _lib.TensorAllocator(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _lib.check(L.gslic_prune_select(P, _lib.ptr(t["xyz"]), _lib.ptr(t["dc"]), _lib.ptr(t["opacity"]), _lib.ptr(t["scaling"]), _lib.ptr(t["rotation"]),
                                        -1.2816, float("inf"), 1, None, None, _lib.ptr(srcs[-1]), P // 2, scratch.cb, None, _lib.ptr(kept), _lib.ptr(new_tie),
                                        ctypes.byref(count), ctypes.byref(below), stream))
        sel.append(1e3 * (time.perf_counter() - t0))
    med = statistics.median
    moved = 2.0 * row_bytes * n
    out = dict(P=P, kept=n, removed_share=round(1.0 - n / P, 4), row_bytes=row_bytes, moved_GB=round(moved / 1e9, 3), rounds=a.rounds,
               gather_rows_profiler_ms=[round(x, 4) for x in prof_gather], gather_rows_profiler_ms_median=round(med(prof_gather), 4),
               gather_rows_event_ms=[round(x, 4) for x in ev_gather], gather_rows_event_ms_median=round(med(ev_gather), 4),
               gather_rows_GBps=round(moved / (1e6 * med(prof_gather)), 1),
               torch_bool_index_19_event_ms=[round(x, 4) for x in ev_torch], torch_bool_index_19_event_ms_median=round(med(ev_torch), 4),
               torch_bool_index_19_GBps=round(moved / (1e6 * med(ev_torch)), 1),
               speedup_vs_torch=round(med(ev_torch) / med(ev_gather), 2),
               prune_select_wall_ms=[round(x, 3) for x in sel[1:]], prune_select_kept=count.value, device=torch.cuda.get_device_name(0))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
