"""Training step of the hot path — mirrors optimize() (src/gaussian.cpp:640-719) and the parts of GaussianModel it
touches (getters :147-175, trainingSetup :399-418), plus the one exchange step the north star adds for N > 1 GPUs:
a single all-reduce of the Gaussian-gradient slab (+ a max-reduce of the visibility mask) per optimiser step.

One process per GPU (torch.distributed, backend "nccl" = RCCL over xGMI; "gloo" on CPU for tests).  Every rank
holds a full replica of the parameters and Adam state, renders a different camera view, and applies the identical
sparse-Adam update, so replicas stay bit-identical without a broadcast.
"""
import math
import os

import numpy as np
import torch

from . import loss as loss_utils
from .optim import SparseGaussianAdam
from .rasterizer import render

# config/fastlivo.yaml:18-22 (position, feature, opacity, scaling, rotation) and lambda_dssim
DEFAULT_LRS = dict(position_lr=1.6e-4, feature_lr=2.5e-3, opacity_lr=5e-2, scaling_lr=5e-3, rotation_lr=1e-3)
LAMBDA_DSSIM = 0.2


def morton_order(xyz, bits=10):
    """Permutation (LongTensor [P], CPU) that sorts the rows by the Morton code of their position: `bits` per axis over the robust bounding box
    (0.1 .. 99.9 percentile per axis, outliers clamped), ties in row order (stable).  View-independent: spatial neighbours become memory
    neighbours, which is what a SLAM map's insertion order gives frame by frame and a synthetic scene in random order does not."""
    import numpy as np
    q = xyz.detach().cpu().double().numpy()
    lo, hi = np.percentile(q, 0.1, axis=0), np.percentile(q, 99.9, axis=0)
    u = (np.clip((q - lo) / np.maximum(hi - lo, 1e-30), 0.0, 1.0) * ((1 << bits) - 1)).astype(np.uint64)

    def spread(v):   # 10 bits -> every third bit
        v = (v | (v << np.uint64(16))) & np.uint64(0x030000FF)
        v = (v | (v << np.uint64(8))) & np.uint64(0x0300F00F)
        v = (v | (v << np.uint64(4))) & np.uint64(0x030C30C3)
        v = (v | (v << np.uint64(2))) & np.uint64(0x09249249)
        return v
    assert bits <= 10
    code = spread(u[:, 0]) | (spread(u[:, 1]) << np.uint64(1)) | (spread(u[:, 2]) << np.uint64(2))
    return torch.from_numpy(np.argsort(code, kind="stable").astype(np.int64))


def morton_box(xyz):
    """The robust bounding box the device re-sorts quantise over, as a float32 tensor [6] = (lo xyz, hi xyz) on xyz's device: the 0.1 % / 99.9 %
    order statistics per axis of a strided sample of at most 65 536 rows (sorted per axis).  The bounds only place the quantisation grid, and
    torch.kthvalue over all rows cost 100 ms of the 103 a re-sort of 2M rows took (profiles/r06d: resort_on_device_ms).  No host read-back."""
    q = xyz.detach().float()
    P = int(q.shape[0])
    smp = q[::max(1, P // 65536)]
    srt = torch.sort(smp, dim=0).values
    n_s = int(srt.shape[0])
    return torch.cat([srt[min(n_s - 1, int(0.001 * n_s))], srt[max(0, min(n_s - 1, int(0.999 * n_s)))]]).contiguous()


def morton_order_library(xyz, box, keys=False):
    """gslic_morton_order on xyz [P,3] (float32, contiguous, on the GPU) and box [6]: the permutation as an int32 device tensor [P] (perm[s] = the old
    row that becomes row s; ascending keys, equal keys in storage order), and with keys=True also the sorted keys (int32 [P] holding the 30-bit codes).
    The key rule is exact (include/gslic_hip.h); for finite inputs and the same box it is morton_order_device's construction."""
    from . import _lib
    P = int(xyz.shape[0])
    assert xyz.dtype == torch.float32 and xyz.is_contiguous() and box.dtype == torch.float32 and box.numel() == 6 and box.is_contiguous()
    perm = torch.empty(P, dtype=torch.int32, device=xyz.device)
    ks = torch.empty(P, dtype=torch.int32, device=xyz.device) if keys else None
    scratch = _lib.TensorAllocator(xyz.device)
    _lib.check(_lib.lib().gslic_morton_order(P, _lib.ptr(xyz), _lib.ptr(box), scratch.cb, None, _lib.ptr(perm), _lib.ptr(ks), _lib.current_stream_ptr()))
    return (perm, ks) if keys else perm


def _permute_in_place(rows, perm, n):
    """a[s, :] = a[perm[s], :] for s < n and every (tensor, row_dwords) of rows, in place: ONE gslic_permute_rows through one staging tensor."""
    from . import _lib
    L = _lib.lib()
    rows = [(t, w) for t, w in rows if w]
    if not rows or not n:
        return
    arr = (_lib.RowArray * len(rows))(*[_lib.RowArray(t.data_ptr(), t.data_ptr(), w) for t, w in rows])
    nbytes = int(L.gslic_permute_rows_staging_bytes(arr, len(rows), int(n)))
    staging = torch.empty(nbytes, dtype=torch.uint8, device=perm.device)
    _lib.check(L.gslic_permute_rows(arr, len(rows), _lib.ptr(perm), int(n), _lib.ptr(staging), nbytes, _lib.current_stream_ptr()))
    # (scratch and staging go back to torch's caching allocator, which hands them out again on this same stream only: behind the launches)


def morton_order_device(xyz, bits=10):
    """morton_order with torch ops on xyz's own device (a few ms for 2M rows on the GPU: what GaussianModel.resort() runs between keyframes).
    Same construction — `bits` per axis over a robust bounding box (the 0.1 % / 99.9 % order statistics per axis), outliers clamped, ties in row
    order (stable sort) — but not necessarily the same permutation as the numpy version to the last row: any permutation renders and trains
    bit-identically (tie_rank), the order only decides how coherent memory is."""
    assert bits <= 10
    q = xyz.detach().float()
    box = morton_box(q)
    lo, hi = box[:3], box[3:]
    u = (((q - lo) / (hi - lo).clamp_min(1e-30)).clamp(0.0, 1.0) * ((1 << bits) - 1)).to(torch.int64)

    def spread(v):   # 10 bits -> every third bit
        v = (v | (v << 16)) & 0x030000FF
        v = (v | (v << 8)) & 0x0300F00F
        v = (v | (v << 4)) & 0x030C30C3
        v = (v | (v << 2)) & 0x09249249
        return v
    code = spread(u[:, 0]) | (spread(u[:, 1]) << 1) | (spread(u[:, 2]) << 2)
    return torch.sort(code, stable=True).indices


def prune_thresholds(min_opacity=None, max_scale=None):
    """The two float32 thresholds of the raw-domain keep rule (include/gslic_hip.h: gslic_prune_select) for limits given in the ACTIVATED domain:
    min_opacity in (0, 1) -> logit(min_opacity) = log(p / (1 - p)), max_scale > 0 -> log(max_scale), each computed ONCE on the host in float64 and
    rounded to float32.  None disables a threshold (-inf / +inf).  Returns (opacity_raw_min, scaling_raw_max) as Python floats holding float32
    values: a row is hit when raw opacity < opacity_raw_min or some raw scaling > scaling_raw_max (both strict)."""
    import math
    import numpy as np
    lo, hi = -math.inf, math.inf
    if min_opacity is not None:
        p = float(min_opacity)
        if not 0.0 < p < 1.0:
            raise ValueError(f"prune: min_opacity must lie in (0, 1), got {min_opacity!r}")
        lo = float(np.float32(math.log(p / (1.0 - p))))
    if max_scale is not None:
        s = float(max_scale)
        if not (s > 0.0 and math.isfinite(s)):
            raise ValueError(f"prune: max_scale must be a finite number > 0, got {max_scale!r}")
        hi = float(np.float32(math.log(s)))
    return lo, hi


def densify_threshold(split_scale):
    """The float32 threshold of the raw-domain split rule (include/gslic_hip.h: gslic_densify_select) for a limit given in the ACTIVATED domain:
    split_scale > 0 -> log(split_scale), computed once on the host in float64 and rounded to float32 (like prune_thresholds); None or +inf: no
    row splits (+inf).  A row splits when some raw scaling > the threshold (strict)."""
    import math
    import numpy as np
    if split_scale is None:
        return math.inf
    s = float(split_scale)
    if not s > 0.0:
        raise ValueError(f"densify: split_scale must be a number > 0, got {split_scale!r}")
    return math.inf if math.isinf(s) else float(np.float32(math.log(s)))


def _row_mask(t, what, who, P, dev):
    """A per-row mask argument of `who` (prune / densify) as a contiguous uint8 tensor [P] on dev, or None; anything else is a ValueError."""
    if t is None:
        return None
    t = torch.as_tensor(t, device=dev)
    if tuple(t.shape) != (P,) or t.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"{who}: {what} must be a bool / uint8 tensor of {P} rows, got {t.dtype} {tuple(t.shape)}")
    return t.to(torch.uint8).contiguous()


def _gather_into(pairs, index, n):
    """dst[k, :] = src[index[k], :] for k < n and every (src, dst, row_dwords) of pairs: ONE gslic_gather_rows (an array of width 0 is skipped)."""
    from . import _lib
    rows = [_lib.RowArray(s.data_ptr() if w else None, d.data_ptr() if w else None, w) for s, d, w in pairs]
    arr = (_lib.RowArray * len(rows))(*rows)
    _lib.check(_lib.lib().gslic_gather_rows(arr, len(rows), _lib.ptr(index), int(n), _lib.current_stream_ptr()))


class GaussianModel:
    """Parameters + activations of src/gaussian.{h,cpp} that the hot path touches, with capacity-doubling storage so that
    extend() appends rows in place instead of six torch::cat reallocations of every parameter and Adam moment per keyframe
    (densificationPostfix, gaussian.cpp:426-497)."""

    NAMES = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")   # group order of gaussian.cpp:399-418
    raw_parameter_leaves = True   # the attributes of those names are the PRE-activation leaves: rasterizer.render() may feed them to the raw-parameter node

    def __init__(self, raw, device, lambda_erank=0.0, capacity=None, scaling_scale=1.0, order="insertion", resort_fraction=0.1):
        """order = "insertion": rows in the order given (the reference's: initialize() then extend() appends).
        order = "morton": the rows are stored sorted by the Morton code of their position (morton_order): what a camera sees is then contiguous
        in memory, whole waves of the per-Gaussian kernels are invisible and skip, and the 128-byte lines of parameters and Adam moments are
        no longer shared between visible and invisible rows.  self.tie_rank[s] = original index of storage row s: the forward breaks depth
        ties by it (gslic_raster_params.tie_rank), so rendering and training are bit-identical to the insertion order; original_order() /
        io_ply.save_map() give the rows back in the original order.  Rows appended by extend() keep their insertion order behind the sorted block;
        once they make up more than `resort_fraction` of the map, extend() re-sorts the whole map on the device (resort(): a few ms between
        keyframes; None = never) — the coherence the layout is for would otherwise decay as a SLAM map grows.
        self.sort_ms: what the sorts cost (the construction's CPU sort, then the device re-sorts), for the record next to a throughput number."""
        self.sh_degree = int(raw["sh_degree"])
        self._tie = None
        self.order = order
        self.resort_fraction = resort_fraction if order == "morton" else None
        self.sort_ms = []
        import time as _time
        _t0 = _time.perf_counter()
        if order == "morton":
            perm = morton_order(raw["xyz"])
            raw = {k: (v[perm].contiguous() if (torch.is_tensor(v) and k in self.NAMES) else v) for k, v in raw.items()}
        else:
            assert order == "insertion", order
            perm = None
        self.lambda_erank = float(lambda_erank)
        self.scaling_scale = float(scaling_scale)
        self.device = device
        self.P = int(raw["xyz"].shape[0])
        cap = max(int(capacity or self.P), self.P)
        self._buf, self._m, self._v = {}, {}, {}
        for n in self.NAMES:
            src = raw[n].to(device).float()
            self._buf[n] = torch.empty((cap,) + tuple(src.shape[1:]), device=device)
            self._buf[n][:self.P].copy_(src)
            self._m[n] = torch.zeros_like(self._buf[n])
            self._v[n] = torch.zeros_like(self._buf[n])
        if perm is not None:
            self._tie = torch.empty(cap, dtype=torch.int32, device=device)
            self._tie[:self.P].copy_(perm.to(torch.int32))
            self.sort_ms.append(round(1e3 * (_time.perf_counter() - _t0), 2))   # (CPU sort + the permuted upload, once, outside any timed region)
        self._sorted_P = self.P      # rows [0, _sorted_P) are in Morton order (order == "morton")
        self.layout_version = 0      # counts the calls that replaced the storage and renumbered the rows (prune())
        self._rows_version = 0       # counts every call that changed which row is where or how many there are (prune(), extend(), resort())
        self._stats = []             # weak references to the attached ContributionStats: carried through prune() / extend() / resort()
        self.optimizer = None
        self._rebind()

    @torch.no_grad()
    def resort(self):
        """Puts ALL rows back into Morton order (order == "morton" only): parameters, both Adam moments and tie_rank are permuted together on the
        device, so the map renders, trains and exports exactly as before (tie_rank still holds every row's ORIGINAL index).  Invalidates hipGraph
        captures of nothing (addresses do not change) but any per-row state a host keeps outside the model must be permuted by the same index
        (attached ContributionStats are): returns the permutation applied (LongTensor [P] on the device; new row s = old row perm[s])."""
        assert self._tie is not None, "resort(): the model keeps its rows in insertion order"
        import time as _time
        torch.cuda.synchronize(self.device) if self.device.type == "cuda" else None
        t0 = _time.perf_counter()
        P = self.P
        if os.environ.get("GSLIC_RESORT", "library") == "torch":   # the LibTorch route (A/B: tools/resort_probe.py): ~10 elementwise kernels, torch.sort, 19 round trips
            perm = moved = morton_order_device(self._buf["xyz"][:P])
            for _d, _n, t, _w, _zero in self._row_arrays():
                t[:P] = t[:P][perm]
        else:   # the box (torch, a sample), one gslic_morton_order, ONE gslic_permute_rows over every row array: in place, addresses unchanged
            xyz = self._buf["xyz"][:P]
            moved = morton_order_library(xyz, morton_box(xyz))
            _permute_in_place([(t, w) for _d, _n, t, w, _zero in self._row_arrays()], moved, P)
            perm = moved.long()
        self._sorted_P = P
        self._rows_version += 1
        for st in self._attached_stats():
            st._permute(moved)
        self._rebind()
        torch.cuda.synchronize(self.device) if self.device.type == "cuda" else None
        self.sort_ms.append(round(1e3 * (_time.perf_counter() - t0), 2))
        return perm

    @torch.no_grad()
    def to_morton_order(self, resort_fraction=0.1):
        """Turns a model whose rows are in insertion order into a Morton-ordered one on the device: tie_rank = arange(P) (every row's original
        index is its present row), then resort().  Afterwards the model behaves as one constructed with order="morton" and grown to this map:
        extend() / densify() append behind the sorted block and re-sort past `resort_fraction` (None: never).  Returns resort()'s permutation.
        A model that already is in Morton order is only re-sorted."""
        if self._tie is None:
            self._tie = torch.empty(self.capacity, dtype=torch.int32, device=self.device)
            self._tie[:self.P].copy_(torch.arange(self.P, dtype=torch.int32, device=self.device))
        self.order = "morton"
        self.resort_fraction = resort_fraction
        return self.resort()

    @property
    def tie_rank(self):
        """int32 [P] original index of every storage row, or None when the rows are in their original order."""
        return None if self._tie is None else self._tie[:self.P]

    def original_order(self):
        """LongTensor [P]: storage rows listed in the ORIGINAL order (x[model.original_order()] un-permutes a per-row tensor x); None = identity."""
        return None if self._tie is None else torch.argsort(self._tie[:self.P].long())

    @property
    def capacity(self):
        return self._buf["xyz"].shape[0]

    def _attached_stats(self):
        """The live ContributionStats attached to this model (dead references are dropped)."""
        live = [(r, r()) for r in self._stats]
        self._stats = [r for r, st in live if st is not None]
        return [st for _r, st in live if st is not None]

    def _rebind(self):
        for n in self.NAMES:
            setattr(self, n, self._buf[n][:self.P].detach().requires_grad_(True))
        if self.optimizer is not None:
            self.optimizer.rebind(self.parameters(), [self._m[n][:self.P] for n in self.NAMES], [self._v[n][:self.P] for n in self.NAMES])

    def _row_arrays(self, include_tie=True):
        """Every per-row storage array once — the parameters, exp_avg, exp_avg_sq (NAMES order each), then tie_rank — as (owner dict or None for
        tie_rank, name, tensor [capacity, ...], row width in dwords, whether rows of new storage must start as zeros: the moments)."""
        for d in (self._buf, self._m, self._v):
            for n in self.NAMES:
                yield d, n, d[n], math.prod(d[n].shape[1:]), d is not self._buf
        if include_tie and self._tie is not None:
            yield None, "tie_rank", self._tie, 1, False

    def _adopt(self, d, n, t):   # t becomes the storage of the row array (d, n) of _row_arrays()
        if d is None:
            self._tie = t
        else:
            d[n] = t

    def _reserve(self, newP):
        if newP <= self.capacity:
            return
        cap = max(2 * self.capacity, newP)
        for d, n, old, _w, zero in list(self._row_arrays()):
            new = (torch.zeros if zero else torch.empty)((cap,) + tuple(old.shape[1:]), dtype=old.dtype, device=self.device)
            new[:self.P].copy_(old[:self.P])
            self._adopt(d, n, new)

    def _rows_appended(self, P0, k, bump_layout):
        """Rows [P0, P0 + k) were appended (extend(), densify()): the counts (bump_layout: layout_version too), the statistics, the views, the re-sort."""
        self.P = P0 + k
        if bump_layout:
            self.layout_version += 1
        self._rows_version += 1
        for st in self._attached_stats():   # appended rows have contributed to nothing yet
            st._appended(P0, k)
        self._rebind()
        if self._tie is not None and self.resort_fraction is not None and (self.P - self._sorted_P) > self.resort_fraction * self.P:
            self.resort()    # the appended tail has grown past resort_fraction of the map: Morton order again (a few ms, between keyframes)

    @torch.no_grad()
    def prune(self, min_opacity=None, max_scale=None, drop=None, protect=None, drop_nonfinite=True):
        """Removes rows from the map on the device: one gslic_prune_select (which rows stay) and one gslic_gather_rows over the 18 parameter and
        moment arrays plus tie_rank (a stable compaction).  Returns (n_removed, kept): kept is a device LongTensor [P'] holding the OLD storage
        row of every new row — per-row state a host keeps outside the model is re-aligned with x = x[kept].

        min_opacity in (0, 1) and max_scale > 0 are given in the ACTIVATED domain.  Both are converted once on the host, in float64, to
        logit(min_opacity) and log(max_scale) and each rounded to float32 (prune_thresholds); those two float32 values are the thresholds of
        the raw-domain rule, which the device evaluates with comparisons only:
            bad[i]  = any of xyz, features_dc, opacity, scaling, rotation of row i is not finite            (only if drop_nonfinite)
            hit[i]  = drop[i] or opacity[i] < logit(min_opacity) or max_j scaling[i, j] > log(max_scale)      (raw values; both strict)
            keep[i] = not bad[i] and (protect[i] or not hit[i])
        drop / protect: optional bool / uint8 [P] in STORAGE row order (protect: rows that are large by construction, a skybox; a non-finite
        row goes even when protected).  features_rest is not scanned for non-finite values.  The rule is the host's to parametrise: when to
        prune and with which limits is policy.

        The gather is out of place: it writes fresh storage of the same capacity, the model adopts it and the old storage is released.
        Afterwards P = P', tie_rank holds the kept rows' original indices re-ranked densely to 0..P'-1 (what original_order(), save_map and
        extend()'s "appended row k gets tie k" rely on), the Morton-sorted prefix ends at the kept rows below the old bound, the optimizer is
        re-bound and layout_version is incremented: anything that baked P or addresses in (GraphedStep) must be rebuilt.  If nothing is
        removed the storage is left untouched and kept = arange(P).  Works on both row orders and before training_setup().  With N > 1
        GPUs every rank calls it with identical arguments.  Attached ContributionStats are gathered with the map (the same kept index)."""
        import ctypes
        from . import _lib
        L = _lib.lib()
        dev, P = self.device, self.P
        lo, hi = prune_thresholds(min_opacity, max_scale)
        if P == 0:
            return 0, torch.empty(0, dtype=torch.int64, device=dev)
        drop, protect = _row_mask(drop, "drop", "prune", P, dev), _row_mask(protect, "protect", "prune", P, dev)
        p = _lib.ptr
        kept_index = torch.empty(P, dtype=torch.int32, device=dev)
        new_tie = torch.empty(P, dtype=torch.int32, device=dev) if self._tie is not None else None
        scratch = _lib.TensorAllocator(dev)
        count, below = ctypes.c_int32(0), ctypes.c_int32(0)
        b = self._buf
        _lib.check(L.gslic_prune_select(P, p(b["xyz"][:P]), p(b["features_dc"][:P]), p(b["opacity"][:P]), p(b["scaling"][:P]), p(b["rotation"][:P]),
                                        lo, hi, int(bool(drop_nonfinite)), p(drop), p(protect), p(self.tie_rank), int(self._sorted_P), scratch.cb, None,
                                        p(kept_index), p(new_tie), ctypes.byref(count), ctypes.byref(below), _lib.current_stream_ptr()))
        Pn = count.value
        if Pn == P:
            return 0, torch.arange(P, dtype=torch.int64, device=dev)
        arrays = list(self._row_arrays())   # (tie_rank is gathered like every other array, then replaced by the dense ranks)
        fresh = [torch.empty_like(t) for _d, _n, t, _w, _zero in arrays]
        _gather_into([(t, f, w) for (_d, _n, t, w, _zero), f in zip(arrays, fresh)], kept_index, Pn)
        for (d, n, _t, _w, _zero), f in zip(arrays, fresh):
            self._adopt(d, n, f)
        if self._tie is not None:
            self._tie[:Pn].copy_(new_tie[:Pn])
        self.P = Pn
        self._sorted_P = below.value
        self.layout_version += 1
        self._rows_version += 1
        for st in self._attached_stats():   # the statistics follow their rows: the same gather, on the same kept index
            st._gather(kept_index, Pn)
        self._rebind()
        return P - Pn, kept_index[:Pn].long()

    @torch.no_grad()
    def densify(self, grow, split_scale, protect=None, seed=0, max_new=None):
        """Clone / split densification on the device: one gslic_densify_select (which rows grow, and where their new rows go) and one
        gslic_densify_emit (the new rows of the 18 parameter and moment arrays plus tie_rank, and the split parents' rows rewritten in place).
        Returns (k, n_split, parents): k new rows of which n_split come from splits; parents is a device LongTensor [k] holding the storage row
        of the parent of new row P0 + j.

        grow / protect: bool / uint8 [P] in STORAGE row order (protect optional).  split_scale > 0 is given in the ACTIVATED domain and converted
        once on the host to the float32 of log(split_scale) (densify_threshold); the device evaluates the raw-domain rule with comparisons only:
            eligible[i] = grow[i] and not protect[i] and xyz, features_dc, opacity, scaling, rotation of row i are all finite and |rotation_i|^2 > 0 (in float32)
            split[i]    = eligible[i] and some scaling[i, j] > log(split_scale)      (raw values; strict: a row at the threshold clones)
            clone[i]    = eligible[i] and not split[i]
        Every eligible row adds one row.  A clone's new row is a bit copy of its parent with zero moments; the parent keeps everything.  A split
        (3DGS densify_and_split, N = 2) replaces the parent's row by child 0 and appends child 1: both shrink the raw scaling by (float)log(1.6)
        and are drawn from N(xyz, R diag(exp(scaling))^2 R^T) of the parent, with zero moments.  The noise is a counter generator keyed by `seed`
        and the row's ORIGINAL index, and new rows are placed in the order of their parents' original indices: a Morton-ordered and an
        insertion-ordered model of the same map densify to the same map, and so do the ranks of an N-GPU run (every rank calls it with
        identical arguments and seed).  Which rows to grow (ContributionStats.grow_mask) and when is the host's policy.

        max_new: if the number of eligible rows exceeds it, ValueError is raised before anything is changed.  Afterwards P = P0 + k, the
        optimizer is re-bound and layout_version is incremented (a GraphedStep built before must be rebuilt); attached ContributionStats get
        zeros for the new rows and for the split parents' rows; the resort_fraction rule of extend() applies.  Works on both row orders and
        before training_setup()."""
        import ctypes
        from . import _lib
        L = _lib.lib()
        dev, P0 = self.device, self.P
        thr = densify_threshold(split_scale)
        if grow is None:
            raise ValueError("densify: grow is required")
        grow, protect = _row_mask(grow, "grow", "densify", P0, dev), _row_mask(protect, "protect", "densify", P0, dev)
        if P0 == 0:
            return 0, 0, torch.empty(0, dtype=torch.int64, device=dev)
        p = _lib.ptr
        parent_index = torch.empty(P0, dtype=torch.int32, device=dev)
        scratch = _lib.TensorAllocator(dev)
        count, n_split = ctypes.c_int32(0), ctypes.c_int32(0)
        b = self._buf
        _lib.check(L.gslic_densify_select(P0, p(b["xyz"][:P0]), p(b["features_dc"][:P0]), p(b["opacity"][:P0]), p(b["scaling"][:P0]), p(b["rotation"][:P0]),
                                          p(grow), p(protect), p(self.tie_rank), thr, scratch.cb, None, p(parent_index), ctypes.byref(count),
                                          ctypes.byref(n_split), _lib.current_stream_ptr()))
        k = count.value
        if max_new is not None and k > int(max_new):
            raise ValueError(f"densify: {k} rows would be added, max_new is {int(max_new)}")
        if k == 0:
            return 0, 0, torch.empty(0, dtype=torch.int64, device=dev)
        parents = parent_index[:k].long()
        stats = self._attached_stats()
        split_rows = None
        if stats and n_split.value:   # which parents split, from the scaling the emission has not yet rewritten (the rule's own comparison)
            split_rows = parents[(self._buf["scaling"][:P0][parents] > thr).any(1)]
        self._reserve(P0 + k)
        M = self._buf["features_rest"].shape[1]

        def six(d):
            return (ctypes.c_void_p * 6)(*[(d[n].data_ptr() if d[n].numel() else None) for n in self.NAMES])
        _lib.check(L.gslic_densify_emit(P0, k, p(parent_index), M, six(self._buf), six(self._m), six(self._v),
                                        None if self._tie is None else ctypes.c_void_p(self._tie.data_ptr()), thr, int(seed) & 0xffffffff,
                                        _lib.current_stream_ptr()))
        for st in stats if split_rows is not None else ():   # child 0 has contributed to nothing yet; a clone's parent is the Gaussian it was
            st._zero_rows(split_rows)                         # (before _rows_appended: a resort there renumbers the rows)
        self._rows_appended(P0, k, bump_layout=True)
        return k, n_split.value, parents

    # gaussian.cpp:147-175
    def get_xyz(self): return self.xyz
    def get_features_dc(self): return self.features_dc
    def get_features_rest(self): return self.features_rest
    def get_opacity(self): return torch.sigmoid(self.opacity)
    def get_scaling(self): return torch.exp(self.scaling)
    def get_rotation(self): return torch.nn.functional.normalize(self.rotation)

    def parameters(self):
        """Group order of trainingSetup (gaussian.cpp:399-418)."""
        return [getattr(self, n) for n in self.NAMES]

    def training_setup(self, lrs=None):
        c = dict(DEFAULT_LRS)
        c.update(lrs or {})
        group_lrs = [c["position_lr"], c["feature_lr"], c["feature_lr"] / 20.0, c["opacity_lr"], c["scaling_lr"], c["rotation_lr"]]
        self.optimizer = SparseGaussianAdam(self.parameters(), group_lrs, eps=1e-15)
        self._rebind()
        return self.optimizer

    @torch.no_grad()
    def extend(self, camera, points, colors, depths_rsp, R_cw, t_cw, intrinsics, bg=None):
        """extend() of gaussian.cpp:499-638 for one new frame: transmittance-only render of the latest camera, GPU selection of
        the LiDAR points that land on not-yet-opaque pixels (nearest per pixel), append of the new Gaussians (+ zero Adam moments)
        in place.  points/colors [n,3], depths_rsp [n] on the device; R_cw [3,3], t_cw [3]; intrinsics = (fx, fy, cx, cy).
        Returns the number of Gaussians inserted.  Attached ContributionStats get zeros for the appended rows."""
        import ctypes
        from . import _lib
        from .rasterizer import render
        L = _lib.lib()
        dev = self.device
        bg = torch.zeros(3, device=dev) if bg is None else bg
        _img, final_T, _pts, _vis, _radii = render(camera, self, bg, no_color=True)
        n = int(points.shape[0])
        fx, fy, cx, cy = (float(v) for v in intrinsics)
        points, colors, depths_rsp = points.contiguous().float(), colors.contiguous().float(), depths_rsp.contiguous().float()
        Rc, tc = R_cw.to(dev).float().contiguous(), t_cw.to(dev).float().contiguous()
        scratch = _lib.TensorAllocator(dev)
        flags, pos, count = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int32(0)
        p = _lib.ptr
        _lib.check(L.gslic_extend_select(n, p(points), p(depths_rsp), p(Rc), p(tc), fx, fy, cx, cy, camera.image_width, camera.image_height,
                                         p(final_T.contiguous()), scratch.cb, None, ctypes.byref(flags), ctypes.byref(pos),
                                         ctypes.byref(count), _lib.current_stream_ptr()))
        k = count.value
        if k == 0:
            return 0
        P0 = self.P
        self._reserve(P0 + k)
        M = self._buf["features_rest"].shape[1]
        row = lambda name: ctypes.c_void_p(self._buf[name][P0:].data_ptr()) if self._buf[name][P0:].numel() else None
        focal = (fx + fy) / 2.0
        _lib.check(L.gslic_extend_emit(n, flags, pos, p(points), p(colors), p(depths_rsp), self.scaling_scale, focal, M, row("xyz"),
                                       row("features_dc"), row("features_rest"), row("opacity"), row("scaling"), row("rotation"),
                                       _lib.current_stream_ptr()))
        for _d, _n, t, _w, zero in self._row_arrays(include_tie=False):
            if zero:                       # new rows start with zero moments (gaussian.cpp:458-459)
                t[P0:P0 + k].zero_()
        if self._tie is not None:          # appended rows are in insertion order behind the sorted block: their original index is their row
            self._tie[P0:P0 + k].copy_(torch.arange(P0, P0 + k, dtype=torch.int32, device=dev))
        torch.cuda.current_stream().synchronize()  # scratch (flags/pos) is released on return
        self._rows_appended(P0, k, bump_layout=False)
        return k


FIXED_FRAC_BITS = 32   # sum_w of gslic_contribution_accumulate: unsigned fixed point with this many fractional bits


def weight_to_fixed(x):
    """float / float64 tensor of non-negative weights -> the int64 bit patterns of their 32.32 fixed-point values, rounded to nearest (ties to even),
    as the kernel converts a tile's partial sum.  Exact for every float32 weight in [2^-9, 2^31): such a value has no bits below 2^-32."""
    return torch.round(torch.as_tensor(x, dtype=torch.float64) * float(1 << FIXED_FRAC_BITS)).to(torch.int64)


def fixed_to_weight(q):
    """int64 tensor holding the bit patterns of unsigned 32.32 fixed-point sums -> float64 (the two 32-bit halves are converted separately,
    so a sum with bit 63 set is not read as negative; exact below 2^21, rounded to float64 above)."""
    q = torch.as_tensor(q, dtype=torch.int64)
    hi, lo = (q >> 32) & 0xffffffff, q & 0xffffffff
    return hi.to(torch.float64) + lo.to(torch.float64) / float(1 << FIXED_FRAC_BITS)


def contribution_drop_mask(max_w, n_pix, max_weight_below=None, pixels_below=None):
    """uint8 [P]: 1 where max_w < max_weight_below (float32 comparison) OR n_pix < pixels_below (integer comparison); a limit of None takes
    no part.  max_w float32 [P], n_pix integer [P].  Comparisons only: the same expression in torch on ContributionStats.max_weight() /
    .pixels() gives the same mask."""
    import numpy as np
    drop = torch.zeros(max_w.shape[0], dtype=torch.bool, device=max_w.device)
    if max_weight_below is not None:
        drop |= max_w < float(np.float32(max_weight_below))
    if pixels_below is not None:
        drop |= n_pix < int(pixels_below)
    return drop.to(torch.uint8)


def contribution_grow_mask(err_fixed, n_pix, error_above, min_pixels=None):
    """uint8 [P]: 1 where the 32.32 fixed-point error sum exceeds weight_to_fixed(error_above) (an integer comparison on the stored bits,
    unsigned: a sum with bit 63 set is above every limit) AND, with min_pixels, n_pix >= min_pixels.  err_fixed int64 [P], n_pix integer [P]."""
    lim = int(weight_to_fixed(float(error_above)))
    if lim < 0:
        raise ValueError(f"grow_mask: error_above must be >= 0, got {error_above!r}")
    err_fixed = torch.as_tensor(err_fixed, dtype=torch.int64)
    grow = (err_fixed > lim) | (err_fixed < 0)
    if min_pixels is not None:
        grow &= torch.as_tensor(n_pix).to(err_fixed.device) >= int(min_pixels)
    return grow.to(torch.uint8)


def contribution_floater_mask(free_fixed, measured_fixed, free_fraction_above, min_measured=0.0):
    """uint8 [P]: 1 where the row was measured at all (measured_fixed != 0), its measured weight reaches min_measured (measured_fixed >=
    weight_to_fixed(min_measured), an integer comparison on the stored bits, unsigned: a sum with bit 63 set reaches every limit) AND more than
    free_fraction_above of that weight lay in front of the measured surface: free_weight > float64(free_fraction_above) * measured_weight, in
    float64 through fixed_to_weight with ONE product and ONE strict comparison — a row at exactly the fraction stays.  free_fixed,
    measured_fixed int64 [P] (ContributionStats.free_fixed() / .measured_fixed()); free_fraction_above in [0, 1]."""
    frac = float(free_fraction_above)
    if not (0.0 <= frac <= 1.0):   # (a NaN fails both comparisons)
        raise ValueError(f"floater_mask: free_fraction_above must be in [0, 1], got {free_fraction_above!r}")
    lim = int(weight_to_fixed(float(min_measured)))
    if not (float(min_measured) >= 0.0) or lim < 0:
        raise ValueError(f"floater_mask: min_measured must be >= 0 and below 2^31, got {min_measured!r}")
    free_fixed = torch.as_tensor(free_fixed, dtype=torch.int64)
    measured_fixed = torch.as_tensor(measured_fixed, dtype=torch.int64).to(free_fixed.device)
    enough = ((measured_fixed >= lim) | (measured_fixed < 0)) & (measured_fixed != 0)
    return (enough & (fixed_to_weight(free_fixed) > frac * fixed_to_weight(measured_fixed))).to(torch.uint8)


def free_space_bound(depth, margin_abs, margin_rel):
    """The near-bound image ContributionStats.accumulate(free_space=...) takes, from a depth image such as camera.project_depth(points) (0 where
    no return fell): float32 [H, W], d - (margin_abs + margin_rel * d) where d > 0 and 0 elsewhere (d <= 0, NaN) — one product, one add, one
    subtraction, each a float32 torch operation in that order.  A Gaussian whose view depth is below the bound sits more than the margin in
    front of the measured surface.  Where the margin exceeds d the bound is <= 0: the pixel reads as not measured.  Plain torch, host policy."""
    if not (float(margin_abs) >= 0.0 and float(margin_rel) >= 0.0):   # (a NaN fails)
        raise ValueError(f"free_space_bound: the margins must be >= 0, got {margin_abs!r} and {margin_rel!r}")
    d = torch.as_tensor(depth).detach().to(torch.float32)
    ma = torch.tensor(float(margin_abs), dtype=torch.float32, device=d.device)
    mr = torch.tensor(float(margin_rel), dtype=torch.float32, device=d.device)
    return torch.where(d > 0, d - (ma + mr * d), torch.zeros((), dtype=torch.float32, device=d.device))


def range_weight(depth, sigma_abs, sigma_rel):
    """A relative-error weight image for the depth loss (depth_weight= of the training steps), from a depth image such as LidarDepth.resolve's:
    float32 [H, W], sigma_abs / (sigma_abs + sigma_rel * d) where d > 0 and 0 elsewhere (d <= 0, NaN) — one product, one add, one division, each a
    float32 torch operation in that order.  1 at the sensor, falling with range as a range noise sigma_abs + sigma_rel * d grows: it keeps the far
    returns of a sweep from outvoting the near structure.  sigma_abs > 0, sigma_rel >= 0.  Plain torch; which weight to use is the host's policy."""
    if not (float(sigma_abs) > 0.0 and float(sigma_rel) >= 0.0 and float(sigma_abs) < float("inf") and float(sigma_rel) < float("inf")):   # (a NaN fails)
        raise ValueError(f"range_weight: sigma_abs must be > 0 and sigma_rel >= 0, both finite, got {sigma_abs!r} and {sigma_rel!r}")
    d = torch.as_tensor(depth).detach().to(torch.float32)
    sa = torch.tensor(float(sigma_abs), dtype=torch.float32, device=d.device)
    sr = torch.tensor(float(sigma_rel), dtype=torch.float32, device=d.device)
    return torch.where(d > 0, sa / (sa + sr * d), torch.zeros((), dtype=torch.float32, device=d.device))


class LidarDepth:
    """The per-pixel LiDAR range image of one camera, built by the library (gslic_lidar_zbuffer_add / _resolve, include/gslic_hip.h): it owns the
    z-buffer of width * height 64-bit keys {float bits of camera z, point index} on `device`.

        ld = LidarDepth(W, H, device);  ld.add(camera, points_world);  out = ld.resolve(footprint=0, margins=(0.1, 0.02))
        training_step_fused(..., gt_depth=out["depth"], lambda_depth=...);  stats.accumulate(camera, free_space=out["near"])

    At footprint 0, depth is camera.project_depth(points) and near is free_space_bound(depth, *margins), bit for bit; a footprint r > 0 gives
    every pixel the NEAREST return of its (2r+1) x (2r+1) window (clipped to the image): a conservative footprint for sparse returns.  Which
    footprint and margins to use, and when to trust a sweep, is the host's policy.  Every call runs on the current stream, allocates only its
    result tensors and reads nothing back."""

    MAX_FOOTPRINT = 8

    def __init__(self, width, height, device):
        self.width, self.height = int(width), int(height)
        if self.width <= 0 or self.height <= 0:
            raise ValueError(f"LidarDepth: the image must not be empty, got {width!r} x {height!r}")
        self.device = torch.device(device)
        self._zbuf = torch.empty(self.height * self.width, dtype=torch.int64, device=self.device)
        self._pending_clear = True   # the first add clears (one memset inside the call)
        self.n_points = 0            # the running index_base: points added since the last clear

    def clear(self):
        """Empties the image: the next add() clears the z-buffer inside its call; a resolve() before any add() gives the empty image."""
        self._pending_clear = True
        self.n_points = 0

    def _add_raw(self, n, points, R_cw, t_cw, fx, fy, cx, cy):
        from . import _lib
        base = self.n_points
        _lib.check(_lib.lib().gslic_lidar_zbuffer_add(n, _lib.ptr(points), _lib.ptr(R_cw), _lib.ptr(t_cw), fx, fy, cx, cy, self.width, self.height,
                                                      _lib.ptr(self._zbuf), int(self._pending_clear), base, _lib.current_stream_ptr()))
        self._pending_clear = False
        self.n_points = base + n
        return base

    @torch.no_grad()
    def add(self, camera, points_world):
        """Adds one sweep: points_world [n,3] (world frame, on the device) seen from `camera` (its pose as project_depth forms it: R_cw = R_wc^T and
        t_cw = -R_wc^T t_wc rounded to float32; its intrinsics).  The nearest return wins a pixel, equal depths go to the lowest index.  Returns the
        index_base of this sweep: its point i is index base + i in resolve()'s index image.  Several sweeps, each with its own pose, accumulate."""
        import numpy as np
        if camera.image_width != self.width or camera.image_height != self.height:
            raise ValueError(f"LidarDepth.add: the camera is {camera.image_width} x {camera.image_height}, the image {self.width} x {self.height}")
        pts = torch.as_tensor(points_world)
        if pts.dim() != 2 or pts.shape[1] != 3 or pts.device != self.device:
            raise ValueError(f"LidarDepth.add: points_world must be [n, 3] on {self.device}, got {tuple(pts.shape)} on {pts.device}")
        pts = pts.detach().to(torch.float32).contiguous()
        R_cw = torch.from_numpy(np.ascontiguousarray(camera.R_wc.T.astype(np.float32))).to(self.device)
        t_cw = torch.from_numpy((-camera.R_wc.T @ camera.t_wc).astype(np.float32)).to(self.device)
        return self._add_raw(int(pts.shape[0]), pts, R_cw, t_cw, float(camera.fx), float(camera.fy), float(camera.cx), float(camera.cy))

    @torch.no_grad()
    def resolve(self, footprint=0, margins=None, index=False, count=False, weight=None, dist2=False):
        """The images of what was added since the last clear(), as a dict: "depth" float32 [H,W] (0 = no return in the window); with
        margins=(margin_abs, margin_rel) also "near" = depth - (margin_abs + margin_rel * depth) where measured and 0 elsewhere
        (free_space_bound's arithmetic; a bound <= 0 is kept as it is); with index=True "index" int32 [H,W] (the winning point, -1 = none); with
        count=True "n_measured", a device int32 scalar tensor holding the number of measured pixels (no read-back here).

        With dist2=True also "dist2" int32 [H,W]: the squared pixel distance from the pixel to the return it was given (0 = its own, at most
        2 footprint^2; -1 = none).  With weight=(sigma_abs, sigma_rel) or (sigma_abs, sigma_rel, falloff) (falloff defaults to 0) also "weight"
        float32 [H,W], usable as it is as depth_weight= of the training steps: range_weight(depth, sigma_abs, sigma_rel) times
        1 / (1 + falloff * dist2), 0 where nothing was measured (the rule of gslic_lidar_zbuffer_resolve_weighted; where dist2 is 0, and everywhere
        at falloff 0, range_weight's bits).  Both come out of the same single launch; with neither, the call is gslic_lidar_zbuffer_resolve's."""
        from . import _lib
        r = int(footprint)
        if not 0 <= r <= self.MAX_FOOTPRINT:
            raise ValueError(f"LidarDepth.resolve: footprint must be in [0, {self.MAX_FOOTPRINT}], got {footprint!r}")
        ma, mr = (0.0, 0.0) if margins is None else (float(margins[0]), float(margins[1]))
        if not (ma >= 0.0 and mr >= 0.0):   # (a NaN fails)
            raise ValueError(f"LidarDepth.resolve: the margins must be >= 0, got {margins!r}")
        sa, sr, fo = 1.0, 0.0, 0.0
        if weight is not None:
            if not isinstance(weight, (tuple, list)) or len(weight) not in (2, 3):
                raise ValueError(f"LidarDepth.resolve: weight must be (sigma_abs, sigma_rel) or (sigma_abs, sigma_rel, falloff), got {weight!r}")
            sa, sr, fo = float(weight[0]), float(weight[1]), (float(weight[2]) if len(weight) == 3 else 0.0)
            if not (sa > 0.0 and sr >= 0.0 and sa < float("inf") and sr < float("inf")):   # (a NaN fails; range_weight's check and words)
                raise ValueError(f"LidarDepth.resolve: sigma_abs must be > 0 and sigma_rel >= 0, both finite, got {weight[0]!r} and {weight[1]!r}")
            if not (fo >= 0.0 and fo < float("inf")):
                raise ValueError(f"LidarDepth.resolve: the falloff must be >= 0 and finite, got {weight[2]!r}")
        if self._pending_clear:
            self._add_raw(0, None, None, None, 0.0, 0.0, 0.0, 0.0)
        H, W, dev = self.height, self.width, self.device
        out = {"depth": torch.empty(H, W, dtype=torch.float32, device=dev)}
        if margins is not None:
            out["near"] = torch.empty(H, W, dtype=torch.float32, device=dev)
        if index:
            out["index"] = torch.empty(H, W, dtype=torch.int32, device=dev)
        if count:
            out["n_measured"] = torch.empty((), dtype=torch.int32, device=dev)
        if weight is not None:
            out["weight"] = torch.empty(H, W, dtype=torch.float32, device=dev)
        if dist2:
            out["dist2"] = torch.empty(H, W, dtype=torch.int32, device=dev)
        p = lambda k: _lib.ptr(out.get(k))
        if weight is None and not dist2:
            _lib.check(_lib.lib().gslic_lidar_zbuffer_resolve(W, H, _lib.ptr(self._zbuf), r, ma, mr, p("depth"), p("index"), p("near"), p("n_measured"),
                                                              _lib.current_stream_ptr()))
        else:
            _lib.check(_lib.lib().gslic_lidar_zbuffer_resolve_weighted(W, H, _lib.ptr(self._zbuf), r, ma, mr, sa, sr, fo, p("depth"), p("index"),
                                                                       p("near"), p("n_measured"), p("weight"), p("dist2"),
                                                                       _lib.current_stream_ptr()))
        return out


def lidar_depth_image(camera, points, footprint=0):
    """camera.project_depth(points) through the library, for points on a GPU: one sweep into a fresh LidarDepth, its depth image [H,W] at the given
    footprint (0: bit for bit project_depth's image)."""
    ld = LidarDepth(camera.image_width, camera.image_height, torch.as_tensor(points).device)
    ld.add(camera, points)
    return ld.resolve(footprint=footprint)["depth"]


class _RowStatistics:
    """What GaussianModel's row changes walk on an attached per-row statistics object (a weak reference in model._stats): _gather (prune), _appended
    (extend / densify), _zero_rows (densify's split parents), _permute (resort), on the arrays a subclass lists in _arrays() and creates, zero-filled
    and sized to the model's capacity, in _alloc(cap).  detach() ends the carriage; a detached object raises from _check() once the rows have changed."""

    def __init__(self, model):
        self.model = model
        self._alloc(model.capacity)
        self._attached = True
        self._sync()
        import weakref
        model._stats.append(weakref.ref(self))

    def _sync(self):
        self._seen = (self.model.layout_version, self.model._rows_version, self.model.P)

    def _check(self):
        now = (self.model.layout_version, self.model._rows_version, self.model.P)
        if now != self._seen:
            name = type(self).__name__
            raise RuntimeError(f"{name}: the model's rows changed since these statistics were taken (layout_version / row changes / P "
                               f"{self._seen} -> {now}: prune(), extend() or resort()) and this object was detached, so it was not carried along — "
                               f"its rows no longer are the model's; build a new {name}")

    def detach(self):
        """The model stops carrying this object through prune() / extend() / resort(); it stays readable until the rows change."""
        self._attached = False
        self.model._stats = [r for r in self.model._stats if r() is not None and r() is not self]

    # --- what the model calls (attached objects only)
    def _gather(self, kept_index, Pn):
        old = self._arrays()
        self._alloc(self.model.capacity)    # fresh and zero: the rows behind Pn stay zero
        if Pn:
            _gather_into([(o, n, w) for (o, w), (n, _w) in zip(old, self._arrays())], kept_index, Pn)
        self._sync()

    def _appended(self, P0, k):
        if self._arrays()[0][0].shape[0] < self.model.capacity:
            old = self._arrays()
            self._alloc(self.model.capacity)
            for (o, _w), (n, _w2) in zip(old, self._arrays()):
                n[:P0].copy_(o[:P0])
        else:
            for a, _w in self._arrays():
                a[P0:P0 + k].zero_()
        self._sync()

    def _zero_rows(self, rows):
        """densify(): the rows of split parents now hold child 0, which has contributed to nothing yet."""
        for a, _w in self._arrays():
            a[rows] = 0
        self._sync()

    def _permute(self, perm):
        """resort(): int32 perm = the library route (one gslic_permute_rows over the accumulators), int64 = torch indexing (GSLIC_RESORT=torch)."""
        P = perm.shape[0]
        if perm.dtype == torch.int32:
            _permute_in_place(self._arrays(), perm, P)
        else:
            for a, _w in self._arrays():
                a[:P] = a[:P][perm]
        self._sync()


class ContributionStats(_RowStatistics):
    """Per-Gaussian contribution statistics accumulated over views (gslic_contribution_accumulate, include/gslic_hip.h): for every storage row
    the largest blend weight w = alpha T it reached in a pixel, the number of (pixel, view) pairs where w >= w_min, and the sum of w — what a
    mapper decides by whether a Gaussian ever contributes, which raw opacity and scale do not say.  When to accumulate, over which keyframes
    and with which limits to prune is the host's policy.

    The object owns three device arrays sized to the model's capacity, zero-filled, and ATTACHES itself to the model (a weak reference):
    model.prune() gathers them with the map, model.extend() gives appended rows zeros, model.resort() permutes them.  detach() ends that; a
    detached object raises from every accessor once the model's rows have changed instead of indexing the wrong rows."""

    W_MIN = 0.05   # default of accumulate(): a pair counts into pixels() when the Gaussian supplies at least 5 % of the pixel

    def __init__(self, model):
        self._err = None             # the error accumulator: allocated by the first accumulate with an error image
        self._free = None            # the two free-space accumulators: allocated by the first accumulate with a near-bound image
        self._meas = None
        self.views = 0
        super().__init__(model)

    def _alloc(self, cap):
        dev = self.model.device
        self._max = torch.zeros(cap, dtype=torch.int32, device=dev)    # uint32 [cap]: float bits
        self._npix = torch.zeros(cap, dtype=torch.int32, device=dev)   # uint32 [cap]
        self._sum = torch.zeros(cap, dtype=torch.int64, device=dev)    # uint64 [cap]: 32.32 fixed point
        self._err = torch.zeros(cap, dtype=torch.int64, device=dev) if self._err is not None else None   # uint64 [cap], lazily
        if self._free is not None:                                     # uint64 [cap] each, lazily and together
            self._free = torch.zeros(cap, dtype=torch.int64, device=dev)
            self._meas = torch.zeros(cap, dtype=torch.int64, device=dev)

    def _arrays(self):
        """The accumulators that exist, with their row widths in dwords."""
        a = [(self._max, 1), (self._npix, 1), (self._sum, 2)]
        a += [(self._err, 2)] if self._err is not None else []
        return a + ([(self._free, 2), (self._meas, 2)] if self._free is not None else [])

    # --- accumulation
    @torch.no_grad()
    def accumulate(self, camera, bg=None, w_min=None, error=None, free_space=None):
        """Renders `camera` (a forward of its own, raw parameters, no autograd) and adds that view's statistics.  error, free_space: see
        accumulate_from."""
        self._check()
        if self.model.P == 0:
            self.views += 1
            return
        bg = torch.zeros(3, device=self.model.device) if bg is None else bg
        fwd = _RawRaster(self.model, camera, bg)
        fwd.forward()
        self.accumulate_from(fwd, w_min, error=error, free_space=free_space)

    @torch.no_grad()
    def accumulate_from(self, fwd, w_min=None, error=None, free_space=None):
        """Adds the statistics of a forward the caller already has: a _RawRaster after forward() (training_step_fused's pieces) or the
        rasterizer.CapacityBuffers a capacity forward filled (GraphedStep.bufs: the launch is sized from the capacities, stops at the real
        counts on the device and does nothing when the forward's status says the lists did not fit).  The forward must be of THIS model's rows.
        error: an [H, W] float device tensor, the view's per-pixel error (host policy, plain torch: (image - gt).abs().mean(0)).  The launch is
        then gslic_contribution_accumulate_error: the same statistics, and error_sum() += sum of w e(p) with e = error clamped to [0, 4]
        (NaN and negative values read as 0).  The fourth accumulator is allocated at the first such call; without `error` it does not exist.
        free_space: an [H, W] float device tensor, the view's near bound in view-space depth units (free_space_bound() of a LiDAR depth image;
        a pixel is measured where it is > 0).  The launch is then gslic_contribution_accumulate_free_space: the same statistics, and
        measured_weight() += sum of w over the measured pixels, free_weight() += sum of w over the measured pixels the Gaussian lies in front
        of (view depth < bound).  Its two accumulators are allocated at the first such call.  With error AND free_space the view takes two
        launches: the error launch with the three base statistics, then the free-space launch without them — nothing is counted twice."""
        from . import rasterizer as rz
        self._check()
        w_min = self.W_MIN if w_min is None else float(w_min)
        if isinstance(fwd, rz.CapacityBuffers):
            if fwd.no_color:
                raise ValueError("ContributionStats: a no_color forward stores no n_contrib")
            P, H, W, R, B, geom, binning, img = fwd.P, fwd.H, fwd.W, fwd.cap_R, fwd.cap_B, fwd.geom, fwd.binning, fwd.img
        else:
            if fwd.state is None:
                raise ValueError("ContributionStats: run forward() on the _RawRaster first")
            R, B, _radii, geom, binning, img, _sample = fwd.state
            P, (H, W) = fwd.xyz.shape[0], fwd.hw
        if P != self.model.P:
            raise ValueError(f"ContributionStats: the forward rendered {P} rows, the model has {self.model.P}")
        for name, t in (("error", error), ("free_space", free_space)):   # both validated before either launch
            if t is None:
                continue
            t = torch.as_tensor(t)
            if tuple(t.shape) != (int(H), int(W)) or not t.is_floating_point() or t.device != self._max.device:
                raise ValueError(f"ContributionStats: {name} must be a float [{int(H)}, {int(W)}] tensor on the model's device, got {t.dtype} "
                                 f"{tuple(t.shape)} on {t.device}")
        base = (self._max, self._npix, self._sum)
        if error is None and free_space is None:
            rz.contribution_accumulate(P, H, W, R, B, geom, binning, img, w_min, *base)
        if error is not None:
            if self._err is None:
                self._err = torch.zeros(self._max.shape[0], dtype=torch.int64, device=self._max.device)
            rz.contribution_accumulate(P, H, W, R, B, geom, binning, img, w_min, *base,
                                       error=torch.as_tensor(error).detach().float().contiguous(), err_sum=self._err)
            base = (None, None, None)   # the free-space launch of the same view leaves them alone
        if free_space is not None:
            if self._free is None:
                self._free = torch.zeros(self._max.shape[0], dtype=torch.int64, device=self._max.device)
                self._meas = torch.zeros(self._max.shape[0], dtype=torch.int64, device=self._max.device)
            rz.contribution_accumulate(P, H, W, R, B, geom, binning, img, w_min, *base,
                                       near_bound=torch.as_tensor(free_space).detach().float().contiguous(), free_sum=self._free, meas_sum=self._meas)
        self.views += 1

    def reset(self):
        self._check()
        for a, _w in self._arrays():
            a.zero_()
        self.views = 0

    # --- results, [P] in storage row order
    def max_weight(self):
        """float32 [P]: the largest w = alpha T the row reached in any pixel of any accumulated view (0: it never contributed)."""
        self._check()
        return self._max[:self.model.P].view(torch.float32)

    def pixels(self):
        """int64 [P]: the (pixel, view) pairs in which the row's w reached w_min (saturating at 2^32 - 1)."""
        self._check()
        return self._npix[:self.model.P].long() & 0xffffffff

    def sum_fixed(self):
        """int64 [P]: the bit patterns of the 32.32 fixed-point sums of w (what is compared bit for bit)."""
        self._check()
        return self._sum[:self.model.P]

    def sum_weight(self):
        """float64 [P]: the sum of w over every contributing (pixel, view) pair of the row."""
        return fixed_to_weight(self.sum_fixed())

    def mean_weight(self):
        """float64 [P]: sum_weight() / pixels(), 0 where pixels() is 0 — the mean weight per counted pair when the views were accumulated with
        w_min = 0 (every contributing pair is counted); with a larger w_min the numerator still holds the pairs below it."""
        n = self.pixels()
        return torch.where(n > 0, self.sum_weight() / n.clamp_min(1).to(torch.float64), torch.zeros((), dtype=torch.float64, device=n.device))

    def error_fixed(self):
        """int64 [P]: the bit patterns of the 32.32 fixed-point sums of w e(p) (zeros before the first accumulate with an error image)."""
        self._check()
        if self._err is None:
            return torch.zeros(self.model.P, dtype=torch.int64, device=self._max.device)
        return self._err[:self.model.P]

    def error_sum(self):
        """float64 [P]: the sum of w e(p) over every contributing (pixel, view) pair of the row — the error-based densification score."""
        return fixed_to_weight(self.error_fixed())

    def grow_mask(self, error_above, min_pixels=None):
        """The uint8 [P] mask model.densify(grow=...) takes: contribution_grow_mask on error_fixed() and pixels()."""
        return contribution_grow_mask(self.error_fixed(), self.pixels(), error_above, min_pixels)

    def free_fixed(self):
        """int64 [P]: the bit patterns of the 32.32 fixed-point sums of w over the measured pixels the row lies in front of (zeros before the
        first accumulate with a near-bound image)."""
        self._check()
        if self._free is None:
            return torch.zeros(self.model.P, dtype=torch.int64, device=self._max.device)
        return self._free[:self.model.P]

    def measured_fixed(self):
        """int64 [P]: the bit patterns of the 32.32 fixed-point sums of w over the measured pixels (zeros before the first such accumulate)."""
        self._check()
        if self._meas is None:
            return torch.zeros(self.model.P, dtype=torch.int64, device=self._max.device)
        return self._meas[:self.model.P]

    def free_weight(self):
        """float64 [P]: the blend weight the row carried in front of the measured surface — in known free space."""
        return fixed_to_weight(self.free_fixed())

    def measured_weight(self):
        """float64 [P]: the blend weight the row carried in pixels with a measurement."""
        return fixed_to_weight(self.measured_fixed())

    def floater_mask(self, free_fraction_above, min_measured=0.0):
        """The uint8 [P] mask model.prune(drop=...) takes: contribution_floater_mask on free_fixed() and measured_fixed()."""
        return contribution_floater_mask(self.free_fixed(), self.measured_fixed(), free_fraction_above, min_measured)

    def drop_mask(self, max_weight_below=None, pixels_below=None):
        """The uint8 [P] mask model.prune(drop=...) takes: contribution_drop_mask on max_weight() and pixels()."""
        return contribution_drop_mask(self.max_weight(), self.pixels(), max_weight_below, pixels_below)


GEOMETRY_DEFAULT = ("opacity", "depth_norm", "depth_median", "top_row")


@torch.no_grad()
def geometry_images(model, camera, bg=None, a_min=0.05, what=GEOMETRY_DEFAULT, out=None):
    """Per-pixel geometry of one view (gslic_geometry_images, include/gslic_hip.h) as a dict of [H, W] device tensors: renders `camera` (a forward
    of its own, raw parameters, no autograd — the training step is not touched) and replays its lists.  what: any of "transmittance" (the
    forward's final_T), "opacity" (A = sum of w = alpha T), "depth_sum" (render(return_depth=True)'s D = sum T alpha z), "depth_norm" (D / A where
    A >= a_min, 0 elsewhere), "depth_median" (the view depth of the entry that takes T below one half; 0: never reached), "top_row" (int32: the
    STORAGE row of the largest w, -1: no contributor) and "top_weight" (that w).  out: see geometry_images_from.  Which a_min to use and what to
    do with the images is the host's policy."""
    H, W = int(camera.image_height), int(camera.image_width)
    if model.P == 0:   # nothing to render: the rule's initial values, from the same launch
        from . import rasterizer as rz
        res = _geometry_out(H, W, model.device, what, out)
        rz.geometry_images(0, H, W, 0, 0, None, None, None, _geometry_a_min(a_min, res), res)
        return res
    bg = torch.zeros(3, device=model.device) if bg is None else bg
    fwd = _RawRaster(model, camera, bg)
    fwd.forward()
    return geometry_images_from(fwd, a_min=a_min, what=what, out=out)


def _geometry_a_min(a_min, res):
    a_min = float(a_min)
    if "depth_norm" in res and not a_min > 0.0:   # (a NaN fails)
        raise ValueError(f"geometry_images: a_min must be > 0 for depth_norm, got {a_min!r}")
    return a_min


def _geometry_out(H, W, device, what, out):
    """The dict of images a geometry call writes, one per name in `what`: out's tensors, or fresh ones."""
    from . import rasterizer as rz
    names = tuple(what)
    unknown = set(names) - set(rz.GEOMETRY_IMAGES)
    if unknown:
        raise ValueError(f"geometry_images: unknown image(s) {sorted(unknown)}; the images are {rz.GEOMETRY_IMAGES}")
    if out is not None:
        missing = [n for n in names if out.get(n) is None]
        if missing:
            raise ValueError(f"geometry_images: out= has no tensor for {missing}")
        return {n: out[n] for n in names}
    return {n: torch.empty(H, W, dtype=torch.int32 if n == "top_row" else torch.float32, device=device) for n in names}


@torch.no_grad()
def geometry_images_from(fwd, a_min=0.05, what=GEOMETRY_DEFAULT, out=None):
    """geometry_images of a forward the caller already has: a _RawRaster after forward() (training_step_fused's pieces) or the
    rasterizer.CapacityBuffers a capacity forward filled (GraphedStep.bufs: the launch is sized from the capacities, stops at the real counts on
    the device and writes NOTHING when the forward's status says the lists did not fit).  A colour-only and a depth forward give the same images.
    out: a dict of preallocated contiguous [H, W] device tensors (float32, top_row int32) keyed by image name — the call then allocates nothing
    and can sit in a captured graph; `what` names the images computed (each must be in out).  Returns the dict of images."""
    from . import rasterizer as rz
    if isinstance(fwd, rz.CapacityBuffers):
        if fwd.no_color:
            raise ValueError("geometry_images: a no_color forward stores no n_contrib")
        P, H, W, R, B, geom, binning, img = fwd.P, fwd.H, fwd.W, fwd.cap_R, fwd.cap_B, fwd.geom, fwd.binning, fwd.img
    else:
        if fwd.state is None:
            raise ValueError("geometry_images: run forward() on the _RawRaster first")
        R, B, _radii, geom, binning, img, _sample = fwd.state
        P, (H, W) = fwd.xyz.shape[0], fwd.hw
    res = _geometry_out(int(H), int(W), geom.device, what, out)
    rz.geometry_images(P, H, W, R, B, geom, binning, img, _geometry_a_min(a_min, res), res)
    return res


def rows_under(top_row, mask, P=None):
    """bool [P]: the storage rows that own at least one pixel where `mask` is true — top_row: geometry_images' int32 [H, W] image, mask: bool (or
    any tensor read as != 0) [H, W] on the same device; a pixel without a contributor (-1) names no row.  P: the number of rows (the model's P;
    default: the largest row named + 1).  Plain torch; usable as it is as drop= / protect= of prune() and grow= / protect= of densify()."""
    top_row, mask = torch.as_tensor(top_row), torch.as_tensor(mask)
    if top_row.shape != mask.shape:
        raise ValueError(f"rows_under: top_row is {tuple(top_row.shape)}, mask {tuple(mask.shape)}")
    rows = top_row[(mask != 0) & (top_row >= 0)].long()
    n = int(P) if P is not None else (int(top_row.max()) + 1 if top_row.numel() else 0)
    owned = torch.zeros(max(n, 0), dtype=torch.bool, device=top_row.device)
    owned[rows] = True
    return owned


def gradient_grow_mask(grad_sum, n_seen, grad_above, min_seen=1):
    """uint8 [P]: 1 where n_seen >= max(min_seen, 1) and grad_sum >= float32(grad_above) * float32(n_seen) — the 3DGS test "mean gradient >=
    threshold" without the division: comparisons and ONE float32 product, so the same expression in torch or numpy gives the same mask.  3DGS's
    >= is kept.  A NaN in grad_sum (or a NaN threshold) compares false: the row does not grow.  grad_sum float32 [P], n_seen integer [P]."""
    import numpy as np
    thr = torch.tensor(float(np.float32(grad_above)), dtype=torch.float32, device=grad_sum.device)
    n = torch.as_tensor(n_seen).to(grad_sum.device)
    return ((n >= max(int(min_seen), 1)) & (grad_sum >= thr * n.to(torch.float32))).to(torch.uint8)


class GradientStats(_RowStatistics):
    """The densification statistics of 3DGS accumulated over views, on every training path (the rule: include/gslic_hip.h, gslic_grad_stats): per
    storage row the sum of the norms of the view-space positional gradient dL/dmean2D (xyz_gradient_accum), the number of views that added one
    (denom) and the largest screen radius (max_radii2D).  Pass the object as grad_stats= to training_step_fused / training_step /
    training_step_with_pose / GraphedStep: the fused Adam backward accumulates inside its per-Gaussian kernel (the gradient never leaves it), the
    other paths hand their dL_dmeans2D to one small kernel.  When to densify or reset, and with which thresholds, is the host's policy.

    Like ContributionStats the object owns its device arrays (sized to the model's capacity, zero-filled) and ATTACHES itself to the model:
    prune() gathers them, extend() / densify() give new rows and split parents zeros, resort() permutes them; detach() ends that and a detached
    object raises once the rows have changed.  Single GPU: under N > 1 ranks the steps refuse it (summing across ranks is not done)."""

    def _alloc(self, cap):
        dev = self.model.device
        self._sum = torch.zeros(cap, dtype=torch.float32, device=dev)     # float32 [cap]
        self._seen_n = torch.zeros(cap, dtype=torch.int32, device=dev)    # uint32 [cap]
        self._maxr = torch.zeros(cap, dtype=torch.int32, device=dev)      # int32 [cap]
        self._m2d = None                                                  # [P,3] scratch of the paths that materialise dL_dmeans2D

    def _arrays(self):
        return [(self._sum, 1), (self._seen_n, 1), (self._maxr, 1)]

    def _descriptor(self):
        """The gslic_grad_stats of the arrays as they are now (what a fused backward takes)."""
        from . import rasterizer as rz
        self._check()
        return rz.grad_stats_descriptor(self._sum, self._seen_n, self._maxr, self.model.P)

    def _mean2d_buffer(self):
        """float32 [P,3] the unfused paths let their backward write dL_dmeans2D into (kept: no allocation per step)."""
        P = self.model.P
        if self._m2d is None or self._m2d.shape[0] != P:
            self._m2d = torch.empty(P, 3, dtype=torch.float32, device=self.model.device)
        return self._m2d

    def _addresses(self):
        return tuple(a.data_ptr() for a, _w in self._arrays())

    @torch.no_grad()
    def accumulate_from(self, dL_dmean2D, radii, rows=None):
        """Adds one view from a dL_dmeans2D [P,3] and radii [P] the caller has (screenspace_points.grad of the operator path, the first result of
        rasterize_gaussians_backward): one gslic_gradient_stats_accumulate on rows [rows[0], rows[1]) or all.  The tensors must be of THIS model's rows."""
        from . import rasterizer as rz
        self._check()
        P = self.model.P
        if tuple(dL_dmean2D.shape) != (P, 3) or tuple(radii.shape) != (P,):
            raise ValueError(f"GradientStats: expected dL_dmean2D [{P}, 3] and radii [{P}], got {tuple(dL_dmean2D.shape)} and {tuple(radii.shape)}")
        if P == 0:
            return
        rz.gradient_stats_accumulate(dL_dmean2D.detach().float().contiguous(), radii.to(torch.int32).contiguous(), self._sum, self._seen_n, self._maxr, rows)

    def reset(self):
        self._check()
        for a, _w in self._arrays():
            a.zero_()

    # --- results, [P] in storage row order
    def grad_sum(self):
        """float32 [P]: the sum of |dL/dmean2D| over the views that saw the row (3DGS: xyz_gradient_accum)."""
        self._check()
        return self._sum[:self.model.P]

    def n_seen(self):
        """int64 [P]: how many views added a (finite) norm (3DGS: denom)."""
        self._check()
        return self._seen_n[:self.model.P].long() & 0xffffffff

    def max_radius(self):
        """int32 [P]: the largest screen radius of the row in any accumulated view (3DGS: max_radii2D); 0: never visible."""
        self._check()
        return self._maxr[:self.model.P]

    def mean_gradient(self):
        """float32 [P]: grad_sum / n_seen, 0 where the row was never seen."""
        n = self.n_seen()
        return torch.where(n > 0, self.grad_sum() / n.clamp_min(1).to(torch.float32), torch.zeros((), dtype=torch.float32, device=n.device))

    def grow_mask(self, grad_above, min_seen=1):
        """The uint8 [P] mask model.densify(grow=...) takes: gradient_grow_mask on grad_sum() and n_seen()."""
        return gradient_grow_mask(self.grad_sum(), self.n_seen(), grad_above, min_seen)

    def big_mask(self, max_screen_radius):
        """The uint8 [P] mask model.prune(drop=...) takes for 3DGS's screen-size prune: max_radius() > max_screen_radius (integer comparison)."""
        return (self.max_radius() > int(max_screen_radius)).to(torch.uint8)


def _grad_stats_for_step(grad_stats, model):
    """The checks every step makes on its grad_stats= argument (None passes): this model's object, its rows current, one GPU."""
    if grad_stats is None:
        return None
    if not isinstance(grad_stats, GradientStats) or grad_stats.model is not model:
        raise ValueError("grad_stats must be a GradientStats of the model that is trained")
    if _dist_on():
        raise NotImplementedError("grad_stats is single-GPU only: the statistics of the ranks' views are not summed across ranks")
    grad_stats._check()
    return grad_stats


COVIS_MAX_FRAMES = 1024        # GSLIC_COVIS_MAX_FRAMES
COVIS_MAX_PAIR_FRAMES = 128    # GSLIC_COVIS_MAX_PAIR_FRAMES


class Covisibility(_RowStatistics):
    """Covisibility sets: which keyframes see which Gaussians, on the device (the rule: include/gslic_hip.h, gslic_covis_*).  One bit per (row,
    frame) in int32 [capacity, Wd] rows, Wd = ceil(n_frames / 32): bit f of a row says "frame f, when it was last recorded, had radii > 0 on this
    row".  record() REPLACES a frame's column, so the state is a function of each frame's last record.  GraphedStep(keyframes=, covis=) records
    the trained slot's column behind its backward; a host without a store calls record(frame, gs.visible) or record(frame, radii).

    Signals only: which keyframe to give up (redundant), which window to train (frame_counts / overlap) and which rows to protect
    (seen_by_fewer_than) stay the host's policy.

    Like the other statistics the object owns its device array (sized to the model's capacity, zero-filled) and ATTACHES itself to the model:
    prune() gathers it, extend() / densify() give new rows and split parents zeros, resort() permutes it — the bits are one more row array of
    run-time width, carried by the same row kernels; detach() ends that and a detached object raises once the rows have changed.  Single GPU."""

    def __init__(self, model, n_frames):
        if _dist_on():
            raise NotImplementedError("Covisibility is single-GPU only: the records of the ranks' views are not merged across ranks")
        F = int(n_frames)
        if not 1 <= F <= COVIS_MAX_FRAMES:
            raise ValueError(f"Covisibility: n_frames = {n_frames} is outside 1 .. {COVIS_MAX_FRAMES}")
        self.n_frames, self.words = F, (F + 31) // 32
        self._word = torch.zeros(1, dtype=torch.int32, device=model.device)   # the frame word of the calls that name their frame by a host int
        super().__init__(model)

    def _alloc(self, cap):
        self._bits = torch.zeros(cap, self.words, dtype=torch.int32, device=self.model.device)   # uint32 [cap, Wd]

    def _arrays(self):
        return [(self._bits, self.words)]

    def _index(self, frame):
        f = int(frame)
        if not 0 <= f < self.n_frames:
            raise IndexError(f"Covisibility: frame {frame} is outside [0, {self.n_frames})")
        return f

    def _frame_word(self, frame):
        """The device int32 [1] a call reads its frame from: a device word as it is (a value outside [0, n_frames) makes record() a no-op and the
        queries return zeros), a host int validated and written into the object's own word (stream-ordered in front of the launch)."""
        if torch.is_tensor(frame):
            if frame.dtype != torch.int32 or frame.numel() != 1 or frame.device != self._bits.device:
                raise ValueError(f"Covisibility: a frame word must be one int32 on {self._bits.device}, got {frame.dtype} {tuple(frame.shape)} on {frame.device}")
            return frame
        self._word.fill_(self._index(frame))
        return self._word

    def _record(self, word, radii=None, visible=None, skip=None, rows=None):
        """One gslic_covis_record on the rows as they are (no checks of the tensors: record() and GraphedStep make them)."""
        from . import _lib
        P = self.model.P
        if P == 0:
            return
        b, e = (0, -1) if rows is None else (int(rows[0]), int(rows[1]))
        _lib.check(_lib.lib().gslic_covis_record(P, self.n_frames, self._bits.data_ptr(), _lib.ptr(radii), _lib.ptr(visible), _lib.ptr(word), _lib.ptr(skip),
                                                 b, e, _lib.current_stream_ptr()))

    @torch.no_grad()
    def record(self, frame, seen, rows=None):
        """Replaces column `frame` (an int, or a device int32 word) by `seen`: radii (int32 [P]: seen where > 0) or a visibility mask (bool / uint8
        [P]), of THIS model's rows; None clears the column.  rows = (begin, end): only those rows.  One launch, no read-back."""
        self._check()
        word = self._frame_word(frame)
        if seen is None:
            return self._record(word, rows=rows)
        P = self.model.P
        if not torch.is_tensor(seen) or tuple(seen.shape) != (P,) or seen.dtype not in (torch.int32, torch.bool, torch.uint8) or seen.device != self._bits.device:
            raise ValueError(f"Covisibility.record: seen must be radii (int32) or a visibility mask (bool / uint8) of {P} rows on {self._bits.device}, got "
                             f"{getattr(seen, 'dtype', type(seen))} {tuple(getattr(seen, 'shape', ()))}")
        seen = seen.contiguous()
        if seen.dtype == torch.int32:
            return self._record(word, radii=seen, rows=rows)
        self._record(word, visible=seen.view(torch.uint8) if seen.dtype == torch.bool else seen, rows=rows)

    def clear(self, frame):
        """Clears column `frame` (what a replaced keyframe slot needs before its first record)."""
        self.record(frame, None)

    def reset(self):
        self._check()
        self._bits.zero_()

    # --- queries
    def bits(self):
        """int32 [P, Wd]: the rows' words as stored (bit f of a row: bit f & 31 of word f >> 5)."""
        self._check()
        return self._bits[:self.model.P]

    @torch.no_grad()
    def pair_counts(self):
        """int64 [F, F]: [f, g] = the number of rows both f and g see (symmetric; the diagonal is each frame's visible count).  n_frames <= 128."""
        from . import _lib
        self._check()
        F = self.n_frames
        if F > COVIS_MAX_PAIR_FRAMES:
            raise ValueError(f"Covisibility.pair_counts: n_frames = {F} is above {COVIS_MAX_PAIR_FRAMES} (use frame_counts per frame)")
        out = torch.zeros(F, F, dtype=torch.int32, device=self._bits.device)
        if self.model.P:
            _lib.check(_lib.lib().gslic_covis_pair_counts(self.model.P, F, self._bits.data_ptr(), _lib.ptr(out), _lib.current_stream_ptr()))
        return out.long()

    @torch.no_grad()
    def frame_counts(self, frame):
        """int64 [F]: [g] = the number of rows that `frame` (an int or a device word) and g both see: the window query around one keyframe."""
        from . import _lib
        self._check()
        word = self._frame_word(frame)
        out = torch.zeros(self.n_frames, dtype=torch.int32, device=self._bits.device)
        if self.model.P:
            _lib.check(_lib.lib().gslic_covis_frame_counts(self.model.P, self.n_frames, self._bits.data_ptr(), _lib.ptr(word), _lib.ptr(out),
                                                           _lib.current_stream_ptr()))
        return out.long()

    def _mask_words(self, frames):
        """frames: None (every frame), a bool [F] tensor / array, or frame indices -> the int32 [Wd] device mask (or None)."""
        if frames is None:
            return None
        import numpy as np
        f = frames.detach().cpu().numpy() if torch.is_tensor(frames) else np.asarray(list(frames) if not isinstance(frames, np.ndarray) else frames)
        if f.dtype == np.bool_:
            if f.shape != (self.n_frames,):
                raise ValueError(f"Covisibility: a frame mask must have {self.n_frames} entries, got {f.shape}")
            idx = np.flatnonzero(f)
        else:
            idx = np.asarray([self._index(i) for i in f.reshape(-1)], dtype=np.int64)
        words = np.zeros(self.words, dtype=np.uint32)
        np.bitwise_or.at(words, idx >> 5, np.uint32(1) << (idx & 31).astype(np.uint32))
        return torch.from_numpy(words.view(np.int32)).to(self._bits.device)

    def _row_counts(self, frames, min_others, with_redundant):
        from . import _lib
        self._check()
        P, dev = self.model.P, self._bits.device
        n_seen = torch.zeros(P, dtype=torch.int32, device=dev)
        red = torch.zeros(self.n_frames, dtype=torch.int32, device=dev) if with_redundant else None
        if int(min_others) < 0:
            raise ValueError(f"Covisibility: min_others = {min_others} is negative")
        if P:
            mask = self._mask_words(frames)
            _lib.check(_lib.lib().gslic_covis_row_counts(P, self.n_frames, self._bits.data_ptr(), _lib.ptr(mask), _lib.ptr(n_seen), int(min_others),
                                                         _lib.ptr(red), _lib.current_stream_ptr()))
        return n_seen, red

    @torch.no_grad()
    def seen_count(self, frames=None):
        """int32 [P]: how many of `frames` (None: all; a bool [F] mask or frame indices) see each row."""
        return self._row_counts(frames, 0, False)[0]

    @torch.no_grad()
    def redundant(self, min_others, frames=None):
        """int64 [F]: [f] = the number of rows f sees that at least 1 + min_others of `frames` (None: all) see — with f among them, "f and at least
        min_others others".  redundant(n) / pair_counts()[f, f] near 1 is the usual criterion for giving keyframe f up."""
        return self._row_counts(frames, min_others, True)[1].long()

    def rows_of(self, frame):
        """bool [P]: the rows frame `frame` (a host int) saw when it was last recorded."""
        self._check()
        f = self._index(frame)
        return ((self._bits[:self.model.P, f >> 5] >> (f & 31)) & 1).bool()

    def seen_by_fewer_than(self, n, frames=None):
        """bool [P]: rows fewer than n of `frames` see — a mask for prune(protect= / drop=) (n = 2: rows only one keyframe ever saw, or none)."""
        return self.seen_count(frames) < int(n)

    def overlap(self, frame):
        """float32 [F]: frame_counts(frame) / the frame's own visible count — the share of what `frame` sees that g sees too; 0 where it sees nothing."""
        fc = self.frame_counts(frame).to(torch.float32)
        own = fc[self._index(frame)] if not torch.is_tensor(frame) else fc.gather(0, frame.long().clamp(0, self.n_frames - 1))
        return torch.where(own > 0, fc / own.clamp_min(1.0), torch.zeros_like(fc))

    def state_dict(self):
        self._check()
        return dict(n_frames=self.n_frames, bits=self._bits[:self.model.P].clone())

    def load_state_dict(self, state):
        self._check()
        P = self.model.P
        bits = torch.as_tensor(state["bits"])
        if int(state["n_frames"]) != self.n_frames or tuple(bits.shape) != (P, self.words) or bits.dtype != torch.int32:
            raise ValueError(f"Covisibility.load_state_dict: expected n_frames = {self.n_frames} and int32 bits [{P}, {self.words}], got "
                             f"n_frames = {state['n_frames']} and {bits.dtype} {tuple(bits.shape)}")
        self._bits[:P].copy_(bits)
        self._bits[P:].zero_()


def _covis_for_step(covis, model, keyframes):
    """The checks GraphedStep makes on its covis= argument (None passes): this model's object, its rows current, a store whose slots fit its columns."""
    if covis is None:
        return None
    if not isinstance(covis, Covisibility) or covis.model is not model:
        raise ValueError("covis must be a Covisibility of the model that is trained")
    if keyframes is None:
        raise ValueError("GraphedStep: covis given without keyframes (the recorded column is the store's slot; a host without a store calls "
                         "covis.record(frame, step.visible) itself)")
    if covis.n_frames < keyframes.capacity:
        raise ValueError(f"GraphedStep: covis has {covis.n_frames} frames, the keyframe store {keyframes.capacity} slots (column = slot)")
    covis._check()
    return covis


def exchange_mode():
    """How the N > 1 step exchanges gradients: "rank1" (default: 11 floats all-reduced + the 3-float colour gradient all-gathered,
    exchange_rank1), "dense" (the whole [P x 59] slab all-reduced in three pipelined segments), "sparse" (only the rows some view sees).
    GSLIC_EXCHANGE selects; GSLIC_SPARSE_EXCHANGE=1 is the older spelling of "sparse"."""
    m = os.environ.get("GSLIC_EXCHANGE", "").lower()
    if m in ("rank1", "dense", "sparse", "single"):   # "single": north_star's wording to the letter — ONE all-reduce per step (allreduce_slab_single)
        return m
    return "sparse" if os.environ.get("GSLIC_SPARSE_EXCHANGE") == "1" else "rank1"


DIST_TIMING = None   # bench.py sets this to a dict: the N > 1 step then records CUDA events at its three phase boundaries


def _dist_mark(name):
    if DIST_TIMING is not None:
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        DIST_TIMING.setdefault(name, []).append(ev)


def exchange_chunks():
    """GSLIC_EXCHANGE_CHUNKS = C > 1: the rank-1 exchange runs the per-Gaussian backward in C row chunks and puts chunk c on the wire (one
    all-gather + one all-reduce per chunk) while chunk c + 1 is computed; the Adam updates of a chunk follow its collectives.  Default 1."""
    try:
        return max(1, int(os.environ.get("GSLIC_EXCHANGE_CHUNKS", "1")))
    except ValueError:
        return 1


def _dist_on():
    """True when the per-step gradient exchange has to run.  GSLIC_FORCE_DIST=1 also takes the exchange path in a process group of
    ONE rank (the RCCL smoke test on a single-GPU box: same code path as N > 1, the all-reduce degenerates to a copy)."""
    if not (torch.distributed.is_available() and torch.distributed.is_initialized()):
        return False
    return torch.distributed.get_world_size() > 1 or os.environ.get("GSLIC_FORCE_DIST") == "1"


class GradSlab:
    """One contiguous fp32 buffer [P x (11+3K)] holding the six gradient tensors back to back (group order of
    gaussian.cpp:399-418).  The fused backward writes straight into its views, so the per-step exchange is ONE in-place
    all-reduce of `flat` with no concatenation copy (472 MB at 2M Gaussians, SH degree 3)."""

    def __init__(self, model):
        self.P = model.P
        shapes = [tuple(p.shape) for p in model.parameters()]
        sizes = [int(torch.tensor(s).prod()) for s in shapes]
        # (the slab is followed by P more floats: GSLIC_EXCHANGE=single ships the visibility mask in the SAME all-reduce, allreduce_slab_single)
        self.flat_and_mask = torch.empty(sum(sizes) + self.P, device=model.device)
        self.flat = self.flat_and_mask[:sum(sizes)]
        self.mask_f = self.flat_and_mask[sum(sizes):]
        # exchange_rank1's all-gather payload of THIS rank, one contiguous block: {colour gradient [P,3] fp32, camera centre [3] fp32,
        # visibility [P] bytes, padding to 4 bytes}; `rgb` (what the backward writes), `pay_campos` and `pay_vis` are views into it
        self.pay_bytes = (12 * self.P + 12 + self.P + 3) // 4 * 4
        self.payload = torch.zeros(self.pay_bytes, dtype=torch.uint8, device=model.device)
        self.rgb = self.payload[:12 * self.P].view(torch.float32).view(self.P, 3)
        self.pay_campos = self.payload[12 * self.P:12 * self.P + 12].view(torch.float32)
        self.pay_vis = self.payload[12 * self.P + 12:12 * self.P + 12 + self.P]
        self.payload_all = None
        self.rgb_all, self.campos_all = None, None
        self.views, off = {}, 0
        for name, shp, n in zip(model.NAMES, shapes, sizes):
            self.views[name] = self.flat[off:off + n].view(shp)
            off += n

    def grads(self, model):
        return [self.views[n] for n in model.NAMES]

    def run(self, model, g0, g1):
        """(flat slice covering the whole groups g0..g1-1, their indices): consecutive groups are contiguous in the slab."""
        sizes = [self.views[n].numel() for n in model.NAMES]
        offs = [0]
        for n in sizes:
            offs.append(offs[-1] + n)
        return self.flat[offs[g0]:offs[g1]], list(range(g0, g1))

    def segments(self, model):
        """The slab as three contiguous runs of whole groups, largest first: features_rest (76 % of the bytes), then
        xyz + features_dc, then opacity + scaling + rotation.  Returns [(flat slice, group indices)]."""
        sizes = [self.views[n].numel() for n in model.NAMES]
        offs = [0]
        for n in sizes:
            offs.append(offs[-1] + n)
        return [(self.flat[offs[2]:offs[3]], [2]), (self.flat[offs[0]:offs[2]], [0, 1]), (self.flat[offs[3]:offs[6]], [3, 4, 5])]


def allreduce_slab(slab, visible):
    """The per-step exchange on a GradSlab: SUM all-reduce of the slab in place + MAX (= OR) of the visibility bytes."""
    vis = visible.to(torch.uint8)
    torch.distributed.all_reduce(slab.flat, op=torch.distributed.ReduceOp.SUM)
    torch.distributed.all_reduce(vis, op=torch.distributed.ReduceOp.MAX)
    return vis.bool()


def allreduce_slab_single(slab, visible):
    """GSLIC_EXCHANGE=single — the exchange exactly as north_star words it: "a single RCCL all-reduce of Gaussian gradients over xGMI per optimiser
    step".  ONE SUM all-reduce of [P x 59] gradient floats + P floats carrying the visibility mask (0 / 1 per view: the sum is > 0 where some view
    sees the Gaussian — the OR), one collective on the wire instead of the default's three, at 4 (59 + 1) P bytes per rank and direction against
    rank-1's 44 P + (N - 1) 13 P (480 vs 114-336 MB at 2M Gaussians, N = 2-8).  Kept selectable so that the first run on real links measures both
    designs in one command (bench.py --gpus N reports `exchange.mode`)."""
    slab.mask_f.copy_(visible)
    torch.distributed.all_reduce(slab.flat_and_mask, op=torch.distributed.ReduceOp.SUM)
    return slab.mask_f > 0


def allreduce_slab_async(slab, visible, model):
    """The same exchange, pipelined against the optimiser: the visibility mask first (2 MB, blocking), then the three segments of
    the slab as asynchronous SUM all-reduces issued back to back.  Returns (reduced visibility, [(work, group indices)]): the
    caller waits for a segment and runs Adam on ITS groups while the following segments are still on the links, so all but the
    last, small Adam launch hide under the transfer (at 2M Gaussians the transfer is the longer leg of an N > 1 step)."""
    vis = visible.to(torch.uint8)
    torch.distributed.all_reduce(vis, op=torch.distributed.ReduceOp.MAX)
    works = [(torch.distributed.all_reduce(seg, op=torch.distributed.ReduceOp.SUM, async_op=True), idx) for seg, idx in slab.segments(model)]
    return vis.bool(), works


def allreduce_slab_sparse(slab, visible, model):
    """The exchange restricted to the rows some view actually sees: MAX (= OR) of the visibility bytes first, then ONE SUM all-reduce
    of a compacted slab holding only the rows of the OR-ed mask (every rank derives the same row list from the same mask), scattered
    back into the full slab.  Rows outside the mask are invisible on every rank: their gradients are exact zeros everywhere and Adam
    skips them.  Bytes on the links: 4 * 59 * |mask| instead of 4 * 59 * P — a SLAM view sees a fraction of the map, the synthetic
    8-view rig ~85 % (tools/exchange_bytes.py).  Result identical to allreduce_slab (bit for bit at N = 2; for N > 2 the rank order of
    the sum may differ per element).  Returns (reduced visibility, rows exchanged)."""
    vis = visible.to(torch.uint8)
    torch.distributed.all_reduce(vis, op=torch.distributed.ReduceOp.MAX)
    mask = vis.bool()
    idx = mask.nonzero(as_tuple=False).squeeze(1)          # (one host sync: the row count sizes the buffer; the MAX-reduce above already blocked)
    P, V = slab.P, int(idx.numel())
    if V == 0:
        return mask, 0
    rows = [slab.views[n].view(P, -1) for n in model.NAMES]
    widths = [r.shape[1] for r in rows]
    compact = torch.empty(V * sum(widths), device=slab.flat.device, dtype=slab.flat.dtype)
    parts, off = [], 0
    for r, w in zip(rows, widths):                          # group-major, like the slab itself
        part = compact[off:off + V * w].view(V, w)
        torch.index_select(r, 0, idx, out=part)
        parts.append(part)
        off += V * w
    torch.distributed.all_reduce(compact, op=torch.distributed.ReduceOp.SUM)
    for r, part in zip(rows, parts):
        r.index_copy_(0, idx, part)
    return mask, V


def exchange_rank1(slab, rgb_local, visible, model, campos):
    """The N > 1 exchange with the SH gradients shipped as what they are — rank-1.  computeColorFromSH's backward (backward.cu:27-136) is
    linear in the clamp-masked colour gradient dRGB: dL_ddc = SH_C0 dRGB, dL_dsh[k] = c_k(dir) dRGB with c_k a function of the view
    direction only.  So of the 59 gradient floats per Gaussian only 11 (xyz, opacity, scaling, rotation) are all-reduced; each rank
    all-gathers the views' 3-float dRGB and rebuilds the summed dL_ddc / dL_dsh itself (gslic_sh_grad_from_rgb: the backward's own
    products, summed in view order — at N = 2 bit-identical to the dense all-reduce).  Bytes on a rank's links per step:
    2 (N-1)/N 44 P + (N-1) 13 P instead of 2 (N-1)/N 236 P — 4.1x less at N = 2, 2.5x less at N = 8 (xGMI is point-to-point: the dense
    slab is per-link bound).

    THREE collectives per step, all asynchronous, none in front of the others: ONE all-gather of a per-rank payload {dRGB, camera centre,
    visibility bytes} (the rebuild kernel reads the gathered blocks in place through a view stride; the masks are OR-ed locally, so no
    separate MAX-reduce blocks the step), and the all-reduces of the two contiguous runs of the gradient slab that hold the 11 small
    floats (xyz | ... | opacity, scaling, rotation).  Returns (OR-ed visibility, works) like allreduce_slab_async: wait on a work, then run
    Adam on its groups; the rebuild of the SH rows runs behind the all-gather while the all-reduces are still on the links.

    ALIASING (folded path, the default): the returned mask is a bool VIEW of the persistent buffer slab.vis_or.  It is filled by the launch
    inside the returned work's wait() — not before — and overwritten by the next step: a caller that keeps `visible` across steps
    (densification statistics, logging) must clone it after wait()."""
    from . import rasterizer as rz
    dist = torch.distributed
    n = dist.get_world_size()
    assert rgb_local.data_ptr() == slab.rgb.data_ptr(), "the colour gradient must have been written into the slab's payload"
    if campos is not None:   # (None: the backward kernel has filled the payload's camera centre and mask itself: gslic_rasterize_backward_rgb_payload)
        slab.pay_campos.copy_(campos.reshape(3))
        slab.pay_vis.copy_(visible)
    if slab.payload_all is None or slab.payload_all.size(0) != n:
        slab.payload_all = torch.empty(n, slab.pay_bytes, dtype=torch.uint8, device=slab.flat.device)
    w_pay = dist.all_gather_into_tensor(slab.payload_all, slab.payload.view(1, slab.pay_bytes), async_op=True)
    works = [(dist.all_reduce(seg, op=dist.ReduceOp.SUM, async_op=True), idx) for seg, idx in (slab.run(model, 0, 1), slab.run(model, 3, 6))]
    P = slab.P
    rgb0 = slab.payload_all[0, :12 * P].view(torch.float32)            # view 0's block; view v sits pay_bytes / 4 floats further
    cam0 = slab.payload_all[0, 12 * P:12 * P + 12].view(torch.float32)
    stride = slab.pay_bytes // 4
    fused = getattr(model, "optimizer", None) is not None and os.environ.get("GSLIC_RANK1_SPLIT_ADAM") != "1"
    if fused and os.environ.get("GSLIC_RANK1_FOLD_ADAM", "1") != "0":
        # ONE launch behind the three collectives: OR of the gathered masks, SH rows rebuilt and consumed, Adam of all six groups
        # (gslic_sh_grad_from_rgb_adam_all) — no MAX-reduce, no mask copies, no separate Adam launches on the step's critical path
        if getattr(slab, "vis_or", None) is None:
            slab.vis_or = torch.zeros(P, dtype=torch.uint8, device=slab.flat.device)
        vis_all0 = slab.payload_all[0, 12 * P + 12:12 * P + 12 + P]

        class _All:
            def wait(self_inner):
                w_pay.wait()
                for w, _ in works:
                    w.wait()
                v = slab.views
                model.optimizer.step_all_from_exchange(model.xyz.detach(), cam0, rgb0, model.sh_degree, n, stride, vis_all0, slab.pay_bytes, slab.vis_or,
                                                       (v["xyz"], v["opacity"], v["scaling"], v["rotation"]))
        return slab.vis_or.view(torch.bool), [(_All(), [])]
    w_pay.wait()   # (orders the current stream behind the gather; the host does not block on RCCL)
    vis = slab.payload_all[:, 12 * P + 12:12 * P + 12 + P].max(0).values.bool()   # OR of the views' masks

    class _Rebuild:   # rebuilds dL_ddc / dL_dsh of all views from the gathered colour gradients (the mask has to be set first: see the caller)
        def wait(self_inner):
            if fused:   # ... and applies the masked Adam to features_dc / features_rest in the same kernel: the rows are never materialised
                model.optimizer.step_sh_from_rgb(model.xyz.detach(), cam0, rgb0, model.sh_degree, n_views=n, view_stride=stride)
            else:       # ... into the slab, for a following optimizer.step(only=[1, 2])
                rz.sh_grad_from_rgb(model.xyz.detach(), cam0, rgb0, model.sh_degree, slab.views["features_dc"], slab.views["features_rest"],
                                    n_views=n, view_stride=stride)
    return vis, [(_Rebuild(), [] if fused else [1, 2])] + works


class _RawRaster:
    """(model, camera, background) as the pieces the raw-parameter forward and backward take (rasterizer._forward / _backward: activations
    inside the kernels, no autograd), with or without the depth image.  pose: (view, proj, campos) device tensors in place of the camera's own
    (GraphedStep's static buffers).  forward() keeps what backward() needs in `state` = (R, B, radii, geom, binning, img, sample)."""

    def __init__(self, model, cam, bg, depth=False, e=None, pose=None):
        self.depth, self.bg = depth, bg
        self.xyz, self.dc, self.rest = model.xyz.detach(), model.features_dc.detach(), model.features_rest.detach()
        self.op, self.sc, self.rot = model.opacity.detach(), model.scaling.detach(), model.rotation.detach()
        self.pose = pose or (cam.d_world_view_transform, cam.d_full_proj_transform, cam.d_camera_center)
        self.hw = (int(cam.image_height), int(cam.image_width))
        self.scal = (float(cam.tanfovx), float(cam.tanfovy), float(cam.limx_neg), float(cam.limx_pos), float(cam.limy_neg), float(cam.limy_pos), 1.0)
        self.degree, self.lambda_erank, self.tie_rank = model.sh_degree, model.lambda_erank, getattr(model, "tie_rank", None)
        # colors_precomp / cov3D_precomp: the empty tensors of the reference's host on the colour path, nothing at all on the depth path
        self.e = e if (e is not None or depth) else torch.empty(0, device=model.device)
        self.state = None

    def forward(self, bufs=None):
        """bufs: a CapacityBuffers (capacity mode) or None.  Returns (image, depth image or None, radii)."""
        from . import rasterizer as rz
        (R, B, image, _final_T, depth, radii, geom, binning, img, sample) = rz._forward(
            bufs, self.depth, self.hw + self.scal, self.degree, False, False, False, True, self.tie_rank, self.bg, self.xyz, self.dc, self.rest, self.e,
            self.op, self.sc, self.rot, self.e, *self.pose)
        self.state = (R, B, radii, geom, binning, img, sample)
        return image, depth, radii

    def backward(self, dL_dimage, dL_ddepth=None, **modes):
        """modes: out= / adam= / xyz_grad= / camera_grads= / rgb_out= ... of rasterizer.rasterize_gaussians_backward[_depth]."""
        from . import rasterizer as rz
        R, B, radii, geom, binning, img, sample = self.state
        return rz._backward((dL_dimage.size(1), dL_dimage.size(2)) + self.scal, self.degree, False, True, self.bg, self.xyz, radii, self.e, self.sc,
                            self.rot, self.e, *self.pose, dL_dimage, dL_ddepth if self.depth else None, self.dc, self.rest, geom, R, binning, img, B,
                            sample, self.lambda_erank, **modes)


class KeyframeStore:
    """The keyframes' ground-truth images on the device as the 8-bit pixels the camera delivered, decoded into the float32 target of a pyramid
    level by one launch (gslic_keyframe_encode / gslic_keyframe_decode; the three rules — storage, decode, encode — are written out in
    include/gslic_hip.h).  The reference keeps every keyframe as a float32 CPU tensor and uploads it at every step (gaussian.cpp:49, :80, :678).
    color: uint8 [capacity, H, W, 3] interleaved RGB; mask (masks=True): uint8 [capacity, H, W], decoded into the float32 [H_l, W_l] weight image
    the weighted loss takes (255 = weight 1).  Slots are handed out in order; `n` of them are filled.  Every slot has a serial number that put()
    bumps: a GraphedStep that has to repeat a step checks it.  Nothing here synchronises; add_u8 is a plain copy.

    depths=True: every slot also holds its LiDAR range image as 16-bit codes — depth: uint16 [capacity, H, W], 0 = not measured, k = depth
    k * depth_step, depth_step a power of two in [2^-16, 1] (2^-9 m: 1.95 mm, 127.998 m) — and, depth_weights=True, a confidence weight —
    dweight: uint8 [capacity, H, W] (gslic_keyframe_encode_depth / gslic_keyframe_decode_depth; the rules are in include/gslic_hip.h).  A level's
    depth target is the nearest return of every 2^l x 2^l block, which is the code-rounded range image of camera.at_level(l): one stored image
    serves every level.  A slot written without depth holds "nothing measured"."""

    MAX_LEVEL = 4   # GSLIC_KEYFRAME_MAX_LEVEL

    def __init__(self, width, height, capacity, device, masks=False, depths=False, depth_step=2.0 ** -9, depth_weights=False):
        W, H, C = int(width), int(height), int(capacity)
        if W < 1 or H < 1 or C < 1:
            raise ValueError(f"KeyframeStore: width = {width}, height = {height}, capacity = {capacity} must all be at least 1")
        if depth_weights and not depths:
            raise ValueError("KeyframeStore: depth_weights=True needs depths=True (the weight is the depth's)")
        mant, exp = math.frexp(float(depth_step)) if 0.0 < float(depth_step) <= 1.0 else (0.0, 0)
        if depths and not (mant == 0.5 and -15 <= exp <= 1):
            raise ValueError(f"KeyframeStore: depth_step = {depth_step!r} must be a power of two in [2^-16, 1]")
        self.width, self.height, self.capacity = W, H, C
        self.device = torch.device(device)
        self.color = torch.zeros(C, H, W, 3, dtype=torch.uint8, device=self.device)
        self.mask = torch.zeros(C, H, W, dtype=torch.uint8, device=self.device) if masks else None
        self.depth = torch.zeros(C, H, W, dtype=torch.uint16, device=self.device) if depths else None
        self.dweight = torch.zeros(C, H, W, dtype=torch.uint8, device=self.device) if depth_weights else None
        self.depth_step = float(depth_step) if depths else None
        self._frames = torch.arange(C, dtype=torch.int32, device=self.device)   # the device word that names slot i is _frames[i]: no copy per decode
        self._serial = [0] * C
        self._n = 0

    @property
    def n(self):
        """Slots filled."""
        return self._n

    @property
    def nbytes(self):
        """Device bytes of the slabs (all `capacity` slots)."""
        return sum(t.numel() * t.element_size() for t in (self.color, self.mask, self.depth, self.dweight) if t is not None)

    @property
    def has_masks(self):
        return self.mask is not None

    @property
    def has_depths(self):
        return self.depth is not None

    @property
    def has_depth_weights(self):
        return self.dweight is not None

    def _index(self, slot):
        s = int(slot)
        if not 0 <= s < self._n:
            raise IndexError(f"KeyframeStore: slot {slot} is outside [0, {self._n})")
        return s

    def serial(self, slot):
        return self._serial[self._index(slot)]

    def level_size(self, level):
        """(W_l, H_l) of a level; raises for a level the image does not have."""
        l = int(level)
        if not 0 <= l <= self.MAX_LEVEL:
            raise ValueError(f"KeyframeStore: level = {level} is outside [0, {self.MAX_LEVEL}]")
        if (self.width >> l) < 1 or (self.height >> l) < 1:
            raise ValueError(f"KeyframeStore: a {self.width} x {self.height} image has no level {l}")
        return self.width >> l, self.height >> l

    def _check_mask(self, mask):
        if mask is not None and self.mask is None:
            raise ValueError("KeyframeStore: mask given to a store built without masks (pass masks=True to the constructor)")

    def _next(self):
        if self._n >= self.capacity:
            raise RuntimeError(f"KeyframeStore: all {self.capacity} slots are filled")
        return self._n

    def _write(self, slot, image, mask):
        """gslic_keyframe_encode of a float image [3,H,W] (and a float mask [H,W]; None on a store with masks: weight 1 everywhere) into `slot`."""
        from . import _lib
        H, W = self.height, self.width
        self._check_mask(mask)
        img = image.detach().to(self.device, torch.float32).contiguous()
        if tuple(img.shape) != (3, H, W):
            raise ValueError(f"KeyframeStore: image of shape {tuple(image.shape)} given to a store of [3, {H}, {W}]")
        m = None
        if mask is not None:
            m = mask.detach().to(self.device, torch.float32).contiguous()
            if tuple(m.shape) != (H, W):
                raise ValueError(f"KeyframeStore: mask of shape {tuple(mask.shape)} given to a store of [{H}, {W}]")
        elif self.mask is not None:
            self.mask[slot].fill_(255)
        _lib.check(_lib.lib().gslic_keyframe_encode(W, H, _lib.ptr(img), _lib.ptr(m), _lib.ptr(self.color), _lib.ptr(self.mask) if m is not None else None,
                                                    self.capacity, slot, _lib.current_stream_ptr()))

    def _write_u8(self, slot, hwc_uint8, mask, bgr):
        H, W = self.height, self.width
        self._check_mask(mask)
        if hwc_uint8.dtype != torch.uint8 or tuple(hwc_uint8.shape) != (H, W, 3):
            raise ValueError(f"KeyframeStore: add_u8 takes a uint8 [{H}, {W}, 3] tensor, not {hwc_uint8.dtype} {tuple(hwc_uint8.shape)}")
        if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != (H, W)):
            raise ValueError(f"KeyframeStore: the mask of add_u8 is a uint8 [{H}, {W}] tensor, not {mask.dtype} {tuple(mask.shape)}")
        self.color[slot].copy_(hwc_uint8.flip(-1) if bgr else hwc_uint8)
        if self.mask is not None:
            if mask is None:
                self.mask[slot].fill_(255)
            else:
                self.mask[slot].copy_(mask)

    def _check_depth(self, depth, depth_weight):
        if depth is not None and self.depth is None:
            raise ValueError("KeyframeStore: depth given to a store built without depths (pass depths=True to the constructor)")
        if depth_weight is not None and self.dweight is None:
            raise ValueError("KeyframeStore: depth_weight given to a store built without depth weights (pass depth_weights=True to the constructor)")
        if depth_weight is not None and depth is None:
            raise ValueError("KeyframeStore: depth_weight given without depth (the weight is the depth's)")

    def _write_depth(self, slot, depth, depth_weight):
        """gslic_keyframe_encode_depth of a float depth image [H,W] (and a float weight [H,W]; None on a store with depth weights: 255 everywhere)
        into `slot`; depth None on a store with depths: the slot is cleared to "nothing measured"."""
        from . import _lib
        H, W = self.height, self.width
        self._check_depth(depth, depth_weight)
        if self.depth is None:
            return
        if depth is None:
            self.depth[slot].view(torch.int16).zero_()
            if self.dweight is not None:
                self.dweight[slot].fill_(255)
            return
        d = depth.detach().to(self.device, torch.float32).contiguous()
        if tuple(d.shape) != (H, W):
            raise ValueError(f"KeyframeStore: depth of shape {tuple(depth.shape)} given to a store of [{H}, {W}]")
        w = None
        if depth_weight is not None:
            w = depth_weight.detach().to(self.device, torch.float32).contiguous()
            if tuple(w.shape) != (H, W):
                raise ValueError(f"KeyframeStore: depth_weight of shape {tuple(depth_weight.shape)} given to a store of [{H}, {W}]")
        _lib.check(_lib.lib().gslic_keyframe_encode_depth(W, H, _lib.ptr(d), _lib.ptr(w), _lib.ptr(self.depth), _lib.ptr(self.dweight), self.capacity,
                                                          slot, self.depth_step, _lib.current_stream_ptr()))

    def add(self, image, mask=None, depth=None, depth_weight=None):
        """Encodes a float32 [3,H,W] image (values clamped to [0, 1], NaN as 0) and, on a store with masks, a float32 [H,W] mask into the next
        slot; on a store with depths, a float32 [H,W] depth image (and depth weight) too; returns the slot."""
        slot = self._next()
        self._check_depth(depth, depth_weight)
        self._write(slot, image, mask)
        self._write_depth(slot, depth, depth_weight)
        self._n += 1
        return slot

    def add_u8(self, hwc_uint8, mask=None, bgr=False, depth=None, depth_weight=None):
        """Copies a uint8 [H,W,3] image (any device; bgr=True: the channels are flipped, in torch) and a uint8 [H,W] mask into the next slot;
        depth / depth_weight: float32 [H,W] images, encoded as add's; returns the slot."""
        slot = self._next()
        self._check_depth(depth, depth_weight)
        self._write_u8(slot, hwc_uint8, mask, bgr)
        self._write_depth(slot, depth, depth_weight)
        self._n += 1
        return slot

    def put(self, slot, image=None, mask=None, u8=None, bgr=False, depth=None, depth_weight=None):
        """Replaces a filled slot — by a float image (as add) or, u8=, a uint8 [H,W,3] one (as add_u8), with its depth (None: nothing measured) —
        and bumps the slot's serial number."""
        s = self._index(slot)
        if (image is None) == (u8 is None):
            raise ValueError("KeyframeStore.put: pass exactly one of image and u8")
        self._check_depth(depth, depth_weight)
        if u8 is None:
            self._write(s, image, mask)
        else:
            self._write_u8(s, u8, mask, bgr)
        self._write_depth(s, depth, depth_weight)
        self._serial[s] += 1
        return s

    def put_depth(self, slot, depth, depth_weight=None):
        """Replaces only the depth (and depth weight) of a filled slot — LiDAR that arrives after the image — and bumps the slot's serial number."""
        s = self._index(slot)
        if self.depth is None:
            raise ValueError("KeyframeStore: put_depth on a store built without depths (pass depths=True to the constructor)")
        if depth is None:
            raise ValueError("KeyframeStore.put_depth: depth is None")
        self._write_depth(s, depth, depth_weight)
        self._serial[s] += 1
        return s

    def _decode(self, word, level, out, weight_out, n_frames=None):
        """gslic_keyframe_decode of the slot the device word names: one launch, colour and (with masks) weight."""
        from . import _lib
        _lib.check(_lib.lib().gslic_keyframe_decode(self.width, self.height, int(level), _lib.ptr(self.color), _lib.ptr(self.mask), _lib.ptr(word),
                                                    self._n if n_frames is None else int(n_frames), _lib.ptr(out),
                                                    None if self.mask is None else _lib.ptr(weight_out), _lib.current_stream_ptr()))

    def target_buffers(self, level=0):
        """Uninitialised (image [3,H_l,W_l], weight [H_l,W_l] or None) of a level, as target(out=) takes them."""
        Wl, Hl = self.level_size(level)
        image = torch.empty(3, Hl, Wl, dtype=torch.float32, device=self.device)
        return image, (torch.empty(Hl, Wl, dtype=torch.float32, device=self.device) if self.mask is not None else None)

    def target(self, slot, level=0, out=None):
        """The float32 target of a slot at a level: image [3,H_l,W_l], or (image, weight [H_l,W_l]) on a store with masks — usable as they are as
        gt_image / weight of every training_step*.  out: the tensor (the pair, with masks) to write into instead of allocating."""
        s = self._index(slot)
        Wl, Hl = self.level_size(level)
        if out is None:
            image, weight = self.target_buffers(level)
        else:
            image, weight = out if self.mask is not None else (out, None)
            for t, shape, name in ((image, (3, Hl, Wl), "image"), (weight, (Hl, Wl), "weight")):
                if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.color.device):
                    raise ValueError(f"KeyframeStore.target: out's {name} must be a contiguous float32 {list(shape)} tensor on the store's device")
        self._decode(self._frames[s:s + 1], level, image, weight)
        return image if self.mask is None else (image, weight)

    def _decode_depth(self, word, level, depth_out, dweight_out, n_frames=None):
        """gslic_keyframe_decode_depth of the slot the device word names: one launch, depth and (with depth weights) its weight."""
        from . import _lib
        _lib.check(_lib.lib().gslic_keyframe_decode_depth(self.width, self.height, int(level), _lib.ptr(self.depth), _lib.ptr(self.dweight),
                                                          _lib.ptr(word), self._n if n_frames is None else int(n_frames), self.depth_step,
                                                          _lib.ptr(depth_out), None if self.dweight is None else _lib.ptr(dweight_out),
                                                          _lib.current_stream_ptr()))

    def depth_target_buffers(self, level=0):
        """Uninitialised (depth [H_l,W_l], weight [H_l,W_l] or None) of a level, as depth_target(out=) takes them."""
        if self.depth is None:
            raise ValueError("KeyframeStore: this store was built without depths (pass depths=True to the constructor)")
        Wl, Hl = self.level_size(level)
        depth = torch.empty(Hl, Wl, dtype=torch.float32, device=self.device)
        return depth, (torch.empty(Hl, Wl, dtype=torch.float32, device=self.device) if self.dweight is not None else None)

    def depth_target(self, slot, level=0, out=None):
        """The float32 depth target of a slot at a level: depth [H_l,W_l] (0 = not measured), or (depth, weight [H_l,W_l]) on a store with depth
        weights — usable as they are as gt_depth / depth_weight of every training_step*.  out: the tensor (the pair) to write into."""
        s = self._index(slot)
        Wl, Hl = self.level_size(level)
        if out is None:
            depth, weight = self.depth_target_buffers(level)
        else:
            if self.depth is None:
                raise ValueError("KeyframeStore: this store was built without depths (pass depths=True to the constructor)")
            depth, weight = out if self.dweight is not None else (out, None)
            for t, name in ((depth, "depth"), (weight, "weight")):
                if t is not None and (tuple(t.shape) != (Hl, Wl) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.color.device):
                    raise ValueError(f"KeyframeStore.depth_target: out's {name} must be a contiguous float32 {[Hl, Wl]} tensor on the store's device")
        self._decode_depth(self._frames[s:s + 1], level, depth, weight)
        return depth if self.dweight is None else (depth, weight)


class Exposure:
    """Trainable per-view exposure: one 3x4 affine colour transform per view (or per group of views — which views share a row is the host's
    policy), applied to the rendered image before the loss: out_c = E[c,:3] . rgb + E[c,3] (gslic_exposure_apply; the rule is written out in
    include/gslic_hip.h).  The reference's host owns such a tensor — [I | 0] with an Adam of its own at exposure_lr, stepped after every view
    (gaussian.cpp:287-291, :419-422, :708-711) — and never applies it; n_views=1 is that single tensor.
    params [V,3,4] starts at [I | 0]; m, v [V,3,4] and steps [V] int32 are torch.optim.Adam's state (WITH bias correction, unlike the map's sparse
    Adam); grad [3,4] holds the last dL/dE a step computed.  The fused steps update the row inside the exposure backward's second launch
    (gslic_exposure_backward with its Adam descriptor); nothing here allocates or synchronises per step."""

    def __init__(self, n_views, device, lr=0.01, betas=(0.9, 0.999), eps=1e-8):
        V = int(n_views)
        if V < 1:
            raise ValueError(f"Exposure: n_views = {n_views} must be at least 1")
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        if not (self.lr >= 0.0 and 0.0 <= self.betas[0] < 1.0 and 0.0 <= self.betas[1] < 1.0 and self.eps >= 0.0):
            raise ValueError(f"Exposure: lr = {lr}, betas = {betas}, eps = {eps} must be >= 0 and the betas below 1")
        self.device = torch.device(device)
        self.params = torch.zeros(V, 3, 4, dtype=torch.float32, device=self.device)
        self.m, self.v = torch.zeros_like(self.params), torch.zeros_like(self.params)
        self.steps = torch.zeros(V, dtype=torch.int32, device=self.device)
        self.grad = torch.zeros(3, 4, dtype=torch.float32, device=self.device)
        self._views = torch.arange(V, dtype=torch.int32, device=self.device)   # the device word that names view i is _views[i]: no copy per step
        self.reset()

    @property
    def n_views(self):
        return self.params.size(0)

    def _index(self, view):
        v = int(view)
        if not 0 <= v < self.n_views:
            raise IndexError(f"Exposure: view {view} is outside [0, {self.n_views})")
        return v

    def matrix(self, view=0):
        """The [3,4] transform of a view: a view into `params` (no copy)."""
        return self.params[self._index(view)]

    def reset(self, view=None):
        """Back to [I | 0] with zero moments and step count: one view, or all of them."""
        rows = slice(None) if view is None else slice(self._index(view), self._index(view) + 1)
        self.params[rows] = torch.eye(3, 4, dtype=torch.float32, device=self.device)
        self.m[rows] = 0
        self.v[rows] = 0
        self.steps[rows] = 0
        if view is None:
            self.grad.zero_()

    def state_dict(self):
        return dict(params=self.params.clone(), m=self.m.clone(), v=self.v.clone(), steps=self.steps.clone(), lr=self.lr, betas=self.betas, eps=self.eps)

    def load_state_dict(self, state):
        if tuple(state["params"].shape) != tuple(self.params.shape):
            raise ValueError(f"Exposure: the state holds {tuple(state['params'].shape)}, this object {tuple(self.params.shape)}")
        self.params.copy_(state["params"]); self.m.copy_(state["m"]); self.v.copy_(state["v"]); self.steps.copy_(state["steps"])
        self.lr, self.betas, self.eps = float(state["lr"]), (float(state["betas"][0]), float(state["betas"][1])), float(state["eps"])

    def clone(self):
        other = Exposure(self.n_views, self.device, self.lr, self.betas, self.eps)
        other.load_state_dict(self.state_dict())
        other.grad.copy_(self.grad)
        return other

    def _descriptor(self, view_word, skip=None):
        """gslic_exposure_adam on this object's arrays; view_word: a device int32 [1] that names the row, skip: the optional device word."""
        from . import _lib
        p = lambda t: t.data_ptr()
        return _lib.ExposureAdam(p(self.params), p(self.m), p(self.v), p(self.steps), p(view_word), self.lr, self.betas[0], self.betas[1], self.eps,
                                 None if skip is None else p(skip))

    def adam_step(self, view, grad):
        """torch.optim.Adam's step on one row from a gradient the caller has (the autograd training_step, as the reference's torch::optim::Adam
        of exposure_ does it: LibTorch ops, bias terms in double).  The fused steps do not come here: their update is inside the backward kernel."""
        i = self._index(view)
        t = int(self.steps[i].item()) + 1
        b1, b2 = self.betas
        g = grad.detach().to(self.params.dtype).reshape(3, 4)
        self.m[i].mul_(b1).add_(g, alpha=1.0 - b1)
        self.v[i].mul_(b2).addcmul_(g, g, value=1.0 - b2)
        denom = (self.v[i].sqrt() / math.sqrt(1.0 - b2 ** t)).add_(self.eps)
        self.params[i].addcdiv_(self.m[i], denom, value=-self.lr / (1.0 - b1 ** t))
        self.steps[i] = t


def _check_exposure(who, exposure, view):
    """The checks every step makes on its exposure= argument (None passes): an Exposure on the image's device, one GPU, a view it has."""
    if exposure is None:
        return None
    if not isinstance(exposure, Exposure):
        raise ValueError(f"{who}: exposure must be a trainer.Exposure")
    if _dist_on():
        raise NotImplementedError(f"{who}: exposure is single-GPU only: the N > 1 gradient exchange carries no exposure gradient (every rank would "
                                  "update its own copy of E from its own view)")
    exposure._index(view)
    return exposure


class PoseSet:
    """Trainable keyframe poses on the device, the pose counterpart of Exposure: one row per view with the three arrays the rasteriser reads —
    view [V,16], proj [V,16], campos [V,3], in the layout and meaning of Camera.world_view_transform, full_proj_transform and camera_center —
    torch.optim.Adam's state on the six coordinates (rho, phi) of a LEFT se(3) increment (m, v [V,6], steps [V] int32, WITH bias correction, a
    rate for the translation and one for the rotation) and, once per set, the pose-independent projection [16].  gslic_pose_step — one launch —
    chains the three camera gradients of the backward to dL/d(rho, phi), steps the row by Adam and moves the pose by the exact retraction
    T_cw <- exp(delta^) T_cw, with R re-orthonormalised (the rule is written out in include/gslic_hip.h, restated in float64 by tests/pose_ref.py);
    grad [6] holds the last gradient.  Nothing here allocates or synchronises per step; camera() is the one call that reads back.

    `camera` supplies what the views share: the projection_matrix and the scalars a step bakes in (tanfov, the four limits).  All of them
    depend only on fx / W, cx / W, fy / H, cy / H (and the depth range), not on the image size, so one set serves every pyramid level l of a
    KeyframeStore whose width and height are divisible by 2^l (Camera.at_level halves W, H and the four intrinsics exactly; an odd size drops a
    column and changes cx / W): a step takes the image size from ITS camera and the pose from the set, and matches(camera.at_level(l)) says
    whether the set serves that camera.  Nothing the kernels read from the set depends on the image size.

    shared=True adds the calibration the views SHARE — a correction of the camera-body extrinsic and of the camera clock offset, the two errors
    that move every keyframe the same way: twist [V,6] (the camera-frame twist (v, w) of each view in m/s and rad/s, T_cw(t + dt) ~
    exp((dt xi)^) T_cw(t); zeros until set_twist / load(twist=) give it), Adam's state sm, sv [7] and ssteps [1] on (rho_x, phi_x, tau) with the
    rates lr_trans, lr_rot and lr_time, the accumulated extrinsic correction X [12] (rows of [R_x | t_x], the identity at the start), the
    accumulated time offset tau [1] in seconds and shared_grad [7], the last shared gradient.  gslic_pose_step_shared — one launch — chains the
    rendered view's camera gradient to g, takes g_tau = xi_i . g, steps the seven coordinates and moves EVERY row by d_x + d_tau xi_j (the rule is
    in include/gslic_hip.h, restated by tests/pose_shared_ref.py); steps reach it through shared=True / train_pose="shared".  extrinsic() and
    time_offset() read X and tau back (they synchronise, like camera()).  load(view, camera, calibrated=True) brings a keyframe that arrives later
    to the calibration the older rows were moved to (gslic_pose_calibrate_rows).  shared=False is the set as it is without, bit for bit."""

    _BAKED = ("tanfovx", "tanfovy", "limx_neg", "limx_pos", "limy_neg", "limy_pos")   # (level-invariant, like the projection)

    _SHARED = ("twist", "sm", "sv", "ssteps", "X", "tau")   # the arrays shared=True adds to the state (shared_grad beside them, like grad)

    def __init__(self, n_views, camera, device, lr_rot=1e-3, lr_trans=1e-3, betas=(0.9, 0.999), eps=1e-8, shared=False, lr_time=0.0):
        V = int(n_views)
        if V < 1:
            raise ValueError(f"PoseSet: n_views = {n_views} must be at least 1")
        self.lr_rot, self.lr_trans = float(lr_rot), float(lr_trans)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        if not (self.lr_rot >= 0.0 and self.lr_trans >= 0.0 and 0.0 <= self.betas[0] < 1.0 and 0.0 <= self.betas[1] < 1.0 and self.eps >= 0.0):
            raise ValueError(f"PoseSet: lr_rot = {lr_rot}, lr_trans = {lr_trans}, betas = {betas}, eps = {eps} must be >= 0 and the betas below 1")
        self.shared, self.lr_time = bool(shared), float(lr_time)
        if not self.lr_time >= 0.0:
            raise ValueError(f"PoseSet: lr_time = {lr_time} must be >= 0")
        if self.lr_time and not self.shared:
            raise ValueError("PoseSet: lr_time given to a set built without shared=True")
        self.device = dev = torch.device(device)
        self._intrinsics = camera   # (fx, fy, cx, cy, znear, zfar and the image size of the cameras camera() returns)
        self._projection_host = np.array(camera.projection_matrix, np.float32).reshape(16)
        self._baked = tuple(float(getattr(camera, k)) for k in self._BAKED)
        self.projection = torch.from_numpy(self._projection_host.copy()).to(dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self.view, self.proj, self.campos = torch.zeros(V, 16, **f32), torch.zeros(V, 16, **f32), torch.zeros(V, 3, **f32)
        self.m, self.v = torch.zeros(V, 6, **f32), torch.zeros(V, 6, **f32)
        self.steps = torch.zeros(V, dtype=torch.int32, device=dev)
        self.grad = torch.zeros(6, **f32)
        self._views = torch.arange(V, dtype=torch.int32, device=dev)    # the device word that names view i is _views[i]: no copy per step
        self._no_step = torch.ones(1, dtype=torch.int32, device=dev)    # a skip word that is set: the chain alone (do_step=False)
        if self.shared:
            self.twist = torch.zeros(V, 6, **f32)
            self.sm, self.sv, self.ssteps = torch.zeros(7, **f32), torch.zeros(7, **f32), torch.zeros(1, dtype=torch.int32, device=dev)
            self.X = torch.eye(3, 4, **f32).reshape(12).contiguous()
            self.tau = torch.zeros(1, **f32)
            self.shared_grad = torch.zeros(7, **f32)
        for i in range(V):   # every row starts as the camera's own pose
            self.load(i, camera)

    @property
    def n_views(self):
        return self.view.size(0)

    def _index(self, view):
        v = int(view)
        if not 0 <= v < self.n_views:
            raise IndexError(f"PoseSet: view {view} is outside [0, {self.n_views})")
        return v

    def matches(self, camera):
        """Whether the set serves `camera`: the set's projection_matrix and baked scalars (tanfov, the four limits) bit for bit.  The image size
        is not compared: a camera of another pyramid level of the same intrinsics matches."""
        same = np.array_equal(np.asarray(camera.projection_matrix, np.float32).reshape(16).view(np.int32), self._projection_host.view(np.int32))
        return same and tuple(float(getattr(camera, k)) for k in self._BAKED) == self._baked

    def _check_camera(self, who, camera):
        if not self.matches(camera):
            raise ValueError(f"{who}: the camera's projection_matrix or baked scalars (tanfov, limits) differ from the pose set's")

    def load(self, view, camera, twist=None, calibrated=False):
        """Row `view` becomes a bit copy of the camera's three arrays, with zero moments and step count.  On a shared set: twist [6] sets the row's
        camera-frame twist as set_twist does (None leaves it), and calibrated=True then applies the set's calibration to the row — T <-
        exp((tau xi)^) (X T), gslic_pose_calibrate_rows, one launch — so that a keyframe that arrives after the calibration has moved starts where
        the older rows were moved to.  calibrated=False is the bit copy."""
        i = self._index(view)
        self._check_camera("PoseSet.load", camera)
        if (twist is not None or calibrated) and not self.shared:
            raise ValueError("PoseSet.load: twist / calibrated given to a set built without shared=True")
        put = lambda dst, a, n: dst.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(n)))
        put(self.view[i], camera.world_view_transform, 16); put(self.proj[i], camera.full_proj_transform, 16); put(self.campos[i], camera.camera_center, 3)
        self.reset_moments(i)
        if twist is not None:
            self.set_twist(i, twist)
        if calibrated:
            self.calibrate_rows(i, 1)

    def _need_shared(self, who):
        if not self.shared:
            raise ValueError(f"{who}: the pose set was built without shared=True")

    def set_twist(self, view, xi):
        """The camera-frame twist (v [m/s], w [rad/s]) of row `view`: six values."""
        self._need_shared("PoseSet.set_twist")
        i = self._index(view)
        xi = np.ascontiguousarray(xi.detach().cpu().numpy() if torch.is_tensor(xi) else xi, np.float32).reshape(-1)
        if xi.size != 6:
            raise ValueError(f"PoseSet.set_twist: a twist is six values (v, w), got {xi.size}")
        self.twist[i].copy_(torch.from_numpy(xi))

    def calibrate_rows(self, first, count):
        """gslic_pose_calibrate_rows on rows [first, first + count): T <- exp((tau xi_j)^) (X T), one launch."""
        import ctypes
        from . import _lib
        self._need_shared("PoseSet.calibrate_rows")
        first, count = int(first), int(count)
        if first < 0 or count < 0 or first + count > self.n_views:
            raise IndexError(f"PoseSet.calibrate_rows: rows [{first}, {first + count}) are outside [0, {self.n_views})")
        d = self._shared_descriptor(self._views[0:1])
        _lib.check(_lib.lib().gslic_pose_calibrate_rows(ctypes.byref(d), first, count, _lib.current_stream_ptr()))

    def extrinsic(self):
        """The accumulated extrinsic correction as a host float64 4x4 [R_x | t_x; 0 0 0 1] (this call synchronises)."""
        self._need_shared("PoseSet.extrinsic")
        X = np.eye(4)
        X[:3, :] = self.X.cpu().numpy().astype(np.float64).reshape(3, 4)
        return X

    def time_offset(self):
        """The accumulated time offset in seconds (this call synchronises)."""
        self._need_shared("PoseSet.time_offset")
        return float(self.tau.cpu()[0])

    def pose(self, view):
        """(view [16], proj [16], campos [3]) of a row: device views into the set (no copy), usable as _RawRaster(..., pose=...)."""
        i = self._index(view)
        return self.view[i], self.proj[i], self.campos[i]

    def camera(self, view, level=0):
        """A new host Camera at the row's pose (this call synchronises: it is for saving trajectories): the intrinsics of the set's camera — at
        pyramid level `level` of it (Camera.at_level) — set_pose from the row's R, t, and then the row's own bits as its three arrays, host and
        device, so that it renders exactly what the row renders."""
        from .camera import Camera
        i, c = self._index(view), self._intrinsics.at_level(level)
        V = self.view[i].cpu().numpy().astype(np.float64).reshape(4, 4).T
        R, t = V[:3, :3], V[:3, 3]
        cam = Camera(c.image_width, c.image_height, c.fx, c.fy, c.cx, c.cy, R.T, -R.T @ t, c.znear, c.zfar)
        cam.world_view_transform = self.view[i].cpu().numpy().reshape(4, 4).copy()
        cam.full_proj_transform = self.proj[i].cpu().numpy().reshape(4, 4).copy()
        cam.camera_center = self.campos[i].cpu().numpy().copy()
        return cam.to_device(self.view.device)

    def reset_moments(self, view=None, shared=False):
        """Zero moments and step count: one view, or all of them (then the last gradient too).  shared=True: the shared state's instead — sm, sv,
        ssteps and shared_grad; X and tau, the calibration itself, stay."""
        if shared:
            self._need_shared("PoseSet.reset_moments")
            for a in (self.sm, self.sv, self.ssteps, self.shared_grad):
                a.zero_()
            return
        rows = slice(None) if view is None else slice(self._index(view), self._index(view) + 1)
        self.m[rows] = 0
        self.v[rows] = 0
        self.steps[rows] = 0
        if view is None:
            self.grad.zero_()

    def state_dict(self):
        state = dict(view=self.view.clone(), proj=self.proj.clone(), campos=self.campos.clone(), projection=self.projection.clone(), m=self.m.clone(),
                     v=self.v.clone(), steps=self.steps.clone(), lr_rot=self.lr_rot, lr_trans=self.lr_trans, betas=self.betas, eps=self.eps)
        if self.shared:
            state.update({k: getattr(self, k).clone() for k in self._SHARED}, lr_time=self.lr_time)
        return state

    def load_state_dict(self, state):
        if tuple(state["view"].shape) != tuple(self.view.shape):
            raise ValueError(f"PoseSet: the state holds {tuple(state['view'].shape)}, this object {tuple(self.view.shape)}")
        if not torch.equal(state["projection"].to(self.device).view(torch.int32), self.projection.view(torch.int32)):
            raise ValueError("PoseSet: the state was saved under another projection_matrix")
        if self.shared != ("X" in state):
            raise ValueError("PoseSet: the state was saved by a set " + ("without" if self.shared else "with") + " shared=True, this object was built "
                             + ("with" if self.shared else "without") + " it")
        for k in ("view", "proj", "campos", "m", "v", "steps") + (self._SHARED if self.shared else ()):
            getattr(self, k).copy_(state[k])
        self.lr_rot, self.lr_trans, self.eps = float(state["lr_rot"]), float(state["lr_trans"]), float(state["eps"])
        self.betas = (float(state["betas"][0]), float(state["betas"][1]))
        if self.shared:
            self.lr_time = float(state["lr_time"])

    def clone(self):
        other = PoseSet(self.n_views, self._intrinsics, self.device, self.lr_rot, self.lr_trans, self.betas, self.eps, self.shared, self.lr_time)
        other.load_state_dict(self.state_dict())
        other.grad.copy_(self.grad)
        if self.shared:
            other.shared_grad.copy_(self.shared_grad)
        return other

    def _descriptor(self, view_word, skip=None):
        """gslic_pose_adam on this object's arrays; view_word: a device int32 [1] that names the row, skip: the optional device word."""
        from . import _lib
        p = lambda t: t.data_ptr()
        return _lib.PoseAdam(p(self.view), p(self.proj), p(self.campos), p(self.m), p(self.v), p(self.steps), p(self.projection), p(view_word),
                             self.n_views, self.lr_trans, self.lr_rot, self.betas[0], self.betas[1], self.eps, None if skip is None else p(skip))

    def _step(self, view, cam_grads, do_step=True):
        """gslic_pose_step on row `view`: grad <- the chain of the three camera gradients; do_step: the row moves (else the skip word is set)."""
        i = self._index(view)
        return self._step_word(self._views[i:i + 1], cam_grads, None if do_step else self._no_step)

    def _step_word(self, view_word, cam_grads, skip):
        """gslic_pose_step on the row a device int32 names, with an optional device skip word (GraphedStep: the forward's overflow word)."""
        import ctypes
        from . import _lib
        gv, gp, gc = cam_grads
        for t, n, name in ((gv, 16, "dL_dviewmatrix"), (gp, 16, "dL_dprojmatrix"), (gc, 3, "dL_dcampos")):
            if t.numel() != n or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.view.device:
                raise ValueError(f"PoseSet: {name} must be {n} contiguous float32 values on the set's device")
        d = self._descriptor(view_word, skip)
        _lib.check(_lib.lib().gslic_pose_step(ctypes.byref(d), _lib.ptr(gv), _lib.ptr(gp), _lib.ptr(gc), _lib.ptr(self.grad), _lib.current_stream_ptr()))
        return self.grad

    def _shared_descriptor(self, view_word, skip=None):
        """gslic_pose_shared on this object's arrays; view_word / skip as _descriptor's."""
        from . import _lib
        p = lambda t: t.data_ptr()
        return _lib.PoseShared(p(self.view), p(self.proj), p(self.campos), p(self.projection), p(view_word), self.n_views, p(self.twist), p(self.sm),
                               p(self.sv), p(self.ssteps), p(self.X), p(self.tau), self.lr_trans, self.lr_rot, self.lr_time, self.betas[0],
                               self.betas[1], self.eps, None if skip is None else p(skip))

    def _step_shared(self, view, cam_grads, do_step=True):
        """gslic_pose_step_shared with row `view`'s gradient: shared_grad <- (g, xi . g); do_step: the seven coordinates step and every row moves."""
        i = self._index(view)
        return self._step_shared_word(self._views[i:i + 1], cam_grads, None if do_step else self._no_step)

    def _step_shared_word(self, view_word, cam_grads, skip):
        """gslic_pose_step_shared on the row a device int32 names, with an optional device skip word (GraphedStep: the forward's overflow word)."""
        import ctypes
        from . import _lib
        self._need_shared("PoseSet")
        gv, gp, gc = cam_grads
        for t, n, name in ((gv, 16, "dL_dviewmatrix"), (gp, 16, "dL_dprojmatrix"), (gc, 3, "dL_dcampos")):
            if t.numel() != n or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.view.device:
                raise ValueError(f"PoseSet: {name} must be {n} contiguous float32 values on the set's device")
        d = self._shared_descriptor(view_word, skip)
        _lib.check(_lib.lib().gslic_pose_step_shared(ctypes.byref(d), _lib.ptr(gv), _lib.ptr(gp), _lib.ptr(gc), _lib.ptr(self.shared_grad),
                                                     _lib.current_stream_ptr()))
        return self.shared_grad

    def shared_adam_step(self, view, cam_grads):
        """The shared kernel on gradients the caller already holds (cam_grads as adam_step's), taken as row `view`'s.  Returns shared_grad."""
        return self._step_shared(view, cam_grads, True)

    def adam_step(self, view, cam_grads):
        """The kernel on gradients the caller already holds: cam_grads = (dL_dviewmatrix [16], dL_dprojmatrix [16], dL_dcampos [3]) device tensors,
        as a backward with camera_grads=True returns them.  Returns grad."""
        return self._step(view, cam_grads, True)

    def _load_row(self, view_word, view_out, proj_out, campos_out):
        """gslic_pose_load: the row the device word names into three buffers (GraphedStep's static pose), one launch."""
        from . import _lib
        p = _lib.ptr
        _lib.check(_lib.lib().gslic_pose_load(p(self.view), p(self.proj), p(self.campos), p(view_word), self.n_views, p(view_out), p(proj_out),
                                              p(campos_out), _lib.current_stream_ptr()))


def _check_poses(who, poses, view, camera=None, shared=False):
    """The checks every step makes on its poses= argument (None passes): a PoseSet, one GPU, a view it has, a camera of the set's intrinsics; shared:
    the step trains the shared calibration, which needs a set built with shared=True."""
    if poses is None:
        if shared:
            raise ValueError(f"{who}: shared=True needs poses= (a trainer.PoseSet built with shared=True holds the calibration)")
        return None
    if not isinstance(poses, PoseSet):
        raise ValueError(f"{who}: poses must be a trainer.PoseSet")
    if _dist_on():
        raise NotImplementedError(f"{who}: poses is single-GPU only: the N > 1 gradient exchange carries no camera gradient (every rank would "
                                  "step its own copy of the pose from its own view)")
    poses._index(view)
    if camera is not None:
        poses._check_camera(who, camera)
    if shared and not poses.shared:
        raise ValueError(f"{who}: shared=True on a pose set built without shared=True")
    return poses


def _exposure_losses(fl, image, gt_image, depth, gt_depth, lambda_depth, weight, depth_weight, depth_huber, exposure, view, exposure_step):
    """_fused_losses under an exposure model: E applied into a scratch image of the FusedLoss, the loss calls — unchanged — on that image, then
    the exposure backward on their dL/dimage, which hands the rasteriser E^T g, leaves dL/dE in exposure.grad and (exposure_step) updates the
    view's row by Adam in its second launch.  The depth image is not touched.  view: the row's index, or GraphedStep's (E [12], the device word
    that names the row, the device word that turns the update off)."""
    if isinstance(view, tuple):
        E, word, skip = view
    else:
        i = exposure._index(view)
        E, word, skip = exposure.params[i], exposure._views[i:i + 1], None
    out = fl.exposure_apply(image, E)
    dL_dout, dL_ddepth, terms = _fused_losses(fl, out, gt_image, depth, gt_depth, lambda_depth, weight, depth_weight, depth_huber)
    dL_dimage = fl.exposure_backward(image, E, dL_dout, exposure.grad, exposure._descriptor(word, skip) if exposure_step else None)
    return dL_dimage, dL_ddepth, terms


def _fused_losses(fl, image, gt_image, depth, gt_depth, lambda_depth, weight=None, depth_weight=None, depth_huber=0.0, exposure=None, view=0,
                  exposure_step=True):
    """The colour loss kernels (weight [H,W]: the weighted ones) and, for a depth image, the depth loss kernels (depth_weight [H,W] / depth_huber:
    the weighted ones): (dL/dimage, dL/ddepth or None, terms).  exposure (a trainer.Exposure) / view: the same calls on the exposure-compensated
    image, between gslic_exposure_apply and gslic_exposure_backward (_exposure_losses); None is exactly the calls below."""
    if exposure is not None:
        return _exposure_losses(fl, image, gt_image, depth, gt_depth, lambda_depth, weight, depth_weight, depth_huber, exposure, view, exposure_step)
    if depth is None:
        dL_dimage, terms = fl.forward_backward(image, gt_image, weight)
        return dL_dimage, None, terms
    dL_dimage, _ = fl.forward_backward(image, gt_image, weight)
    dL_ddepth, _ = fl.depth_forward_backward(depth, gt_depth, lambda_depth, depth_weight, depth_huber)
    return dL_dimage, dL_ddepth, fl.terms3


def _use_depth(who, gt_depth, lambda_depth, depth_weight, depth_huber):
    """Whether a step runs depth supervision, and the checks every step shares: a depth weight or Huber threshold needs a depth target, and the
    threshold is finite and >= 0.  (gt_depth with lambda_depth == 0 is the colour-only step; the two arguments are then not used.)"""
    if not (0.0 <= float(depth_huber) < float("inf")):   # (a NaN fails)
        raise ValueError(f"{who}: depth_huber = {depth_huber!r} must be finite and >= 0")
    if gt_depth is None and (depth_weight is not None or float(depth_huber) != 0.0):
        raise ValueError(f"{who}: depth_weight / depth_huber given without gt_depth (they shape the depth term of the loss: pass gt_depth and lambda_depth)")
    return gt_depth is not None and lambda_depth != 0.0


def _depth_xyz_grad(model):
    """The [P,3] buffer, kept on the model, in which the fused depth backwards assemble the xyz gradient before its update."""
    xg = getattr(model, "_depth_xyz_grad", None)
    if xg is None or xg.shape[0] != model.P or xg.device != model.xyz.device:
        xg = model._depth_xyz_grad = torch.empty(model.P, 3, dtype=torch.float32, device=model.device)
    return xg


def _grad_slab(model):
    slab = getattr(model, "_grad_slab", None)
    if slab is None or slab.P != model.P:
        slab = model._grad_slab = GradSlab(model)
    return slab


class _ChunkedExchange:
    """Buffers of the chunked rank-1 exchange for one (P, world, chunks): per chunk c = rows [p0, p1) a block of the 11 small gradient floats
    {xyz [n,3] | opacity [n] | scaling [n,3] | rotation [n,4]} (ONE all-reduce) and an all-gather payload {dRGB [n,3], camera centre [3],
    visibility [n] bytes}.  The backward kernels index their outputs by the absolute Gaussian index: they get the blocks' addresses moved back
    by p0 rows."""

    def __init__(self, P, world, chunks, device):
        self.P, self.world, self.chunks = P, world, chunks
        step = -(-P // chunks)
        step = -(-step // 256) * 256
        self.bounds = [(p0, min(p0 + step, P)) for p0 in range(0, P, step)]
        self.small = torch.empty(11 * P, device=device)
        self.vis = torch.zeros(P, dtype=torch.uint8, device=device)
        self.pay, self.pay_all, self.small_off = [], [], []
        off = 0
        for p0, p1 in self.bounds:
            n = p1 - p0
            nbytes = (12 * n + 12 + n + 3) // 4 * 4
            self.pay.append(torch.zeros(nbytes, dtype=torch.uint8, device=device))
            self.pay_all.append(torch.empty(world, nbytes, dtype=torch.uint8, device=device))
            self.small_off.append(off)
            off += 11 * n


def training_step_rank1_chunked(model, cam, bg, dL_dimage, fwd, chunks):
    """The N > 1 step behind the forward and the loss, with the exchange overlapped chunk by chunk (exchange_chunks()).  Per chunk: the
    per-Gaussian backward of its rows (the blend backward runs once, with the first chunk), then — asynchronously, on RCCL's streams — ONE
    all-gather of the chunk's {dRGB, camera centre, mask} and ONE all-reduce of its 11 small gradient floats, while the next chunk is being
    computed.  Then, chunk by chunk as the collectives land: OR of the masks, SH rows rebuilt and consumed by the masked Adam of
    features_dc / features_rest, Adam of the four small groups.  Same arithmetic per Gaussian as the unchunked step."""
    dist = torch.distributed
    radii = fwd[2]
    dev = model.device
    rr = _RawRaster(model, cam, bg)
    rr.state = fwd
    xyz = rr.xyz
    n_world = dist.get_world_size()
    cx = getattr(model, "_chunk_xchg", None)
    if cx is None or cx.P != model.P or cx.world != n_world or cx.chunks != chunks:
        cx = model._chunk_xchg = _ChunkedExchange(model.P, n_world, chunks, dev)
    slab = model._grad_slab
    visible_local = (radii > 0).to(torch.uint8)
    works = []
    for c, (p0, p1) in enumerate(cx.bounds):
        n = p1 - p0
        sm = cx.small.data_ptr() + 4 * cx.small_off[c]
        pay = cx.pay[c]
        addr = {"xyz": sm - 12 * p0, "opacity": sm + 12 * n - 4 * p0, "scaling": sm + 16 * n - 12 * p0, "rotation": sm + 28 * n - 16 * p0,
                "rgb": pay.data_ptr() - 12 * p0}
        rr.backward(dL_dimage, out=slab.views, rgb_out=slab.rgb, rows=(p0, p1), skip_blend=(c > 0), out_addr=addr)
        pay[12 * n:12 * n + 12].view(torch.float32).copy_(cam.d_camera_center.reshape(3))
        pay[12 * n + 12:12 * n + 12 + n].copy_(visible_local[p0:p1])
        if c == 0:
            _dist_mark("bwd_done")   # (first chunk on the wire: everything behind it overlaps with the remaining chunks' compute)
        w_pay = dist.all_gather_into_tensor(cx.pay_all[c], pay.view(1, -1), async_op=True)
        w_red = dist.all_reduce(cx.small[cx.small_off[c]:cx.small_off[c] + 11 * n], op=dist.ReduceOp.SUM, async_op=True)
        works.append((w_pay, w_red))
    model.optimizer.set_visibility_and_N(cx.vis, model.P)
    for c, (p0, p1) in enumerate(cx.bounds):
        n = p1 - p0
        w_pay, w_red = works[c]
        w_pay.wait()
        pa = cx.pay_all[c]
        cx.vis[p0:p1] = pa[:, 12 * n + 12:12 * n + 12 + n].max(0).values
        rgb0 = pa[0, :12 * n].view(torch.float32)
        cam0 = pa[0, 12 * n:12 * n + 12].view(torch.float32)
        model.optimizer.step_sh_from_rgb(xyz, cam0, rgb0, model.sh_degree, n_views=n_world, view_stride=pa.shape[1] // 4, rows=(p0, p1))
        w_red.wait()
        sm = cx.small.data_ptr() + 4 * cx.small_off[c]
        model.optimizer.step(None, only=[0, 3, 4, 5], rows=(p0, p1), grad_addr={0: sm, 3: sm + 12 * n, 4: sm + 16 * n, 5: sm + 28 * n})
    _dist_mark("end")
    return cx.vis.bool()


def allreduce_gradients(grads, visible):
    """The per-step exchange: SUM of the concatenated gradient slab [P x (11+3K)] and MAX (= OR) of the visibility
    bytes.  One collective each; returns (list of reduced gradient views, reduced visibility)."""
    flat = torch.cat([g.reshape(-1) for g in grads])
    vis = visible.to(torch.uint8)
    torch.distributed.all_reduce(flat, op=torch.distributed.ReduceOp.SUM)
    torch.distributed.all_reduce(vis, op=torch.distributed.ReduceOp.MAX)
    out, off = [], 0
    for g in grads:
        n = g.numel()
        out.append(flat[off:off + n].view_as(g))
        off += n
    return out, vis.bool()


def training_step(model, camera, gt_image, bg, lambda_dssim=LAMBDA_DSSIM, do_step=True, raw_render=None, one_node_loss=False, gt_depth=None,
                  lambda_depth=0.0, weight=None, grad_stats=None, depth_weight=None, depth_huber=0.0, exposure=None, view=0):
    """One iteration of optimize()'s loop (gaussian.cpp:674-716) the way the reference's host writes it: render -> 0.8*L1 + 0.2*(1-SSIM) ->
    loss.backward() -> sparse Adam, on LibTorch autograd.  Returns (loss tensor, visible mask).
    raw_render: passed to render() — None = its default (the drop-in renderer: activations inside the kernels), False = renderer.cpp as written
    (getOpacity / getScaling / getRotation as LibTorch ops, the pure operator path).  one_node_loss: the optional loss_utils.l1_ssim_loss node
    instead of the reference's l1_loss + fused_ssim lines (gaussian.cpp:685-691).
    gt_depth [H,W] (0 = no measurement, e.g. Camera.project_depth of the LiDAR points) with lambda_depth > 0 (not in the reference): the
    rendered depth (render(return_depth=True)) is supervised too, loss += lambda_depth * depth_l1(depth, gt_depth).  gt_depth=None or
    lambda_depth=0 is exactly the colour-only step (no depth is rendered).
    weight [H,W] (not in the reference; a mask is the 0/1 case, clamped to [0,1]): the colour terms become the weighted means
    (w |d|).sum() / (3 S) and (FusedSSIMMap w).sum() / (3 S), S = w.sum() (both 0 when S == 0), from the existing operators; None = the plain means.
    grad_stats (a GradientStats of this model; single GPU): this view's dL_dmeans2D — screenspace_points.grad, or on the raw path what its backward
    node writes out — and radii are added to it by one small kernel (GradientStats.accumulate_from); the step itself is unchanged.
    depth_weight [H,W] / depth_huber (with gt_depth; not in the reference): the depth term becomes depth_l1(depth, gt_depth, depth_weight, depth_huber),
    the per-pixel weighted mean (NaN, negative and +inf weights read as 0, no clamp at 1) of the smooth-L1 of the residual with threshold depth_huber
    (0 = L1); None and 0 are exactly the unweighted term.
    exposure (a trainer.Exposure; single GPU) / view: the loss is taken of loss.apply_exposure(image, E_view) — one more autograd node, on
    gslic_exposure_apply / _backward — which is what the reference's host asks for with apply_exposure and never gets; exposure.grad is then dL/dE
    and do_step also steps E_view by torch.optim.Adam's rule (Exposure.adam_step, as the reference's exposure_optimizer_).  The depth image is not
    touched.  None is exactly the step without it."""
    use_depth = _use_depth("training_step", gt_depth, lambda_depth, depth_weight, depth_huber)
    exposure = _check_exposure("training_step", exposure, view)
    grad_stats = _grad_stats_for_step(grad_stats, model)
    m2d = {} if grad_stats is None else dict(mean2d_grad_out=grad_stats._mean2d_buffer())
    if use_depth:
        image, _final_T, _pts, visible, _radii, depth = render(camera, model, bg, raw=raw_render, return_depth=True, **m2d)
    else:
        image, _final_T, _pts, visible, _radii = render(camera, model, bg, raw=raw_render, **m2d)
    if exposure is not None:
        E = exposure.matrix(view).detach().clone().requires_grad_(True)
        image = loss_utils.apply_exposure(image, E)
    if one_node_loss:
        loss = loss_utils.l1_ssim_loss(image, gt_image, lambda_dssim, weight)
    elif weight is not None:
        w = loss_utils.clamp_weight(weight.detach())
        n = (3.0 * w.sum()).clamp_min(torch.finfo(torch.float32).tiny)
        Ll1 = (w * torch.abs(image - gt_image)).sum() / n
        ssim_value = (loss_utils.FusedSSIMMap.apply(loss_utils.C1, loss_utils.C2, image.unsqueeze(0), gt_image.unsqueeze(0)) * w).sum() / n
        loss = (1.0 - lambda_dssim) * Ll1 + lambda_dssim * (1.0 - ssim_value)
    else:
        Ll1 = loss_utils.l1_loss(image, gt_image)
        ssim_value = loss_utils.fused_ssim(image.unsqueeze(0), gt_image.unsqueeze(0))
        loss = (1.0 - lambda_dssim) * Ll1 + lambda_dssim * (1.0 - ssim_value)
    if use_depth:
        loss = loss + lambda_depth * loss_utils.depth_l1(depth, gt_depth, depth_weight, depth_huber)
    loss.backward()
    if exposure is not None:
        exposure.grad.copy_(E.grad)
        if do_step:
            exposure.adam_step(view, E.grad)
    if grad_stats is not None:
        grad_stats.accumulate_from(_pts.grad if _pts.grad is not None else m2d["mean2d_grad_out"], _radii)
    if do_step:
        params = model.parameters()
        grads = [p.grad if p.grad is not None else torch.zeros_like(p) for p in params]
        if _dist_on():
            grads, visible = allreduce_gradients(grads, visible)
        model.optimizer.set_visibility_and_N(visible, model.xyz.size(0))
        model.optimizer.step(grads)
        model.optimizer.zero_grad(True)
    return loss.detach(), visible


def pose_gradient(model, camera, gt_image, bg, fused_loss=None, gt_depth=None, lambda_depth=0.0, weight=None, depth_weight=None, depth_huber=0.0,
                  exposure=None, view=0, poses=None, do_step=False, shared=False):
    """dL/dxi of the training loss w.r.t. a left se(3) increment of the camera pose (Camera.pose_gradient) for the current map: forward -> loss
    kernels -> gslic_rasterize_backward_camera -> the chain.  The map is not touched.  Returns (float64 [6] = (d/drho, d/dphi), terms).
    One step of pose refinement is `camera.apply_pose_increment(-lr * g); camera.to_device(dev)`.
    gt_depth [H,W] with lambda_depth != 0 (LiDAR depth supervision, as training_step_fused's): the loss gains lambda_depth * depth_l1 and the
    gradient its share — depth forward -> colour and depth loss kernels -> gslic_rasterize_backward_depth_camera -> the same chain; terms is
    then [mean L1, mean SSIM, L_d].  gt_depth=None or lambda_depth=0 is exactly the colour-only path.
    weight [H,W]: the weighted colour loss (FusedLoss.forward_backward); it combines freely with gt_depth.
    depth_weight [H,W] / depth_huber: the weighted / Huber depth term, as training_step_fused's.
    exposure / view: the loss of the exposure-compensated image, as training_step_fused's; exposure.grad is written, E is not updated.
    poses (a trainer.PoseSet) / view: the render is from row `view` of the set (`camera` supplies only the intrinsics and must match the set's) and
    the chain runs on the device (gslic_pose_step, one launch behind the backward): returns (poses.grad [6] float32 DEVICE tensor, terms) with no
    synchronisation and no host copy.  do_step=True also steps the row (Adam and the retraction, in the same launch); view names the exposure's
    row as well when both are given.
    shared=True (with poses=, a set built with shared=True): gslic_pose_step_shared runs in place of gslic_pose_step — the same chain on row `view`,
    then g_tau = xi_view . g; do_step=True steps the shared extrinsic / time-offset coordinates and moves EVERY row.  Returns
    (poses.shared_grad [7] float32 DEVICE tensor, terms).  Per-view and shared training in one step are not offered."""
    fl = fused_loss or _default_fused_loss()
    use_depth = _use_depth("pose_gradient", gt_depth, lambda_depth, depth_weight, depth_huber)
    exposure = _check_exposure("pose_gradient", exposure, view)
    poses = _check_poses("pose_gradient", poses, view, camera, shared)
    if poses is None and do_step:
        raise ValueError("pose_gradient: do_step=True needs poses= (a trainer.PoseSet holds the optimiser's state)")
    with torch.no_grad():
        rr = _RawRaster(model, camera, bg, use_depth, pose=None if poses is None else poses.pose(view))
        image, depth, _radii = rr.forward()
        dL_dimage, dL_ddepth, terms = _fused_losses(fl, image, gt_image, depth, gt_depth, float(lambda_depth), weight, depth_weight, depth_huber,
                                                    exposure, view, False)
        out = rr.backward(dL_dimage, dL_ddepth, camera_grads=True)
        if poses is not None:
            return (poses._step_shared if shared else poses._step)(view, out[9:12], do_step), terms
    return camera.pose_gradient(out[9], out[10], out[11]), terms


def training_step_with_pose(model, camera, gt_image, bg, pose_lr=0.0, fused_loss=None, gt_depth=None, lambda_depth=0.0, weight=None, grad_stats=None,
                            depth_weight=None, depth_huber=0.0, exposure=None, view=0, poses=None, adam_in_backward=False, shared=False):
    """One joint map + pose iteration: forward -> loss kernels -> gslic_rasterize_backward_camera (parameter gradients AND the camera gradient in
    one pass) -> masked Adam on the map -> `camera` moved by -pose_lr * dL/dxi (left se(3) increment; 35 floats cross to the host, which is the
    step's only synchronisation).  Returns (terms, visible, dL/dxi).
    gt_depth [H,W] with lambda_depth != 0: the same step under LiDAR depth supervision (depth forward, colour and depth loss kernels,
    gslic_rasterize_backward_depth_camera); the map update equals training_step_fused(gt_depth=...)'s, terms is [mean L1, mean SSIM, L_d].
    gt_depth=None or lambda_depth=0 is exactly the colour-only step.  weight [H,W]: the weighted colour loss, as training_step_fused's.
    grad_stats (a GradientStats of this model): the backward also writes dL_dmeans2D, which one small kernel adds to the statistics.
    depth_weight [H,W] / depth_huber: the weighted / Huber depth term, as training_step_fused's.
    exposure / view: the exposure model of the view, applied and updated as training_step_fused's.
    poses (a trainer.PoseSet) / view: the same joint iteration on row `view` of the set — the render is from the row (`camera` supplies only the
    intrinsics and must match the set's), and the pose step is ONE launch behind the map's Adam (gslic_pose_step: chain, Adam on the six tangent
    coordinates with the set's two rates, retraction): no host copy of the 35 floats, no numpy, no to_device, no synchronisation.  Returns
    (terms, visible, poses.grad [6] float32 DEVICE tensor).  pose_lr != 0 together with poses= raises (the set has its own rates); with exposure=
    as well, view names both rows.
    adam_in_backward=True: the map's Adam runs inside the backward that also returns the camera gradient (gslic_rasterize_backward_camera_adam /
    _depth_camera_adam): the ten gradients are neither written to the slab nor read back and SparseGaussianAdam.step's launches go away.  The
    camera gradient is that of the map before its update; parameters, moments, the mask and the pose step are bit-identical to the default's.
    `visible` is the mask the kernel wrote; the pose step follows unchanged, through poses= or pose_lr.  It combines with gt_depth, weight,
    depth_weight, depth_huber, exposure and grad_stats (the backward then writes dL_dmeans2D too, and the same small kernel adds it).  Single GPU
    only (NotImplementedError under the N > 1 exchange).  False (the default) is the step as it was, launch for launch.
    shared=True (with poses=, a set built with shared=True): the pose launch is gslic_pose_step_shared — the view's gradient steps the shared
    extrinsic / time-offset coordinates and EVERY row of the set moves; the per-view moments are not touched.  Returns (terms, visible,
    poses.shared_grad [7]).  It combines with everything the per-view step combines with, adam_in_backward included; False is the step as it was."""
    fl = fused_loss or _default_fused_loss()
    use_depth = _use_depth("training_step_with_pose", gt_depth, lambda_depth, depth_weight, depth_huber)
    exposure = _check_exposure("training_step_with_pose", exposure, view)
    poses = _check_poses("training_step_with_pose", poses, view, camera, shared)
    pose_step = None if poses is None else (poses._step_shared if shared else poses._step)
    if poses is not None and pose_lr:
        raise ValueError("training_step_with_pose: pose_lr != 0 given together with poses= (the pose set steps by its own lr_rot / lr_trans)")
    if adam_in_backward and _dist_on():
        raise NotImplementedError("training_step_with_pose(adam_in_backward=True) is single-GPU only: under the N > 1 exchange the gradients "
                                  "travel between the backward and the Adam update")
    grad_stats = _grad_stats_for_step(grad_stats, model)
    cam = camera
    with torch.no_grad():
        if adam_in_backward:
            rr = _RawRaster(model, cam, bg, use_depth, pose=None if poses is None else poses.pose(view))
            image, depth, radii = rr.forward()
            dL_dimage, dL_ddepth, terms = _fused_losses(fl, image, gt_image, depth, gt_depth, float(lambda_depth), weight, depth_weight, depth_huber,
                                                        exposure, view)
            vis_u8 = torch.empty(model.P, dtype=torch.uint8, device=model.device)
            m2d = None if grad_stats is None else grad_stats._mean2d_buffer()
            out = rr.backward(dL_dimage, dL_ddepth, adam=model.optimizer.fused_descriptor(visible_out=vis_u8),
                              xyz_grad=_depth_xyz_grad(model) if use_depth else None, camera_grads=True, mean2d_out=m2d)
            if grad_stats is not None:
                grad_stats.accumulate_from(m2d, radii)
            model.optimizer.count_step()
            visible = vis_u8.view(torch.bool)
            if poses is not None:
                return terms, visible, pose_step(view, out)
            g = cam.pose_gradient(*out)
            if pose_lr:
                cam.apply_pose_increment(-float(pose_lr) * g).to_device(model.device)
            return terms, visible, g
        if use_depth:
            _grad_slab(model)   # (the depth step sets the slab up ahead of its forward, the colour step behind its loss: both as they were)
        rr = _RawRaster(model, cam, bg, use_depth, pose=None if poses is None else poses.pose(view))
        image, depth, radii = rr.forward()
        dL_dimage, dL_ddepth, terms = _fused_losses(fl, image, gt_image, depth, gt_depth, float(lambda_depth), weight, depth_weight, depth_huber,
                                                    exposure, view)
        slab = _grad_slab(model)
        out = rr.backward(dL_dimage, dL_ddepth, out=slab.views, camera_grads=True, mean2d_out=None if grad_stats is None else grad_stats._mean2d_buffer())
        if grad_stats is not None:
            grad_stats.accumulate_from(out[0], radii)
        visible = radii > 0
        model.optimizer.set_visibility_and_N(visible, model.P)
        model.optimizer.step(slab.grads(model))
        if poses is not None:
            return terms, visible, pose_step(view, out[9:12])
        g = cam.pose_gradient(out[9], out[10], out[11])
        if pose_lr:
            cam.apply_pose_increment(-float(pose_lr) * g).to_device(model.device)
    return terms, visible, g


def training_step_fused(model, camera, gt_image, bg, fused_loss=None, do_step=True, adam_in_backward=True, gt_depth=None, lambda_depth=0.0,
                        weight=None, grad_stats=None, depth_weight=None, depth_huber=0.0, exposure=None, view=0):
    """The same iteration as training_step — identical arithmetic up to fp32 rounding — on the fused entry points
    (SURVEY.md §8f row 2): sigmoid / exp / normalize and their backward run inside preprocess / preprocess_bwd (raw_params),
    the loss and dL/dimage come from two loss kernels, and there is no autograd graph: 0 LibTorch elementwise launches per step
    (the drop-in path issues ~35).  Returns (terms [mean L1, mean SSIM] device tensor, visible mask).
    gt_depth [H,W] with lambda_depth != 0 (LiDAR depth supervision, as training_step's): the depth forward, the two colour-loss and the two
    depth-loss kernels (gslic_depth_l1_loss_forward_backward), then the depth backward with the Adam update inside
    (gslic_rasterize_backward_depth_adam) or, adam_in_backward=False, the depth backward and SparseGaussianAdam.step; terms is then
    [mean L1, mean SSIM, L_d] and the loss FusedLoss.value(terms, lambda_depth).  gt_depth=None or lambda_depth=0 is exactly the colour-only
    step.  Single GPU only: the N > 1 exchange carries no depth gradient (NotImplementedError).
    weight [H,W] float (a mask is the 0/1 case): the colour loss becomes the weighted one (FusedLoss.forward_backward(weight=...): three loss
    launches instead of two, terms the weighted means, FusedLoss.weight_sum the sum of the weights); it combines freely with gt_depth and, the
    loss being rank-local, with N > 1.  weight=None is exactly the unweighted step.
    grad_stats (a GradientStats of this model; single GPU): the view is added to the densification statistics — with the Adam update inside the
    backward by that kernel itself (gslic_rasterize_backward_adam_stats / _depth_adam_stats: the gradient never leaves it), otherwise from the
    dL_dmeans2D the backward then also writes (one small kernel).  Parameters and moments are bit-identical with and without it; None is today's
    step, launch for launch.
    depth_weight [H,W] float32 and / or depth_huber > 0 (with gt_depth): the depth term becomes the weighted mean, over the measured pixels, of the
    smooth-L1 of the residual with threshold depth_huber (0 = L1) — FusedLoss.depth_forward_backward(weight=, huber=), the two launches of
    gslic_depth_loss_weighted_forward_backward in place of the two of the unweighted call, plus a 4-byte copy.  NaN, negative and +inf weights read
    as 0 and there is NO clamp at 1 (unlike `weight`); a pixel of weight 0 is an unmeasured pixel; FusedLoss.depth_weight_sum is the sum of the
    weights.  `weight` does not reach the depth term and depth_weight does not reach the colour terms.  depth_weight=None with depth_huber=0 is
    exactly today's depth step, launch for launch.  Without gt_depth they raise; single GPU only, like gt_depth.
    exposure (a trainer.Exposure) / view (the row of it this view uses): the loss is taken of the exposure-compensated image — gslic_exposure_apply
    into a scratch image of the FusedLoss, the loss calls above unchanged on that image, then gslic_exposure_backward, which hands the rasteriser's
    backward E^T dL/dout, leaves dL/dE in exposure.grad and, in its second launch, steps the view's row by torch-style Adam (bias-corrected, as the
    reference's exposure optimiser): three more launches per step.  It combines freely with weight, gt_depth, depth_weight, depth_huber and
    grad_stats; the depth image is not touched, and the SSIM statistics see the compensated image.  do_step=False computes exposure.grad and
    updates nothing.  Single GPU only: under the N > 1 exchange it raises NotImplementedError, because the exchange carries no exposure gradient
    (each rank would step its own copy of E from its own view and the replicas would part).  exposure=None is exactly today's step, launch for
    launch."""
    exposure = _check_exposure("training_step_fused", exposure, view)
    fl = fused_loss or _default_fused_loss()
    # (ahead of _use_depth: under the exchange a depth weight or threshold is refused as depth supervision is, with or without a depth target)
    if ((gt_depth is not None and lambda_depth != 0.0) or depth_weight is not None or depth_huber) and _dist_on():
        raise NotImplementedError("training_step_fused with depth supervision is single-GPU only: the N > 1 gradient exchange (rank1 / slab "
                                  "all-reduce) carries no depth gradient; use training_step(gt_depth=...) or run on one GPU")
    use_depth = _use_depth("training_step_fused", gt_depth, lambda_depth, depth_weight, depth_huber)
    grad_stats = _grad_stats_for_step(grad_stats, model)
    dev = model.device
    cam = camera
    if DIST_TIMING is not None and do_step and _dist_on():
        _dist_mark("start")
    with torch.no_grad():
        rr = _RawRaster(model, cam, bg, use_depth)
        image, depth, radii = rr.forward()
        dL_dimage, dL_ddepth, terms = _fused_losses(fl, image, gt_image, depth, gt_depth, float(lambda_depth), weight, depth_weight, depth_huber,
                                                    exposure, view, do_step)
        if do_step and adam_in_backward and not _dist_on():
            # single GPU: nothing to exchange, so the Adam update runs inside the per-Gaussian backward kernel while the
            # gradients are still in registers / LDS (bit-identical to backward + SparseGaussianAdam.step, ~2 GB less HBM traffic);
            # under depth supervision every group but xyz there, xyz once dL/dz is in (its gradient is assembled in a buffer kept on the model)
            xg = _depth_xyz_grad(model) if use_depth else None
            vis_u8 = torch.empty(model.P, dtype=torch.uint8, device=dev)
            rr.backward(dL_dimage, dL_ddepth, adam=model.optimizer.fused_descriptor(visible_out=vis_u8), xyz_grad=xg,
                        grad_stats=None if grad_stats is None else grad_stats._descriptor())
            model.optimizer.count_step()
            return terms, vis_u8.view(torch.bool)   # `radii > 0` (renderer.cpp:85), written by the backward kernel: no compare launch
        slab = _grad_slab(model)
        mode = exchange_mode() if (do_step and _dist_on()) else None
        if mode == "rank1" and exchange_chunks() > 1 and os.environ.get("GSLIC_RANK1_SPLIT_ADAM") != "1":
            visible = training_step_rank1_chunked(model, cam, bg, dL_dimage, rr.state, exchange_chunks())
            return terms, visible
        if mode == "rank1":
            # the SH gradients travel as the 3-float colour gradient they are the outer product of (exchange_rank1);
            # mask and camera centre of the all-gather payload come out of the same kernel
            rr.backward(dL_dimage, out=slab.views, rgb_out=slab.rgb, payload=(slab.pay_vis, slab.pay_campos))
            _dist_mark("bwd_done")
            visible, works = exchange_rank1(slab, slab.rgb, None, model, None)
            model.optimizer.set_visibility_and_N(visible, model.P)
            grads = slab.grads(model)
            for work, idx in works:
                work.wait()
                model.optimizer.step(grads, only=idx)
            _dist_mark("end")
            return terms, visible
        out = rr.backward(dL_dimage, dL_ddepth, out=slab.views, mean2d_out=None if grad_stats is None else grad_stats._mean2d_buffer())
        if grad_stats is not None:
            grad_stats.accumulate_from(out[0], radii)
        visible = radii > 0
        if do_step:
            if _dist_on():
                _dist_mark("bwd_done")
            if mode == "sparse":
                visible, _rows = allreduce_slab_sparse(slab, visible, model)   # visible rows only: fewer bytes on the links, one gather / scatter pass
                model.optimizer.set_visibility_and_N(visible, model.P)
                model.optimizer.step(slab.grads(model))
            elif mode == "single":
                visible = allreduce_slab_single(slab, visible)                 # ONE collective: slab + mask (north_star's wording)
                model.optimizer.set_visibility_and_N(visible, model.P)
                model.optimizer.step(slab.grads(model))
            elif _dist_on():
                visible, works = allreduce_slab_async(slab, visible, model)
                model.optimizer.set_visibility_and_N(visible, model.P)
                grads = slab.grads(model)
                for work, idx in works:       # Adam on a segment's groups as soon as ITS all-reduce is done
                    work.wait()
                    model.optimizer.step(grads, only=idx)
            else:
                model.optimizer.set_visibility_and_N(visible, model.P)
                model.optimizer.step(slab.grads(model))       # group order of gaussian.cpp:399-418
            if _dist_on():
                _dist_mark("end")
    return terms, visible


_FUSED_LOSS = None


def _default_fused_loss():
    global _FUSED_LOSS
    if _FUSED_LOSS is None:
        _FUSED_LOSS = loss_utils.FusedLoss(LAMBDA_DSSIM)
    return _FUSED_LOSS


def render_fwd_bwd(model, camera, dL_dimage, bg):
    """Bare rendered view forward + backward (the metric's "(fwd+bwd)"), no loss kernels, no optimiser."""
    image, _final_T, _pts, visible, _radii = render(camera, model, bg)
    image.backward(dL_dimage)
    for p in model.parameters():
        p.grad = None
    return visible


class _StepInput:
    """One static input image of GraphedStep — the buffer the step reads and the serial number of its loads — and the rule all four live by.
    load(t) copies a tensor that lives in other storage and counts the copy.  snapshot(t) is what a repeat of a step issued with t needs: the
    tensor by reference with its version counter, or, for t=None ("the one that is loaded"), the serial of the load.  restore(snap) loads it
    again, and refuses when that evidence says the data is no longer what the step ran on.  Tensor operations only."""

    def __init__(self, noun, arg, buffer, loaded_noun=None, check_shape=False):
        """noun: what the messages call the image; arg: step()'s name for it; loaded_noun: the noun of "the one that is loaded" where it
        differs; check_shape: load() refuses a tensor of another shape (else that is copy_'s business)."""
        self.noun, self.loaded_noun, self.arg, self.buffer, self.check_shape = noun, loaded_noun or noun, arg, buffer, check_shape
        self.serial = 0

    def load(self, t):
        if self.check_shape and tuple(t.shape) != tuple(self.buffer.shape):
            raise ValueError(f"GraphedStep: {self.arg} of shape {tuple(t.shape)} given to a step built for {tuple(self.buffer.shape)}")
        if t.data_ptr() != self.buffer.data_ptr():
            self.buffer.copy_(t)
            self.serial += 1

    def snapshot(self, t):
        return (t, None if t is None else t._version, self.serial)

    def restore(self, snap):
        t, version, serial = snap
        if t is None:
            if serial != self.serial:
                raise RuntimeError(f"GraphedStep: a step that has to be repeated ran on a {self.loaded_noun} that has been replaced since (it was "
                                   f"issued with {self.arg}=None); pass it explicitly to step() when it changes between checks")
            return
        if t._version != version:
            raise RuntimeError(f"GraphedStep: the {self.noun} of a step that has to be repeated was modified in place after the step was issued")
        self.load(t)


class GraphedStep:
    """training_step_fused captured in a hipGraph: forward in capacity mode (gslic_rasterize_forward_capacity: no host round trip, the
    reference blocks twice per forward, rasterizer_impl.cu:398,442) -> loss kernels -> backward with the Adam update inside, replayed
    with ONE launch per step.  Camera matrices and the ground-truth image are read from static device buffers that `step()` refreshes
    before the replay.  Single GPU (the N > 1 path has an exchange between backward and Adam and runs eagerly).

    The scratch capacities come from one eager forward (R, B) with `headroom`; the instance / bucket counts of a step stay on the
    device.  If they outgrow the buffers the step turns itself into a no-op (status bits; no gradients, no Adam) and `check()` —
    called every `check_every` steps (at most 32: the device keeps one did-not-fit bit per issued step), and by the caller at the
    end — grows the buffers from the largest counts seen, re-captures and repeats exactly the steps that did not fit, each with ITS
    pose (snapshotted by value) and ground truth (kept by reference with its version counter: a target that was modified in place, or
    replaced while steps were issued with gt_image=None, makes the repeat fail loudly instead of training on the wrong data), after the
    ones that did.  extend() and prune() change P / the rows: build a new GraphedStep afterwards (step() raises otherwise).

    gt_depth [H,W] with lambda_depth != 0 (LiDAR depth supervision): the step is training_step_fused's depth step in capacity mode
    (gslic_rasterize_forward_depth_capacity -> colour and depth loss kernels -> gslic_rasterize_backward_depth_adam).  lambda_depth is baked
    into the step; the depth target lives in a static buffer like the image and is passed to step() the same way (and repeated steps use their
    own, checked by reference and version counter like gt_image).  terms is then [mean L1, mean SSIM, L_d].

    weight [H,W]: the step runs the weighted colour loss (training_step_fused(weight=...)).  Whether it does is baked into the step; the weight
    image lives in a static buffer like the depth target and is passed to step() the same way (None = the one that is loaded), under the same
    checks when a step is repeated.  A step built without a weight raises when it is handed one; a step built with one raises on weight=False.

    depth_weight [H,W] / depth_huber (with gt_depth and lambda_depth != 0): the step runs the weighted / Huber depth loss
    (training_step_fused(depth_weight=, depth_huber=)).  depth_weight lives in a static buffer exactly as `weight` does and is replaced through
    step(depth_weight=...) under the same checks; a step built without one raises when it is handed one.  depth_huber is an argument of the kernels
    inside the step and so fixed when the step is built.

    exposure (a trainer.Exposure) / view: the step runs training_step_fused(exposure=, view=)'s calls.  Which row a step uses is a device int32 that
    step(view=...) fills (None = the one that is loaded), so a captured graph changes views without being re-captured: the step first gathers the
    row into a fixed 12-float buffer (one index_select launch, inside the step), applies it from there, and the exposure backward's second launch
    updates the row the word names.  A step that did not fit its buffers updates no row either (the descriptor's skip word is the forward's
    status word) and is repeated with its own view.  Eager and captured runs issue the same calls.

    keyframes (a trainer.KeyframeStore) / frame / level, with gt_image=None: the step's static target is filled INSIDE the step by the store's
    decode launch (gslic_keyframe_decode at `level`) from the slot a device int32 names; step(camera, frame=j) fills that word (None = the one that
    is loaded) and that is all a change of target costs — no 25 MB copy, no re-capture.  The step is built at camera.at_level(level) resolution: a
    camera of the store's full size is converted, one that already has the level's size is used as it is.  A store with masks feeds the step's
    weight buffer from the same launch: the step is then a weighted step.  The launch is given the store's CAPACITY as its frame count (frames
    added after a capture stay reachable); the index is validated against the filled slots on the host before the word is written.  A repeated step
    uses its own frame index and the slot's serial number: a slot replaced (put) since the step was issued fails loudly.  gt_image together with
    a store, or frame given to a step built without one, raises.  Without keyframes the step is what it was, launch for launch.
    A store with depths under lambda_depth != 0: the step is the depth step, and its static gt_depth buffer — with depth weights its depth_weight
    buffer too — is filled by ONE gslic_keyframe_decode_depth launch right behind the colour decode, from the same frame word: step(frame=j)
    changes colour target, mask, depth target and depth weight together.  gt_depth= given to such a step (at construction or in step()) raises,
    and so does depth_weight= on a store with depth weights; depth_weight= on a depth store without them is host-loaded as ever.  put_depth bumps
    the slot's serial number like put.  lambda_depth == 0, or a store without depths, is the step as it was, launch for launch.

    poses (a trainer.PoseSet) / view: the step READS its pose from the set: one gslic_pose_load launch inside the step fills the static view / proj /
    campos buffers from the row a device int32 names; step(view=j) fills that word (and the exposure's, when there is one: view names both rows),
    so a captured graph changes keyframe pose without a host copy or a re-capture.  `camera` supplies the intrinsics and must match the set's;
    step(camera=...) on such a step raises.  A repeated step (the overflow window) repeats with its view index and reads the row AS IT IS THEN — a
    pose step issued since moves the repeat with it.  poses=None is the step as it was, launch for launch.

    train_pose=True (with poses): the step is the joint map + pose iteration, training_step_with_pose(poses=, adam_in_backward=True) in capacity
    mode.  Its launches, in order: gslic_pose_load, the capacity forward, the loss kernels, gslic_rasterize_backward_camera_adam (or
    _depth_camera_adam) into a static 35-float buffer, gslic_pose_step on the same device word — so step(view=j) changes the row that is rendered
    from AND trained without a re-capture.  The skip word of the pose step is the forward's status word, exactly as the exposure backward's is: a
    step that did not fit moves neither map nor pose (its camera gradient is zeros) and check() repeats it with its view index.  The warm-up and
    capture passes run the step, so the set's state (view, proj, campos, m, v, steps, grad) is saved and restored around them like the map's.
    train_pose=True without poses raises ValueError; with grad_stats it raises NotImplementedError (the camera kernel accumulates no statistics,
    and the small statistics kernel has no overflow word: a step that did not fit would add stale gradients).  train_pose="shared" (a set built with
    shared=True): the same launches with the last one replaced by gslic_pose_step_shared — training_step_with_pose(shared=True,
    adam_in_backward=True) in capacity mode: the view's gradient steps the shared extrinsic / time-offset coordinates and every row moves.  Its skip
    word is the forward's status word too, so a step that did not fit moves nothing and is repeated; the set's shared state (sm, sv, ssteps, X, tau,
    shared_grad) is saved and restored around the warm-up and capture passes with the rest.  On a set without shared=True it raises ValueError, with
    grad_stats NotImplementedError, as True does.  train_pose=False: the step does
    not train the pose — pose steps are then issued between graphed steps through pose_gradient(..., poses=, do_step=True) or
    training_step_with_pose(poses=) — and is the step as it was, launch for launch.

    covis (a trainer.Covisibility of this model, with keyframes): ONE gslic_covis_record launch behind the backward (behind the pose step under
    train_pose; it is independent of the camera kernel) replaces the column of the slot the step trained on — column = slot, so covis.n_frames must
    be at least the store's capacity — by radii > 0 of the step's own forward, read from the capacity buffers; the column is named by the store's
    frame word, so step(frame=j) changes target and recorded column together, eager and captured.  Its skip word is the forward's status word: a
    step that did not fit records nothing, and check() repeats it with its frame.  The warm-up and capture passes record too, so the one word per
    row that holds the loaded slot's column is saved and restored around them: building or re-capturing a step leaves no record behind.  covis
    without keyframes raises ValueError (a host without a store calls covis.record(frame, step.visible)); covis=None is the step as it was,
    launch for launch."""

    def __init__(self, model, camera, gt_image, bg, headroom=1.25, check_every=16, cap_R=None, cap_B=None, use_graph=False, gt_depth=None,
                 lambda_depth=0.0, weight=None, grad_stats=None, depth_weight=None, depth_huber=0.0, exposure=None, view=0, keyframes=None,
                 frame=None, level=0, poses=None, train_pose=False, covis=None):
        """use_graph=False (default since round 5): the capacity-mode step (caller-owned scratch, no host round trip, overflow checks and repeats as
        below) issued as eager launches; use_graph=True: captured in a hipGraph and replayed with one launch per step.  The two are equally fast at
        2M Gaussians (bench.py: `capacity_eager` / `graphed`; the host runs ahead of the device either way), and the eager form has no hazard:
        on ROCm 7.2 a replay FAULTS (GPU memory access fault) when the host has called torch.cuda.synchronize() and then enqueued ANY other device
        work — a copy, a fill — before it (tools/experiments/graph_check_repro.py, modes B / C / E; a synchronise alone, or a blocking .cpu() copy
        alone, is harmless: modes A / D / F).  A host that uses the graph must keep its own device work off that pattern."""
        assert not _dist_on(), "GraphedStep is the single-GPU path"
        # grad_stats (a GradientStats of this model): every step that fits adds its view to the statistics inside the backward kernel; a step that
        # did not fit touches nothing (and is repeated).  The three arrays are fixed when the step is built: see _issue.
        self.grad_stats = _grad_stats_for_step(grad_stats, model)
        self.use_graph = bool(use_graph)
        self.model, self.bg, self.headroom, self.check_every = model, bg, float(headroom), int(check_every)
        dev = model.device
        self.keyframes, self.level = keyframes, int(level)
        # a store with depths under lambda_depth != 0: the depth target (and the store's depth weight) is decoded inside the step as well
        self._kf_depth = isinstance(keyframes, KeyframeStore) and keyframes.has_depths and lambda_depth != 0.0
        # covis (a Covisibility of this model, with keyframes): every step that fits records radii > 0 into the column of the slot it trained on
        self.covis = _covis_for_step(covis, model, keyframes if isinstance(keyframes, KeyframeStore) else None)
        if keyframes is None:
            if frame is not None or self.level != 0:
                raise ValueError("GraphedStep: frame / level given without keyframes (pass a trainer.KeyframeStore)")
            self._kf_host = None
        else:
            if not isinstance(keyframes, KeyframeStore):
                raise ValueError("GraphedStep: keyframes must be a trainer.KeyframeStore")
            if gt_image is not None:
                raise ValueError("GraphedStep: gt_image given together with keyframes (the step decodes its target from the store: pass gt_image=None "
                                 "and frame=)")
            if weight is not None and keyframes.has_masks:
                raise ValueError("GraphedStep: weight given together with a keyframe store that has masks (the store's mask is the step's weight)")
            if self._kf_depth and gt_depth is not None:
                raise ValueError("GraphedStep: gt_depth given together with a keyframe store that has depths (the step decodes its depth target "
                                 "from the store, from the same frame word)")
            if self._kf_depth and depth_weight is not None and keyframes.has_depth_weights:
                raise ValueError("GraphedStep: depth_weight given together with a keyframe store that has depth weights (the store's depth weight "
                                 "is the step's)")
            self._kf_size = keyframes.level_size(self.level)
            self._kf_host = keyframes._index(0 if frame is None else frame)
            self._kf_word = torch.full((1,), self._kf_host, dtype=torch.int32, device=dev)
            camera = self._kf_camera(camera)
        self.H, self.W = int(camera.image_height), int(camera.image_width)
        self.cam = camera
        self.view = camera.d_world_view_transform.clone()
        self.proj = camera.d_full_proj_transform.clone()
        self.campos = camera.d_camera_center.clone()
        self._pose_host = self._pose_of(camera)
        self.poses = _check_poses("GraphedStep", poses, view, camera)
        if isinstance(train_pose, str) and train_pose != "shared":
            raise ValueError(f"GraphedStep: train_pose = {train_pose!r} must be False, True or \"shared\"")
        self.train_pose = bool(train_pose)
        self._pose_shared = train_pose == "shared"   # the pose launch is gslic_pose_step_shared: every row moves
        if self.train_pose and self.poses is None:
            raise ValueError("GraphedStep: train_pose=True needs poses= (a trainer.PoseSet holds the rows and the optimiser's state)")
        if self._pose_shared and not self.poses.shared:
            raise ValueError("GraphedStep: train_pose=\"shared\" on a pose set built without shared=True")
        if self.train_pose and self.grad_stats is not None:
            raise NotImplementedError("GraphedStep: train_pose=True together with grad_stats (the camera kernel accumulates no statistics, and the "
                                      "small statistics kernel has no overflow word: a step that did not fit would add stale gradients)")
        self._cam_grads = torch.zeros(35, dtype=torch.float32, device=dev) if self.train_pose else None   # the backward's three camera outputs
        self._pose_view_host = None if self.poses is None else int(view)                     # the row that is loaded
        if self.poses is not None:
            self._pose_word = torch.full((1,), int(view), dtype=torch.int32, device=dev)     # which row: filled by _load
            self.poses._load_row(self._pose_word, self.view, self.proj, self.campos)         # (the sizing forward below renders from the row)
            self._pose_host = None                                                           # the pose is the row's, read inside the step
        kf_weight = None
        if keyframes is None:
            self.gt = gt_image.clone()
        else:
            self.gt, kf_weight = keyframes.target_buffers(self.level)   # filled by the decode launch inside the step
        kf_gt_depth, kf_depth_weight = keyframes.depth_target_buffers(self.level) if self._kf_depth else (None, None)   # filled by the depth decode launch
        self.use_depth = _use_depth("GraphedStep", kf_gt_depth if self._kf_depth else gt_depth, lambda_depth, depth_weight, depth_huber)
        self.lambda_depth = float(lambda_depth) if self.use_depth else 0.0
        self.depth_weight = depth_weight.detach().float().contiguous().clone() if self.use_depth and depth_weight is not None else kf_depth_weight
        self.depth_huber = float(depth_huber) if self.use_depth else 0.0
        self.gt_depth = kf_gt_depth if self._kf_depth else (gt_depth.detach().float().contiguous().clone() if self.use_depth else None)
        self.use_weight = weight is not None or kf_weight is not None
        self.weight = kf_weight if kf_weight is not None else (weight.detach().float().contiguous().clone() if self.use_weight else None)

        def slot(buffer, noun, arg, **kw):
            return None if buffer is None else _StepInput(noun, arg, buffer, **kw)
        # the four images the step reads from static buffers, under step()'s names for them and in the order a repeat restores them; None: the
        # step was built without that input.  self.gt, .weight, .depth_weight and .gt_depth stay the buffers themselves.
        self._slots = dict(gt_image=slot(self.gt, "ground-truth tensor", "gt_image", loaded_noun="target"),
                           weight=slot(self.weight, "weight image", "weight", check_shape=True),
                           depth_weight=slot(self.depth_weight, "depth weight image", "depth_weight", check_shape=True),
                           gt_depth=slot(self.gt_depth, "depth target", "gt_depth"))
        self.fl = loss_utils.FusedLoss(LAMBDA_DSSIM)
        self.exposure = _check_exposure("GraphedStep", exposure, view)
        self._ex_view_host = None if self.exposure is None else int(view)                    # the row that is loaded
        if self.exposure is not None:
            self._ex_E = torch.empty(1, 12, dtype=torch.float32, device=dev)                  # the row the step applies, gathered inside the step
            self._ex_view = torch.full((1,), int(view), dtype=torch.int32, device=dev)       # which row: filled by _load
        self.e = torch.empty(0, device=dev)
        # sizes from one eager forward of the current state
        with torch.no_grad():
            sizing = _RawRaster(model, camera, bg, False, e=self.e, pose=(self.view, self.proj, self.campos))
            sizing.forward()
            R, B = sizing.state[:2]
        self.cap_R, self.cap_B = int(R * self.headroom) + 65536, int(B * self.headroom) + 1024
        if cap_R is not None:
            self.cap_R = int(cap_R)
        if cap_B is not None:
            self.cap_B = int(cap_B)
        assert self.check_every <= 32, "the device keeps one did-not-fit bit per step of a window of 32"
        self.graph, self.bufs = None, None
        self.steps_issued = 0      # replays since the last check
        self.window = []           # (camera, ground truth) of those replays, in issue order
        self.recaptures = 0
        self._capture()

    def _kf_camera(self, camera):
        """The camera a step on a keyframe store runs at: one of the level's size as it is, one of the store's full size through at_level."""
        size = (int(camera.image_width), int(camera.image_height))
        if size == self._kf_size:
            return camera
        if size != (self.keyframes.width, self.keyframes.height):
            raise ValueError(f"GraphedStep: a {size[0]} x {size[1]} camera given to a step on {self.keyframes.width} x {self.keyframes.height} keyframes "
                             f"at level {self.level} ({self._kf_size[0]} x {self._kf_size[1]})")
        return camera.at_level(self.level)

    def _eager(self):
        if self.keyframes is not None:
            self.keyframes._decode(self._kf_word, self.level, self.gt, self.weight, n_frames=self.keyframes.capacity)
            if self._kf_depth:
                self.keyframes._decode_depth(self._kf_word, self.level, self.gt_depth, self.depth_weight, n_frames=self.keyframes.capacity)
        if self.poses is not None:
            self.poses._load_row(self._pose_word, self.view, self.proj, self.campos)
        rr = _RawRaster(self.model, self.cam, self.bg, self.use_depth, e=self.e, pose=(self.view, self.proj, self.campos))
        image, depth, _radii = rr.forward(self.bufs)
        if self.exposure is None:
            ex_view = 0
        else:
            torch.index_select(self.exposure.params.view(-1, 12), 0, self._ex_view, out=self._ex_E)
            ex_view = (self._ex_E.view(12), self._ex_view, self.bufs.status[2:3])
        dL_dimage, dL_ddepth, self.terms = _fused_losses(self.fl, image, self.gt, depth, self.gt_depth, self.lambda_depth, self.weight, self.depth_weight,
                                                         self.depth_huber, self.exposure, ex_view)
        if self.train_pose:
            cam = rr.backward(dL_dimage, dL_ddepth, adam=self._adam, xyz_grad=self._xyz_grad, camera_grads=True, cam_out=self._cam_grads)
            step_word = self.poses._step_shared_word if self._pose_shared else self.poses._step_word
            step_word(self._pose_word, cam, self.bufs.status[2:3])   # (skip: the forward's overflow word, as the exposure's)
        else:
            rr.backward(dL_dimage, dL_ddepth, adam=self._adam, xyz_grad=self._xyz_grad, grad_stats=self._gstat)
        if self.covis is not None:   # column = the slot the frame word names; a step that did not fit records nothing (skip: the same status word)
            self.covis._record(self._kf_word, radii=self.bufs.radii, skip=self.bufs.status[2:3])

    def _capture(self):
        from . import rasterizer as rz
        dev = self.model.device
        self.bufs = rz.CapacityBuffers(self.model.P, self.W, self.H, self.cap_R, self.cap_B, dev, depth=self.use_depth)
        self._adam = self.model.optimizer.fused_descriptor()
        self._xyz_grad = torch.empty(self.model.P, 3, dtype=torch.float32, device=dev) if self.use_depth else None
        self._gstat = None if self.grad_stats is None else self.grad_stats._descriptor()
        self._gstat_addr = None if self.grad_stats is None else self.grad_stats._addresses()
        # warm-up on a side stream (allocations of the loss scratch, library one-offs), then capture.  The warm-up and the capture
        # pass both execute the step, so the parameters are saved and restored around them.
        names = self.model.NAMES
        saved = [(self.model._buf[n][:self.model.P].clone(), self.model._m[n][:self.model.P].clone(), self.model._v[n][:self.model.P].clone())
                 for n in names]
        saved_stats = [] if self.grad_stats is None else [a.clone() for a, _w in self.grad_stats._arrays()]   # (the two passes are no views of the host's)
        ex = self.exposure
        saved_ex = None if ex is None else [(a, a.clone()) for a in (ex.params, ex.m, ex.v, ex.steps, ex.grad)]
        ps = self.poses if self.train_pose else None
        saved_ps = None if ps is None else [(a, a.clone()) for a in (ps.view, ps.proj, ps.campos, ps.m, ps.v, ps.steps, ps.grad)]
        if self._pose_shared:
            saved_ps += [(a, a.clone()) for a in (ps.sm, ps.sv, ps.ssteps, ps.X, ps.tau, ps.shared_grad)]
        cv = self.covis   # the two passes record into the loaded slot's column: the one word per row that holds it is saved and restored
        self._cv_addr = None if cv is None else cv._bits.data_ptr()
        saved_cv = None if cv is None else cv._bits[:, self._kf_host >> 5].clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            self._eager()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = None
        if self.use_graph:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g), torch.no_grad():
                self._eager()
            torch.cuda.synchronize()
        for n, (p, m1, m2) in zip(names, saved):
            self.model._buf[n][:self.model.P].copy_(p); self.model._m[n][:self.model.P].copy_(m1); self.model._v[n][:self.model.P].copy_(m2)
        for (a, _w), keep in zip(self.grad_stats._arrays() if saved_stats else (), saved_stats):
            a.copy_(keep)
        for a, keep in (saved_ex or []) + (saved_ps or []):
            a.copy_(keep)
        if cv is not None:
            cv._bits[:, self._kf_host >> 5].copy_(saved_cv)
        self.bufs.status.zero_()
        self.graph = g
        self.steps_issued = 0
        self.window = []
        self._captured_layout = (self.model.P, getattr(self.model, "layout_version", 0))   # what the buffers, the Adam descriptor and a graph bake in

    _BAKED = ("tanfovx", "tanfovy", "limx_neg", "limx_pos", "limy_neg", "limy_pos")   # scalars of the camera that are constants of the captured graph

    @staticmethod
    def _pose_of(camera):
        """The three pose arrays of a Camera by VALUE, on the host (they are numpy members of the object: no device work, no allocation on the
        device between two replays)."""
        return (camera.world_view_transform.copy(), camera.full_proj_transform.copy(), camera.camera_center.copy())

    def _load(self, camera, gt_image, gt_depth=None, weight=None, depth_weight=None, view=None, frame=None):
        """Refresh the static buffers the captured step reads.  The pose is copied on every call that names a camera (the same Camera object
        may have been moved in place since it was loaded last)."""
        if self.keyframes is None:
            if frame is not None:
                raise ValueError("GraphedStep: frame given to a step built without a keyframe store (pass keyframes to the constructor)")
        else:
            if gt_image is not None:
                raise ValueError("GraphedStep: gt_image given to a step built on a keyframe store (its target is decoded inside the step: pass frame=)")
            if weight is not None and weight is not False and self.keyframes.has_masks:
                raise ValueError("GraphedStep: weight given to a step whose keyframe store has masks (the store's mask is the step's weight)")
            if gt_depth is not None and self._kf_depth:
                raise ValueError("GraphedStep: gt_depth given to a step whose keyframe store has depths (its depth target is decoded inside the step: "
                                 "pass frame=)")
            if depth_weight is not None and self._kf_depth and self.keyframes.has_depth_weights:
                raise ValueError("GraphedStep: depth_weight given to a step whose keyframe store has depth weights (the store's depth weight is the "
                                 "step's)")
            if frame is not None and self.keyframes._index(frame) != self._kf_host:
                self._kf_host = self.keyframes._index(frame)
                self._kf_word.fill_(self._kf_host)
            if camera is not None:
                camera = self._kf_camera(camera)
        if camera is not None and self.poses is not None:
            raise ValueError("GraphedStep: camera given to a step built on a pose set (its pose is read from the set inside the step: pass view=)")
        if view is not None:
            if self.exposure is None and self.poses is None:
                raise ValueError("GraphedStep: view given to a step built without an exposure or a pose set (pass exposure or poses to the constructor)")
            if self.exposure is not None and self.exposure._index(view) != self._ex_view_host:
                self._ex_view_host = self.exposure._index(view)
                self._ex_view.fill_(self._ex_view_host)
            if self.poses is not None and self.poses._index(view) != self._pose_view_host:
                self._pose_view_host = self.poses._index(view)
                self._pose_word.fill_(self._pose_view_host)
        if weight is False:   # "this step runs without a weight": true only of a step that was built without one
            if self.use_weight:
                raise ValueError("GraphedStep: this step was built with a weight and always runs the weighted loss (pass ones to weigh every pixel "
                                 "alike, or build a step without a weight)")
            weight = None
        for arg, t, without, ctor in (("weight", weight, "one", "weight"), ("depth_weight", depth_weight, "one", "depth_weight"),
                                      ("gt_depth", gt_depth, "depth supervision", "gt_depth / lambda_depth")):
            if t is not None:
                if self._slots[arg] is None:
                    raise ValueError(f"GraphedStep: {arg} given to a step built without {without} (pass {ctor} to the constructor)")
                self._slots[arg].load(t)
        if camera is not None:
            for k in self._BAKED:
                assert float(getattr(camera, k)) == float(getattr(self.cam, k)), f"{k} is baked into the graph"
            self.view.copy_(camera.d_world_view_transform); self.proj.copy_(camera.d_full_proj_transform); self.campos.copy_(camera.d_camera_center)
            self.cam = camera
            self._pose_host = self._pose_of(camera)
        if gt_image is not None:
            self._slots["gt_image"].load(gt_image)

    def _snapshot(self, gt_image=None, gt_depth=None, weight=None, depth_weight=None):
        """What a repeat of this step needs, independent of what the caller does to its objects afterwards: the pose by VALUE (host copies of the
        35 floats that are loaded now), the exposure row and keyframe slot that are loaded (the slot with its serial number), and every image by
        reference together with the evidence that it is still the same data (_StepInput.snapshot: the tensor's version counter; for None — "the
        one that is loaded" — the serial number of the load)."""
        given = dict(gt_image=gt_image, gt_depth=gt_depth, weight=weight, depth_weight=depth_weight)
        kf = self.keyframes
        view = self._ex_view_host if self.poses is None else self._pose_view_host   # (one index names both rows)
        return dict(frame=self._kf_host, frame_serial=None if kf is None else kf.serial(self._kf_host), view=view, pose=self._pose_host,
                    images={arg: slot.snapshot(given[arg]) for arg, slot in self._slots.items() if slot is not None})

    def _load_snapshot(self, snap):
        dev = self.view.device
        if snap["pose"] is not None:   # (None: a step on a pose set reads the row its view index names, inside the step)
            v, p, c = snap["pose"]
            self.view.copy_(torch.from_numpy(v).to(dev)); self.proj.copy_(torch.from_numpy(p).to(dev)); self.campos.copy_(torch.from_numpy(c).to(dev))
            self._pose_host = snap["pose"]
        if snap["view"] is not None:
            self._load(None, None, view=snap["view"])
        if self.keyframes is not None:
            if self.keyframes.serial(snap["frame"]) != snap["frame_serial"]:
                raise RuntimeError(f"GraphedStep: slot {snap['frame']} of the keyframe store was replaced (put) after a step that has to be repeated "
                                   "was issued on it")
            self._load(None, None, frame=snap["frame"])
        for arg, image in snap["images"].items():
            self._slots[arg].restore(image)

    def _issue(self):
        now = (self.model.P, getattr(self.model, "layout_version", 0))
        if now != self._captured_layout:
            raise RuntimeError(f"GraphedStep: the model's rows changed since this step was built (P / layout_version {self._captured_layout} -> {now}: "
                               "extend() or prune()); its buffers, Adam descriptor and graph hold the old row count and addresses — build a new "
                               "GraphedStep")
        if self.grad_stats is not None:
            self.grad_stats._check()
            if self.grad_stats._addresses() != self._gstat_addr:
                raise RuntimeError("GraphedStep: the arrays of the GradientStats were reallocated since this step was built; the step holds the old "
                                   "addresses — build a new GraphedStep")
        if self.covis is not None:
            self.covis._check()
            if self.covis._bits.data_ptr() != self._cv_addr:
                raise RuntimeError("GraphedStep: the array of the Covisibility was reallocated since this step was built; the step holds the old "
                                   "address — build a new GraphedStep")
        if self.graph is not None:
            self.graph.replay()
        else:
            with torch.no_grad():
                self._eager()

    def step(self, camera=None, gt_image=None, gt_depth=None, weight=None, depth_weight=None, view=None, frame=None):
        """One optimiser step (replay).  Returns the device tensor [mean L1, mean SSIM] of this step's loss terms ([mean L1, mean SSIM, L_d]
        with depth supervision; gt_depth: this step's depth target, None = the one that is loaded; weight: this step's weight image, likewise;
        depth_weight: this step's depth weight image, likewise; view: the row of the exposure this step applies and updates and / or the row of
        the pose set it renders from, likewise; frame: the slot of the keyframe store this step trains on, likewise)."""
        self._load(camera, gt_image, gt_depth, weight, depth_weight, view, frame)
        self._issue()
        self.steps_issued += 1
        if len(self.window) < 32:
            self.window.append(self._snapshot(gt_image, gt_depth, None if weight is False else weight, depth_weight))
        self.model.optimizer.count_step()
        if self.check_every and self.steps_issued >= self.check_every:
            self.check()
        return self.terms

    def check(self):
        """Synchronise and read the status words.  Steps that did not fit were no-ops: grow the buffers from the largest counts seen,
        re-capture and repeat THOSE steps — each with the camera and ground truth it was issued with — until all of them fitted.
        Returns the number of steps that had to be repeated."""
        repeated = 0
        for _round in range(8):
            issued, failed_mask, max_R, max_B = self.bufs.read_window()
            _R, _B, bits, good = self.bufs.read_status()
            missed = issued - good
            if missed <= 0:
                break
            # which steps: one bit per issue index while the window is at most 32 steps long; a longer unchecked run (check_every = 0)
            # can only be repeated on the view that is loaded now
            todo = [self.window[i] for i in range(min(issued, len(self.window))) if (failed_mask >> i) & 1] if issued <= 32 else [self._snapshot()] * missed
            self.cap_R = max(self.cap_R, int(max_R * self.headroom) + 65536)
            self.cap_B = max(self.cap_B, int(max_B * self.headroom) + 1024)
            if max_R > 0x7fffffff // 2 or bits & 16:
                raise RuntimeError("GraphedStep: the instance count does not fit 31 bits")
            self.recaptures += 1
            self._capture()                     # (zeroes the status words, empties the window)
            for snap in todo:
                self._load_snapshot(snap)
                self._issue()
                self.steps_issued += 1
                self.window.append(snap)
            repeated += len(todo)
        else:
            raise RuntimeError("GraphedStep: steps keep overflowing their capacity buffers")
        self.bufs.status.zero_()
        self.steps_issued = 0
        self.window = []
        return repeated

    @property
    def visible(self):
        return self.bufs.radii > 0
