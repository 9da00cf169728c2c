"""CPU-only: the pruning surface that needs no device — the two new exports are declared and bound, the activated-domain limits become the
float32 raw-domain thresholds as documented, and gslic_prune_select / gslic_gather_rows reject bad arguments before any device work (no case
here may reach a HIP call: without a GPU it would fail, not pass)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = ctypes.c_void_p


def _libs():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    return _lib, _lib.lib()


def test_header_declares_and_lib_binds_the_two_exports():
    _l, L = _libs()
    src = open(os.path.join(ROOT, "include", "gslic_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("gslic_prune_select", "gslic_gather_rows"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in _l.EXPORTS and hasattr(L, name)
    assert re.search(r"typedef\s+struct\s+gslic_row_array\s*\{\s*const\s+void\s*\*\s*src;\s*void\s*\*\s*dst;\s*uint32_t\s+row_dwords;\s*\}", code)
    assert "#define GSLIC_ABI_VERSION 8" in src and L.gslic_abi_version() == 8     # additive: the ABI number stays
    assert len(L.gslic_prune_select.argtypes) == 20 and len(L.gslic_gather_rows.argtypes) == 5
    assert ctypes.sizeof(_l.RowArray) == 24 and _l.RowArray.row_dwords.offset == 16   # two pointers, one u32, padding: the C layout
    # the rule is stated verbatim in the header
    for line in ("bad[i]  = any of xyz[i,0..2], dc[i,0..2], opacity[i], scaling[i,0..2], rotation[i,0..3] is not finite",
                 "hit[i]  = (drop != NULL && drop[i]) || opacity[i] < opacity_raw_min || max_j scaling[i,j] > scaling_raw_max",
                 "keep[i] = !bad[i] && ((protect != NULL && protect[i]) || !hit[i])"):
        assert line in src, line


def test_profiler_ids_are_appended_behind_the_existing_ones():
    _l, L = _libs()
    names = [L.gslic_profile_kernel_name(i).decode() for i in range(L.gslic_profile_num_kernels())]
    assert names[-2:] == ["prune_select", "gather_rows"]
    assert names.index("depth_loss") == 29 and names.index("extend") == 20 and names.index("preprocess") == 0   # the old ids keep their values


def test_threshold_conversion():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd.trainer import prune_thresholds
    assert prune_thresholds() == (-math.inf, math.inf)
    for p, s in ((0.005, 10.0), (0.05, 3.0), (0.5, 1.0), (1e-7, 1e-3), (0.999, 250.0)):
        lo, hi = prune_thresholds(p, s)
        assert lo == float(np.float32(math.log(p / (1.0 - p)))) and hi == float(np.float32(math.log(s)))   # float64 on the host, rounded once
        assert np.float32(lo) == lo and np.float32(hi) == hi                                                 # ... to float32 values
    assert prune_thresholds(0.5, None) == (0.0, math.inf) and prune_thresholds(None, 1.0) == (-math.inf, 0.0)
    # the float32 threshold, not the double, decides: 0.005 -> logit = -5.2933048...; its float32 neighbours fall on either side
    lo, _ = prune_thresholds(0.005)
    t = torch.tensor([lo], dtype=torch.float32)
    below, above = torch.nextafter(t, torch.tensor([-math.inf])), torch.nextafter(t, torch.tensor([math.inf]))
    assert bool(below < lo) and not bool(t < lo) and not bool(above < lo)
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="min_opacity"):
            prune_thresholds(bad, None)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="max_scale"):
            prune_thresholds(None, bad)


def test_prune_of_an_empty_model_and_bad_limits_without_a_device():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    raw = dict(xyz=torch.zeros(0, 3), scaling=torch.zeros(0, 3), rotation=torch.zeros(0, 4), opacity=torch.zeros(0, 1),
               features_dc=torch.zeros(0, 1, 3), features_rest=torch.zeros(0, 15, 3), sh_degree=3)
    m = trainer.GaussianModel(raw, torch.device("cpu"))
    assert m.layout_version == 0
    n, kept = m.prune(min_opacity=0.1, max_scale=2.0)
    assert n == 0 and kept.dtype == torch.int64 and kept.numel() == 0 and m.layout_version == 0
    with pytest.raises(ValueError, match="min_opacity"):
        m.prune(min_opacity=2.0)


def _select_args(_l, **over):
    """A complete, valid gslic_prune_select argument list for P = 8 on dummy (never dereferenced) pointers; `over` replaces arguments by name."""
    names = ["P", "xyz", "dc", "opacity", "scaling", "rotation", "lo", "hi", "dnf", "drop", "protect", "tie", "split", "alloc", "ctx", "kept", "new_tie",
             "count", "below", "stream"]
    calls = []

    def _alloc(_ctx, n):
        calls.append(n)
        return None
    cb = _l.ALLOC_FN(_alloc)
    count, below = ctypes.c_int32(77), ctypes.c_int32(77)
    vals = dict(P=8, xyz=vp(0x10000), dc=vp(0x20000), opacity=vp(0x30000), scaling=vp(0x40000), rotation=vp(0x50000), lo=-1.0, hi=1.0, dnf=1, drop=None,
                protect=None, tie=None, split=4, alloc=cb, ctx=None, kept=vp(0x60000), new_tie=None, count=ctypes.byref(count), below=ctypes.byref(below),
                stream=None)
    for k, v in over.items():
        assert k in vals
        vals[k] = _l.ALLOC_FN() if (k == "alloc" and v is None) else v
    return [vals[n] for n in names], calls, count, below, cb


def test_prune_select_validates_before_any_device_work():
    _l, L = _libs()
    args, calls, count, below, _cb = _select_args(_l, P=0)
    assert L.gslic_prune_select(*args) == 0 and count.value == 0 and below.value == 0 and calls == []      # P == 0: at once, no allocator call
    args, calls, count, below, _cb = _select_args(_l, P=0, xyz=None, kept=None, alloc=None)
    assert L.gslic_prune_select(*args) == 0 and calls == []
    args, calls, _c, _b, _cb = _select_args(_l, P=-1)
    assert L.gslic_prune_select(*args) == -1 and b"negative P" in L.gslic_last_error() and calls == []
    for k in ("xyz", "dc", "opacity", "scaling", "rotation", "kept", "alloc"):
        args, calls, _c, _b, _cb = _select_args(_l, **{k: None})
        assert L.gslic_prune_select(*args) == -1 and b"NULL pointer" in L.gslic_last_error() and calls == [], k
    for k in ("count", "below"):
        args, calls, _c, _b, _cb = _select_args(_l, **{k: None})
        assert L.gslic_prune_select(*args) == -1 and b"NULL count" in L.gslic_last_error() and calls == [], k
    # an allocator that returns NULL is GSLIC_ERR_ALLOC, with the size it was asked for (flags + positions + scan temp, 256-B aligned)
    args, calls, _c, _b, _cb = _select_args(_l)
    assert L.gslic_prune_select(*args) == -3 and b"prune scratch allocator returned NULL" in L.gslic_last_error() and len(calls) == 1 and calls[0] >= 3 * 256


def _arrays(_l, rows):
    return (_l.RowArray * len(rows))(*[_l.RowArray(s, d, w) for s, d, w in rows]), len(rows)


def test_gather_rows_validates_and_rejects_overlap_before_any_device_work():
    _l, L = _libs()
    idx = vp(0x900000)
    ok, n = _arrays(_l, [(0x100000, 0x200000, 3), (0x300000, 0x400000, 45)])
    assert L.gslic_gather_rows(ok, n, idx, 0, None) == 0                       # n_rows == 0: at once
    assert L.gslic_gather_rows(None, 0, None, 100, None) == 0                  # no arrays: at once
    assert L.gslic_gather_rows(ok, n, idx, -1, None) == -1 and b"negative" in L.gslic_last_error()
    assert L.gslic_gather_rows(ok, -1, idx, 10, None) == -1 and b"negative" in L.gslic_last_error()
    assert L.gslic_gather_rows(None, 2, idx, 10, None) == -1 and b"NULL pointer" in L.gslic_last_error()
    assert L.gslic_gather_rows(ok, n, None, 10, None) == -1 and b"NULL pointer" in L.gslic_last_error()
    bad, n = _arrays(_l, [(0x100000, 0x200000, 3), (0x300000, None, 45)])
    assert L.gslic_gather_rows(bad, n, idx, 10, None) == -1 and b"array 1 has a NULL pointer" in L.gslic_last_error()
    bad, n = _arrays(_l, [(None, 0x200000, 1)])
    assert L.gslic_gather_rows(bad, n, idx, 10, None) == -1 and b"array 0 has a NULL pointer" in L.gslic_last_error()
    # arrays of width 0 are skipped whatever their pointers are: nothing is left to launch
    empty, n = _arrays(_l, [(None, None, 0), (0x100000, 0x100000, 0)])
    assert L.gslic_gather_rows(empty, n, idx, 10, None) == 0
    # overlap: in place, partial from either side, one array's dst on another's src, two dsts on each other; 10 rows of 3 dwords = 120 bytes
    for rows, what in (([(0x100000, 0x100000, 3)], b"dst of array 0 overlaps src of array 0"),
                       ([(0x100000, 0x100000 + 116, 3)], b"dst of array 0 overlaps src of array 0"),
                       ([(0x100000 + 116, 0x100000, 3)], b"dst of array 0 overlaps src of array 0"),
                       ([(0x100000, 0x200000, 3), (0x300000, 0x100000 + 60, 3)], b"dst of array 1 overlaps src of array 0"),
                       ([(0x100000, 0x200000, 3), (0x300000, 0x200000 + 119, 1)], b"dst of array 0 overlaps dst of array 1")):
        arr, n = _arrays(_l, rows)
        assert L.gslic_gather_rows(arr, n, idx, 10, None) == -1 and what in L.gslic_last_error(), (rows, L.gslic_last_error())
