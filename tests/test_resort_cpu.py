"""CPU-only: the re-sort surface that needs no device — the three exports are declared and bound (ABI still 8), the numpy float32 transcription
of the key rule (tests/resort_ref.py, the yardstick of the GPU tests) gives hand-computed keys, and gslic_morton_order / gslic_permute_rows /
gslic_permute_rows_staging_bytes reject bad arguments before any device work (no case here may reach a HIP call: without a GPU it would fail)."""
import ctypes
import os
import re

import numpy as np
import pytest

import resort_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = ctypes.c_void_p
NAN, INF = float("nan"), float("inf")


def _libs():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    return _lib, _lib.lib()


def test_header_declares_and_lib_binds_the_three_exports():
    _l, L = _libs()
    src = open(os.path.join(ROOT, "include", "gslic_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, ret in (("gslic_morton_order", "int"), ("gslic_permute_rows", "int"), ("gslic_permute_rows_staging_bytes", "size_t")):
        assert re.search(r"\b" + ret + r"\s+" + name + r"\s*\(", code), name
        assert name in _l.EXPORTS and hasattr(L, name)
    assert "#define GSLIC_ABI_VERSION 8" in src and L.gslic_abi_version() == 8     # additive: the ABI number stays
    assert len(L.gslic_morton_order.argtypes) == 8 and len(L.gslic_permute_rows.argtypes) == 7 and len(L.gslic_permute_rows_staging_bytes.argtypes) == 3
    names = [L.gslic_profile_kernel_name(i).decode() for i in range(L.gslic_profile_num_kernels())]
    assert names[-2:] == ["prune_select", "gather_rows"]                            # no profiler id of its own
    # the rule is stated in the header, step by step
    for line in ("d = (e > 1e-30f) ? e : 1e-30f", "t = (xyz[i,k] - lo_k) / d", "c = (t > 0) ? ((t < 1) ? t : 1) : 0", "u_k = (uint32) trunc(c * 1023.0f)",
                 "key[i] = spread(u_0) | spread(u_1) << 1 | spread(u_2) << 2"):
        assert line in src, line


def test_key_rule_reference_gives_hand_computed_keys():
    S511, S1023 = 0x01249249, 0x09249249          # spread(0b0111111111), spread(0b1111111111): every third bit
    assert int(ref.spread10(np.array([511], np.uint32))[0]) == S511 and int(ref.spread10(np.array([1023], np.uint32))[0]) == S1023
    box = np.array([0, 0, 0, 1, 2, 4], np.float32)
    cases = [
        ((0, 0, 0), 0),                                           # the low corner
        ((1, 2, 4), 0x3FFFFFFF),                                  # the high corner: 1023 on every axis, all 30 bits
        ((0.5, 1, 2), 0x07FFFFFF),                                # the centre: 0.5 * 1023 = 511.5 -> 511 on every axis
        ((0.25, 0, 0), 0x00249249),                               # 255.75 -> 255 = 0xFF on x
        ((-5, 1, 2), (S511 << 1) | (S511 << 2)),                  # an outlier below: clamped to cell 0 on x
        ((7, 1, 2), S1023 | (S511 << 1) | (S511 << 2)),           # an outlier above: clamped to cell 1023 on x
        ((0.5, -3, 9), S511 | (S1023 << 2)),                      # ... on the two other axes
        ((NAN, 0, 0), 0), ((0, NAN, 4), S1023 << 2),              # NaN reads as 0 on its axis only
        ((INF, 0, 0), S1023), ((-INF, 0, 0), 0), ((0, INF, -INF), S1023 << 1),
    ]
    xyz = np.array([c[0] for c in cases], np.float32)
    assert [int(k) for k in ref.morton_keys(xyz, box)] == [c[1] for c in cases]
    # one third: (float) 1/3 = 0.33333334, * 1023 rounds to 341.00003 -> 341 = 0b0101010101
    assert int(ref.morton_keys(np.array([[1, 0, 0]], np.float32), np.array([0, 0, 0, 3, 1, 1], np.float32))[0]) == 0x01041041
    # a degenerate axis (hi == lo): d = 1e-30f, rows at or below lo on cell 0, rows above it on cell 1023
    flat = np.array([0, 0, 3, 1, 2, 3], np.float32)
    z = np.array([[0, 0, 3], [0, 0, 3.5], [0, 0, 2], [0, 0, NAN]], np.float32)
    assert [int(k) for k in ref.morton_keys(z, flat)] == [0, S1023 << 2, 0, 0]
    # inf - inf in the box (axis 0: a NaN extent reads as 1e-30f), an infinite extent with an infinite lo (axis 1: x - lo is +inf or NaN, over inf: NaN -> 0) and
    # inf - inf in the numerator (NaN reads as 0)
    wild = np.array([INF, -INF, 0, INF, INF, 1], np.float32)
    assert [int(k) for k in ref.morton_keys(np.array([[1, 1, 1], [INF, INF, 0], [-INF, -INF, 0.5]], np.float32), wild)] == [S1023 << 2, 0, S511 << 2]
    # the permutation: ascending keys, equal keys in storage order
    pts = np.array([[1, 2, 4], [0, 0, 0], [0.5, 1, 2], [0, 0, 0], [1, 2, 4], [-1, -1, -1]], np.float32)
    perm, ks = ref.morton_perm(pts, box)
    assert perm.tolist() == [1, 3, 5, 2, 0, 4] and ks.tolist() == [0, 0, 0, 0x07FFFFFF, 0x3FFFFFFF, 0x3FFFFFFF] and perm.dtype == np.uint32


def _order_args(_l, **over):
    """A complete, valid gslic_morton_order argument list for P = 8 on dummy (never dereferenced) pointers; `over` replaces arguments by name."""
    names = ["P", "xyz", "box", "alloc", "ctx", "perm", "keys", "stream"]
    calls = []

    def _alloc(_ctx, n):
        calls.append(n)
        return None
    cb = _l.ALLOC_FN(_alloc)
    vals = dict(P=8, xyz=vp(0x10000), box=vp(0x20000), alloc=cb, ctx=None, perm=vp(0x30000), keys=None, stream=None)
    for k, v in over.items():
        assert k in vals
        vals[k] = _l.ALLOC_FN() if (k == "alloc" and v is None) else v
    return [vals[n] for n in names], calls, cb


def test_morton_order_validates_before_any_device_work():
    _l, L = _libs()
    args, calls, _cb = _order_args(_l, P=0)
    assert L.gslic_morton_order(*args) == 0 and calls == []                    # P == 0: at once, no allocator call
    args, calls, _cb = _order_args(_l, P=0, xyz=None, box=None, perm=None, alloc=None)
    assert L.gslic_morton_order(*args) == 0 and calls == []
    args, calls, _cb = _order_args(_l, P=-1)
    assert L.gslic_morton_order(*args) == -1 and b"negative P" in L.gslic_last_error() and calls == []
    for k in ("xyz", "box", "perm", "alloc"):
        args, calls, _cb = _order_args(_l, **{k: None})
        assert L.gslic_morton_order(*args) == -1 and b"NULL pointer" in L.gslic_last_error() and calls == [], k
    # an allocator that returns NULL is GSLIC_ERR_ALLOC, after ONE call for the three u32 arrays and the sort's scratch
    args, calls, _cb = _order_args(_l)
    assert L.gslic_morton_order(*args) == -3 and b"morton order scratch allocator returned NULL" in L.gslic_last_error()
    assert len(calls) == 1 and calls[0] >= 3 * 256
    args, calls, _cb = _order_args(_l, keys=vp(0x40000))                       # keys_sorted given: the same single request
    assert L.gslic_morton_order(*args) == -3 and len(calls) == 1


def _arrays(_l, rows):
    return (_l.RowArray * len(rows))(*[_l.RowArray(p, p if q is None else q, w) for p, q, w in rows]), len(rows)


def test_permute_rows_validates_and_rejects_overlap_before_any_device_work():
    _l, L = _libs()
    perm, stage = vp(0x900000), vp(0x4000000)
    ok, n = _arrays(_l, [(0x100000, None, 3), (0x300000, None, 45)])         # 10 rows: 120 + 1800 = 1920 bytes of staging
    assert L.gslic_permute_rows_staging_bytes(ok, n, 10) == L.gslic_scratch_round_up(1920) >= 1920
    assert L.gslic_permute_rows_staging_bytes(ok, n, 0) == 0 and L.gslic_permute_rows_staging_bytes(None, 0, 10) == 0
    assert L.gslic_permute_rows_staging_bytes(ok, -1, 10) == 0 and L.gslic_permute_rows_staging_bytes(ok, n, -1) == 0
    big = 2000000 * 4 * (45 + 3)
    assert L.gslic_permute_rows_staging_bytes(ok, n, 2000000) == L.gslic_scratch_round_up(big) >= big        # no 32-bit overflow
    assert L.gslic_permute_rows(ok, n, perm, 0, None, 0, None) == 0               # n_rows == 0: at once
    assert L.gslic_permute_rows(None, 0, None, 100, None, 0, None) == 0           # no arrays: at once
    assert L.gslic_permute_rows(ok, n, perm, -1, stage, 1 << 20, None) == -1 and b"negative" in L.gslic_last_error()
    assert L.gslic_permute_rows(ok, -1, perm, 10, stage, 1 << 20, None) == -1 and b"negative" in L.gslic_last_error()
    assert L.gslic_permute_rows(None, 2, perm, 10, stage, 1 << 20, None) == -1 and b"NULL pointer" in L.gslic_last_error()
    assert L.gslic_permute_rows(ok, n, None, 10, stage, 1 << 20, None) == -1 and b"NULL pointer" in L.gslic_last_error()
    assert L.gslic_permute_rows(ok, n, perm, 10, None, 1 << 20, None) == -1 and b"NULL pointer" in L.gslic_last_error()
    # too small by one byte; exactly enough passes the checks (and would launch: not tried here)
    assert L.gslic_permute_rows(ok, n, perm, 10, stage, 1919, None) == -1 and b"staging holds 1919 bytes, 1920 are needed" in L.gslic_last_error()
    assert L.gslic_permute_rows(ok, n, perm, 10, stage, 0, None) == -1 and b"1920 are needed" in L.gslic_last_error()
    bad, n1 = _arrays(_l, [(0x100000, None, 3), (None, None, 45)])
    bad[1].src, bad[1].dst = None, None
    assert L.gslic_permute_rows(bad, n1, perm, 10, stage, 1 << 20, None) == -1 and b"array 1 has a NULL pointer" in L.gslic_last_error()
    bad, n1 = _arrays(_l, [(0x100000, 0x200000, 3)])
    assert L.gslic_permute_rows(bad, n1, perm, 10, stage, 1 << 20, None) == -1 and b"array 0 has src != dst" in L.gslic_last_error()
    # arrays of width 0 are skipped whatever their pointers are: nothing is left to move
    empty, n0 = _arrays(_l, [(0x100000, None, 0), (0x200000, 0x300000, 0)])
    empty[0].src, empty[0].dst = None, None
    assert L.gslic_permute_rows(empty, n0, perm, 10, None, 0, None) == 0
    # overlap: the staging buffer as declared against the first 10 rows of an array (from either side), and two arrays on each other
    for rows, st, nb, what in (([(0x100000, None, 3), (0x300000, None, 45)], 0x300000 + 1799, 1920, b"staging overlaps array 1"),
                               ([(0x100000, None, 3), (0x300000, None, 45)], 0x100000 - 1919, 1920, b"staging overlaps array 0"),
                               ([(0x100000, None, 3), (0x300000, None, 45)], 0x200000, 0x100001, b"staging overlaps array 1"),
                               ([(0x100000, None, 3), (0x100000 + 119, None, 1)], 0x4000000, 1 << 20, b"array 1 overlaps array 0"),
                               ([(0x100000 + 39, None, 1), (0x100000, None, 3)], 0x4000000, 1 << 20, b"array 1 overlaps array 0")):
        arr, k = _arrays(_l, rows)
        assert L.gslic_permute_rows(arr, k, perm, 10, vp(st), nb, None) == -1 and what in L.gslic_last_error(), (rows, L.gslic_last_error())


def test_resort_of_an_insertion_order_model_stays_an_error():
    import torch
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    raw = dict(xyz=torch.zeros(4, 3), scaling=torch.zeros(4, 3), rotation=torch.zeros(4, 4), opacity=torch.zeros(4, 1),
               features_dc=torch.zeros(4, 1, 3), features_rest=torch.zeros(4, 15, 3), sh_degree=3)
    m = trainer.GaussianModel(raw, torch.device("cpu"))
    with pytest.raises(AssertionError, match="insertion order"):
        m.resort()
    assert callable(trainer.morton_box) and hasattr(trainer.GaussianModel, "to_morton_order")
    box = trainer.morton_box(torch.tensor([[0., 1., 2.], [3., 4., 5.]]))
    assert box.dtype == torch.float32 and box.tolist() == [0., 1., 2., 3., 4., 5.]
