"""No GPU: the three gradient-statistics exports are declared, bound and refuse bad arguments before any device work; the mask rules against numpy
on hand-made arrays; the attach / detach protocol of trainer.GradientStats on a CPU model; and what rasterizer.py hands the library with and
without grad_stats (a recorder stands in for the library)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gradstats_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gslic_rasterize_backward_adam_stats", "gslic_rasterize_backward_depth_adam_stats", "gslic_gradient_stats_accumulate")


def _libs():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    return _lib, _lib.lib()


def _prm(_lib, P=8, M=3, D=1, raw=1):
    return _lib.RasterParams(P, D, M, 40, 24, 1.0, 1.0, -1.0, 1.0, -1.0, 1.0, 1.0, 0, 0, 0, raw, None)


def _adam(_lib, base=0x100000):
    a = _lib.AdamFused()
    for g in range(6):
        a.param[g], a.exp_avg[g], a.exp_avg_sq[g] = base + 0x10000 * (3 * g), base + 0x10000 * (3 * g + 1), base + 0x10000 * (3 * g + 2)
        a.lr[g] = 1e-3
    a.b1, a.b2, a.eps = 0.9, 0.999, 1e-15
    return a


def test_exports_are_declared_bound_and_abi_stays():
    _lib, L = _libs()
    header = open(os.path.join(ROOT, "include", "gslic_hip.h")).read()
    assert L.gslic_abi_version() == 8 and "#define GSLIC_ABI_VERSION 8" in header.replace("  ", " ")
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name)
        decl = re.search(r"int %s\((.*?)\);" % name, header, re.S)
        assert decl is not None, name
        args = [a for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",") if a.strip()]
        assert len(args) == len(getattr(L, name).argtypes), name
    assert len(L.gslic_rasterize_backward_adam_stats.argtypes) == len(L.gslic_rasterize_backward_adam.argtypes) + 1
    assert len(L.gslic_rasterize_backward_depth_adam_stats.argtypes) == len(L.gslic_rasterize_backward_depth_adam.argtypes) + 1
    assert [f[0] for f in _lib.GradStats._fields_] == ["grad_sum", "n_seen", "max_radius"] and ctypes.sizeof(_lib.GradStats) == 24
    assert re.search(r"typedef struct gslic_grad_stats \{\s*float\* grad_sum;.*?uint32_t\* n_seen;.*?int32_t\* max_radius;", header, re.S)


def _bad_stats(_lib, P=8):
    """(label, GradStats or None, word the message must hold): every refused statistics descriptor for P rows of 4 bytes."""
    a, b, c = 0x10000, 0x20000, 0x30000
    yield "stats NULL", None, "NULL"
    for hole in range(3):
        v = [a, b, c]
        v[hole] = None
        yield f"array {hole} NULL", _lib.GradStats(*v), "NULL"
    yield "sum == seen", _lib.GradStats(a, a, c), "overlap"
    yield "seen inside radius", _lib.GradStats(a, c + 4 * P - 4, c), "overlap"
    yield "sum one word into radius", _lib.GradStats(c - 4 * P + 4, b, c), "overlap"


@pytest.mark.parametrize("depth", [False, True])
def test_fused_entry_points_refuse_bad_arguments_before_any_device_work(depth):
    """Every call passes host addresses as device buffers: an implementation that launched anything would fault."""
    _lib, L = _libs()
    fn = L.gslic_rasterize_backward_depth_adam_stats if depth else L.gslic_rasterize_backward_adam_stats
    junk = ctypes.c_void_p(0x1000)
    prm, adam = _prm(_lib), _adam(_lib)
    good = _lib.GradStats(0x10000, 0x20000, 0x30000)

    def call(prm_, adam_, st):
        head = [ctypes.byref(prm_) if prm_ is not None else None, 1, 1] + [junk] * 16 + [junk] * (2 if depth else 1)
        tail = [None, junk, None, None, None, None, 0.0, ctypes.byref(adam_) if adam_ is not None else None, ctypes.byref(st) if st is not None else None, None]
        rc = fn(*head, *tail)
        return rc, L.gslic_last_error().decode()

    for label, st, word in _bad_stats(_lib):
        rc, msg = call(prm, adam, st)
        assert rc == -1 and word in msg, (label, rc, msg)
    # ... one word of grad_sum inside an Adam tensor (group 4's exp_avg_sq: [P,3] floats), and just behind it
    t = adam.exp_avg_sq[4]
    rc, msg = call(prm, adam, _lib.GradStats(t + 4 * 3 * 8 - 4, 0x20000, 0x30000))
    assert rc == -1 and "overlaps an Adam tensor of group 4" in msg
    rc, msg = call(prm, adam, _lib.GradStats(0x10000, 0x20000, adam.param[0] - 4 * 8 + 4))
    assert rc == -1 and "overlaps an Adam tensor of group 0" in msg
    rc, msg = call(prm, None, good)
    assert rc == -1 and "adam descriptor is NULL" in msg
    rc, msg = call(None, adam, good)
    assert rc == -1 and "params is NULL" in msg
    rc, msg = call(_prm(_lib, P=-1), adam, good)
    assert rc == -1 and "P=-1" in msg
    # behind the statistics' own checks the shared ones still answer before anything runs (here: colors_precomp is not supported)
    rc, msg = call(prm, adam, good)
    assert rc == -2 and "colors_precomp" in msg


def test_stand_alone_export_refuses_bad_arguments_before_any_device_work():
    _lib, L = _libs()
    fn = L.gslic_gradient_stats_accumulate
    junk = ctypes.c_void_p(0x1000)
    good = _lib.GradStats(0x10000, 0x20000, 0x30000)

    def call(P, dL, radii, st, r0, r1):
        rc = fn(P, dL, radii, ctypes.byref(st) if st is not None else None, r0, r1, None)
        return rc, L.gslic_last_error().decode()

    for label, st, word in _bad_stats(_lib):
        rc, msg = call(8, junk, junk, st, 0, -1)
        assert rc == -1 and word in msg, (label, rc, msg)
    for r0, r1 in ((-1, 4), (5, 4), (0, 9), (9, -1)):
        rc, msg = call(8, junk, junk, good, r0, r1)
        assert rc == -1 and "row range" in msg, (r0, r1, msg)
    rc, msg = call(-3, junk, junk, good, 0, -1)
    assert rc == -1 and "P=-3" in msg
    rc, msg = call(8, None, junk, good, 0, -1)
    assert rc == -1 and "NULL" in msg
    rc, msg = call(8, junk, None, good, 0, 8)
    assert rc == -1 and "NULL" in msg
    assert fn(0, None, None, ctypes.byref(good), 0, -1, None) == 0       # nothing to do
    assert fn(8, junk, junk, ctypes.byref(good), 4, 4, None) == 0        # an empty range


def test_mask_rules_on_hand_made_arrays():
    from gaussian_lic_amd import trainer
    thr = 0.3
    t32 = np.float32(thr)
    three = np.float32(t32 * np.float32(3.0))                      # equality at the threshold for n_seen = 3
    below = np.nextafter(three, np.float32(0))
    #                 unseen  unseen+sum  at the bar  just below  above   NaN       one view at bar  inf      huge count
    gsum = np.array([0.0,     9.0,        three,      below,      2.0,    np.nan,   t32,             np.inf,  4.0e9], np.float32)
    seen = np.array([0,       0,          3,          3,          3,      3,        1,               2,       0xffffffff], np.uint32)
    want = gr.grow_mask(gsum, seen, thr)
    assert want.tolist() == [0, 0, 1, 0, 1, 0, 1, 1, 1]            # >= is kept; unseen rows and NaN sums never grow
    tg, ts = torch.from_numpy(gsum), torch.from_numpy(seen.astype(np.int64))
    got = trainer.gradient_grow_mask(tg, ts, thr)
    assert got.dtype == torch.uint8 and got.tolist() == want.tolist()
    for min_seen, expect in ((0, want.tolist()), (2, [0, 0, 1, 0, 1, 0, 0, 1, 1]), (4, [0, 0, 0, 0, 0, 0, 0, 0, 1])):
        assert trainer.gradient_grow_mask(tg, ts, thr, min_seen).tolist() == expect == gr.grow_mask(gsum, seen, thr, min_seen).tolist()
    assert trainer.gradient_grow_mask(tg, ts, float("nan")).tolist() == [0] * 9 == gr.grow_mask(gsum, seen, float("nan")).tolist()
    rad = np.array([0, 19, 20, 21, -5, 2 ** 31 - 1], np.int32)
    assert gr.big_mask(rad, 20).tolist() == [0, 0, 0, 1, 0, 1]     # strict


def test_rule_transcription_on_hand_made_rows():
    """A check of the yardstick, not of the feature (it passes without it): tests/gradstats_ref.py's transcription on rows worked out by hand."""
    gs, ns, mr = gr.sentinels(6)
    g = np.zeros((6, 3), np.float32)
    g[:, 0] = [3.0, 1e-30, np.inf, np.nan, 0.5, 2.0]
    g[:, 1] = [4.0, 0.0, 1.0, 1.0, 0.0, 2.0]
    g[:, 2] = 99.0                                                  # never read
    radii = np.array([9, 3, 12, 2, 0, -1], np.int32)
    gr.apply_rule(gs, ns, mr, g, radii)
    s, c, r = float(gr.SENT_SUM), int(gr.SENT_SEEN), int(gr.SENT_RADIUS)
    assert gs.tolist() == [s + 5.0, float(np.float32(s) + np.float32(1e-30)), s, s, s, s]
    assert ns.tolist() == [c + 1, c + 1, c, c, c, c] and mr.tolist() == [9, r, 12, r, r, r]
    gr.apply_rule(gs, ns, mr, g, radii, rows=(1, 3))
    assert ns.tolist() == [c + 1, c + 2, c, c, c, c]


def test_stats_object_on_a_cpu_model_tracks_the_rows():
    """The bookkeeping of GradientStats without a kernel: sizes, zero fill, accessors, masks, and the stale-rows error of a detached object."""
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    m = trainer.GaussianModel(gr.scene(96, 3), torch.device("cpu"), capacity=200)
    st = trainer.GradientStats(m)
    cs = trainer.ContributionStats(m)
    assert [a.shape for a, _w in st._arrays()] == [(200,)] * 3 and [w for _a, w in st._arrays()] == [1, 1, 1]
    assert [a.dtype for a, _w in st._arrays()] == [torch.float32, torch.int32, torch.int32] and not any(bool(a.any()) for a, _w in st._arrays())
    assert m._attached_stats() == [st, cs]
    st._sum[:4] = torch.tensor([0.9, 0.5, 0.0, 7.0])
    st._seen_n[:4] = torch.tensor([3, -1, 0, 2], dtype=torch.int32)          # -1: the bit pattern of 2^32 - 1
    st._maxr[:4] = torch.tensor([5, 21, 0, 20], dtype=torch.int32)
    assert st.grad_sum().shape == (96,) and st.n_seen()[:4].tolist() == [3, (1 << 32) - 1, 0, 2] and st.max_radius().dtype == torch.int32
    mg = st.mean_gradient()
    assert mg.dtype == torch.float32 and mg[:4].tolist() == [float(np.float32(0.9) / np.float32(3)), float(np.float32(0.5) / np.float32(2 ** 32 - 1)), 0.0, 3.5]
    assert st.grow_mask(0.3)[:4].tolist() == gr.grow_mask(st._sum[:4].numpy(), st._seen_n[:4].numpy().view(np.uint32), 0.3).tolist() == [0, 0, 0, 1]   # (float32(0.3) * 3 rounds above float32(0.9))
    assert st.big_mask(20)[:4].tolist() == [0, 1, 0, 0]
    # the model walks the protocol: a permutation by torch indexing, zeros for rows, then the stale-rows error once detached
    perm = torch.arange(95, -1, -1)
    st._permute(perm)
    assert st.grad_sum()[-4:].flip(0).tolist() == [float(np.float32(v)) for v in (0.9, 0.5, 0.0, 7.0)]
    st._zero_rows(torch.tensor([95]))
    assert st.grad_sum()[95] == 0 and st.n_seen()[95] == 0 and st.max_radius()[95] == 0 and st.max_radius()[94] == 21
    st.reset()
    assert not any(bool(a.any()) for a, _w in st._arrays())
    st.detach()
    assert m._attached_stats() == [cs]
    m._rows_version += 1                                                       # what prune() / extend() / resort() do
    with pytest.raises(RuntimeError, match="GradientStats: the model's rows changed"):
        st.grad_sum()
    with pytest.raises(RuntimeError, match="ContributionStats: the model's rows changed"):
        cs._check()
    with pytest.raises(RuntimeError, match="rows changed"):
        trainer._grad_stats_for_step(st, m)
    with pytest.raises(ValueError, match="GradientStats of the model"):
        trainer._grad_stats_for_step(trainer.GradientStats(trainer.GaussianModel(gr.scene(8, 3), torch.device("cpu"))), m)
    assert trainer._grad_stats_for_step(None, m) is None


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, sym):
        def fn(*args):
            self.calls.append((sym, args))
            return 0
        return fn


def test_without_grad_stats_the_library_sees_the_old_calls(monkeypatch):
    _lib, _L = _libs()
    from gaussian_lic_amd import rasterizer as rz
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "current_stream_ptr", lambda: ctypes.c_void_p(0x5eadbeef))
    P, M, H, W = 8, 3, 16, 32
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)
    bg, xyz, dc, sh, sc, rot = z(3), z(P, 3), z(P, 1, 3), z(P, M, 3), z(P, 3), z(P, 4)
    view, proj, campos, radii = z(4, 4), z(4, 4), z(3), z(P, dt=torch.int32)
    geom, binning, img, sample = (z(64, dt=torch.uint8) for _ in range(4))
    dL, dLd, e = z(3, H, W), z(H, W), torch.empty(0)
    adam = _adam(_lib)
    arrays = z(P), z(P, dt=torch.int32), z(P, dt=torch.int32)
    gs = rz.grad_stats_descriptor(*arrays, P)
    assert (gs.grad_sum, gs.n_seen, gs.max_radius) == tuple(a.data_ptr() for a in arrays)

    def run(depth, **kw):
        rec.calls.clear()
        if depth:
            rz.rasterize_gaussians_backward_depth(bg, xyz, radii, sc, rot, 1.0, view, proj, 1.0, 1.0, -1.0, 1.0, -1.0, 1.0, dL, dLd, dc, sh, 1, campos, geom, 11,
                                                  binning, img, 5, sample, 0.0, False, raw_params=True, **kw)
        else:
            rz.rasterize_gaussians_backward(bg, xyz, radii, e, sc, rot, 1.0, e, view, proj, 1.0, 1.0, -1.0, 1.0, -1.0, 1.0, dL, dc, sh, 1, campos, geom, 11,
                                            binning, img, 5, sample, 0.0, False, raw_params=True, **kw)
        assert len(rec.calls) == 1
        return rec.calls[0]

    val = lambda a: a.value if isinstance(a, ctypes.c_void_p) else (None if a is None else (a if isinstance(a, (int, float)) else "ref"))
    for depth, old, new in ((False, "gslic_rasterize_backward_adam", "gslic_rasterize_backward_adam_stats"),
                            (True, "gslic_rasterize_backward_depth_adam", "gslic_rasterize_backward_depth_adam_stats")):
        xg = dict(xyz_grad=z(P, 3)) if depth else {}
        sym0, args0 = run(depth, adam=adam, **xg)
        sym1, args1 = run(depth, adam=adam, grad_stats=None, **xg)
        sym2, args2 = run(depth, adam=adam, grad_stats=gs, **xg)
        assert sym0 == sym1 == old and sym2 == new
        assert len(args0) == len(args1) == (30 if depth else 29) and len(args2) == len(args0) + 1
        assert [val(a) for a in args0] == [val(a) for a in args1]
        assert [val(a) for a in args2[:-2]] == [val(a) for a in args0[:-1]] and val(args2[-1]) == val(args0[-1]) == 0x5eadbeef
        assert args2[-2]._obj is gs
    # the ten-gradient backward with caller storage: dL_dmeans2D stays unmaterialised unless mean2d_out asks for it
    out = dict(xyz=z(P, 3), features_dc=z(P, 1, 3), features_rest=z(P, M, 3), opacity=z(P, 1), scaling=z(P, 3), rotation=z(P, 4))
    m2 = z(P, 3)
    _s, a_plain = run(False, out=out)
    _s, a_m2 = run(False, out=out, mean2d_out=m2)
    assert _s == "gslic_rasterize_backward" and a_plain[20] is None and a_m2[20].value == m2.data_ptr()
    assert [val(a) for a in a_plain[:20]] == [val(a) for a in a_m2[:20]] and [val(a) for a in a_plain[21:]] == [val(a) for a in a_m2[21:]]
    with pytest.raises(ValueError, match="grad_stats goes with adam"):
        run(False, out=out, grad_stats=gs)
    # the stand-alone export
    rec.calls.clear()
    rz.gradient_stats_accumulate(m2, radii, *arrays, rows=(0, 8))
    sym, a = rec.calls[0]
    assert sym == "gslic_gradient_stats_accumulate" and a[0] == P and a[1].value == m2.data_ptr() and a[2].value == radii.data_ptr() and a[4:6] == (0, 8)
    with pytest.raises(ValueError, match="accumulator"):
        rz.gradient_stats_accumulate(m2, radii, arrays[0], arrays[1].long(), arrays[2])
