"""The comparators of tests/gpu_helpers.py and the file writer of tests/fused_check_io.py on CPU tensors: a comparator that can no longer fail,
or a file the C++ side would not find, shows here and not only on a GPU machine."""
import os
import types

import numpy as np
import pytest
import torch

import fused_check_io as fio
import gpu_helpers as gh

NAMES = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")
WIDTHS = (3, 3, 6, 1, 3, 4)


def _flip(t, i=0):
    """One bit of element i flipped, in place (the lowest mantissa bit: a float comparison sees it too)."""
    t.view(-1).view(torch.int32)[i] ^= 1


def _rows(P, seed):
    g = torch.Generator().manual_seed(seed)
    return {n: torch.rand(P, w, generator=g) + 0.5 for n, w in zip(NAMES, WIDTHS)}


def _map(P=5, order=None, capacity=8):
    """A stand-in with what map_snapshot / same_map read of a GaussianModel: the rows of a fixed map, stored in `order` behind spare capacity."""
    idx = torch.arange(P) if order is None else order
    store = lambda d: {n: torch.cat([t[idx], torch.full((capacity - P, t.shape[1]), 7.0)]) for n, t in d.items()}
    m = types.SimpleNamespace(NAMES=NAMES, P=P, _buf=store(_rows(P, 1)), _m=store(_rows(P, 2)), _v=store(_rows(P, 3)),
                              _tie=None if order is None else idx.to(torch.int32))
    for n in NAMES:
        setattr(m, n, m._buf[n][:P])
    m.original_order = lambda: None if m._tie is None else torch.argsort(m._tie[:P].long())
    return m


def _trained(seed=1):
    """A stand-in with what model_state reads: parameters and an optimizer state per group."""
    m = types.SimpleNamespace(NAMES=NAMES, **_rows(4, seed))
    m.optimizer = types.SimpleNamespace(state=[dict(exp_avg=t, exp_avg_sq=u) for t, u in zip(_rows(4, seed + 1).values(), _rows(4, seed + 2).values())])
    return m


def test_bits_and_same_tensors():
    a = [torch.arange(4.0), torch.arange(3)]
    assert gh.same_tensors(a, [t.clone() for t in a])
    assert not gh.same_tensors(a, a[:1]) and not gh.same_tensors(a[:1], a) and not gh.same_tensors(a, a + a[:1])
    b = [t.clone() for t in a]
    _flip(b[0], 2)
    assert not gh.same_tensors(a, b)
    z = torch.zeros(2)
    assert torch.equal(z, -z) and not torch.equal(gh.bits(z), gh.bits(-z))        # bits() tells what a float comparison does not
    assert gh.bits(torch.ones(2, 3)[:, 1]).dtype == torch.int32                    # (a strided view is taken contiguous first)


def test_assert_same_state_rejects_one_bit_anywhere():
    a = gh.model_state(_trained())
    assert sorted(a) == sorted([n + s for n in NAMES for s in ("", ".m", ".v")])
    gh.assert_same_state(a, gh.model_state(_trained()))
    for key in ("opacity", "scaling.m", "rotation.v"):
        b = gh.model_state(_trained())
        _flip(b[key], 1)
        with pytest.raises(AssertionError, match=key):
            gh.assert_same_state(a, b)
    b = gh.model_state(_trained())
    del b["xyz.v"]
    with pytest.raises(AssertionError):
        gh.assert_same_state(a, b)
    fresh = _trained()
    fresh.optimizer.state[0] = None                                                 # a group the optimizer has not stepped yet: no moments listed
    assert "xyz" in gh.model_state(fresh) and "xyz.m" not in gh.model_state(fresh)


@pytest.mark.parametrize("view", [gh.bits, None])
def test_same_map_rejects_one_bit_in_a_parameter_or_a_moment(view):
    order = torch.tensor([3, 0, 4, 1, 2])
    gh.same_map(_map(), _map(order=order), view=view)
    for field in ("_buf", "_m", "_v"):
        b = _map(order=order)
        _flip(getattr(b, field)["scaling"], 4)
        with pytest.raises(AssertionError, match="scaling"):
            gh.same_map(_map(), b, view=view)
    b = _map(order=order)
    _flip(b._buf["xyz"], 3 * 5)                                                     # behind row P: not part of the map
    gh.same_map(_map(), b, view=view)
    gh.same_map(_map(), _map(order=torch.tensor([3, 0, 4, 2, 1])), view=view)      # another storage order of the same map
    b = _map(order=order)
    b._tie[1] ^= 4                                                                  # one bit of the tie rank: the rows are listed in another order
    with pytest.raises(AssertionError):
        gh.same_map(_map(), b, view=view)


def test_map_snapshot_copies_rows_moments_and_tie_rank():
    order = torch.tensor([3, 0, 4, 1, 2])
    m = _map(order=order)
    snap = gh.map_snapshot(m, tie=True)
    assert sorted(snap) == sorted([n + s for n in NAMES for s in ("", ".m", ".v")] + ["tie"])
    assert snap["tie"].dtype == torch.int64 and torch.equal(snap["tie"], order) and snap["xyz"].shape == (5, 3)
    assert "tie" not in gh.map_snapshot(m) and gh.map_snapshot(_map(), tie=True)["tie"] is None
    back = gh.map_snapshot(m, m.original_order())
    plain = gh.map_snapshot(_map())
    assert all(torch.equal(gh.bits(back[k]), gh.bits(plain[k])) for k in plain)
    for field, key in (("_buf", "opacity"), ("_m", "opacity.m"), ("_v", "opacity.v")):
        _flip(getattr(m, field)["opacity"], 2)
        now = gh.map_snapshot(m, tie=True)
        assert not torch.equal(gh.bits(now[key]), gh.bits(snap[key])) and torch.equal(now["xyz"], snap["xyz"])   # a copy, and of that array
    m._tie[1] ^= 1
    assert not torch.equal(gh.map_snapshot(m, tie=True)["tie"], snap["tie"])


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_guards_intact_sees_every_guard_word(dtype):
    n = 10
    buf, words = gh.guarded(n, dtype, 7, device="cpu")
    assert buf.numel() == n + 2 * gh.GUARD and words.data_ptr() == buf[gh.GUARD:].data_ptr() and bool((words == 7).all())
    assert gh.guards_intact(buf, n)
    words.fill_(-1)                                                                 # the words themselves are the caller's
    assert gh.guards_intact(buf, n)
    for i in (0, gh.GUARD - 1, gh.GUARD + n, buf.numel() - 1):
        hit = buf.clone()
        hit[i] = 0
        assert not gh.guards_intact(hit, n), i
    raw, _w = gh.guarded(n, device="cpu")
    assert bool((raw == gh.SENTINEL).all())                                         # no fill: the words start as guard words too
    nan_buf, _w = gh.guarded(n, device="cpu", sentinel=0x7FC0FFEE)
    assert gh.guards_intact(nan_buf, n, sentinel=0x7FC0FFEE) and not gh.guards_intact(nan_buf, n)


def _camera(k):
    f = lambda *shape: (np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape) + 100.0 * k)   # float64, as Camera holds them
    return types.SimpleNamespace(world_view_transform=f(4, 4), full_proj_transform=f(4, 4) + 0.5, camera_center=f(3) + 0.25, tanfovx=0.5 + k,
                                 tanfovy=0.25 + k, limx_neg=-1.5 - k, limx_pos=1.5 + k, limy_neg=-1.25 - k, limy_pos=1.25 + k)


def _raw(P, M):
    g = torch.Generator().manual_seed(P + M)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(xyz=r(P, 3), scaling=r(P, 3), rotation=r(P, 4), opacity=r(P, 1), features_dc=r(P, 1, 3), features_rest=r(P, M, 3), sh_degree=3 if M else 0)


def test_write_inputs_writes_what_the_header_reads(tmp_path):
    """The file list of gaussian-lic_amd/shim/fused_check_io.h: names, float32 bytes, the order of the scalars, the camera tag."""
    d = str(tmp_path)
    P, raw, cams = 7, _raw(7, 15), [_camera(0), _camera(1)]
    gt = torch.rand(3, 4, 5)
    tie = torch.randperm(P).to(torch.int32)
    fio.write_inputs(d, raw, cams, scalars_extra=(9.0, 10.5), gt=gt, tie_rank=tie, near=torch.rand(4, 5).double())
    f32 = lambda name: np.fromfile(os.path.join(d, name + ".f32"), np.float32)
    assert sorted(os.listdir(d)) == sorted(n + ".f32" for n in ("xyz", "scaling", "rotation", "opacity", "dc", "rest", "view", "proj", "campos",
                                                                "view2", "proj2", "campos2", "scalars", "gt", "tie_rank", "near"))
    for key, name in fio.GROUPS:
        assert f32(name).tobytes() == raw[key].numpy().tobytes(), name
    assert f32("rest").size == P * 15 * 3 and f32("dc").size == P * 3
    for tag, cam in (("", cams[0]), ("2", cams[1])):
        assert np.array_equal(f32("view" + tag), cam.world_view_transform.astype(np.float32).reshape(-1))
        assert np.array_equal(f32("proj" + tag), cam.full_proj_transform.astype(np.float32).reshape(-1))
        assert np.array_equal(f32("campos" + tag), cam.camera_center.astype(np.float32))
    assert f32("scalars").tolist() == [0.5, 0.25, -1.5, 1.5, -1.25, 1.25, 9.0, 10.5]        # the first camera's six, then the program's own
    assert f32("gt").tobytes() == gt.numpy().tobytes()
    assert np.array_equal(f32("tie_rank"), tie.numpy().astype(np.float32))                  # the indices as floats: probe_tie_rank converts back
    assert f32("near").size == 20                                                           # (float64 in, float32 on disk)
    fio.write(d, "exp_kept", np.array([3, 1, 2]), np.int32, "i32")
    assert np.fromfile(os.path.join(d, "exp_kept.i32"), np.int32).tolist() == [3, 1, 2]


def test_write_inputs_from_a_model_and_without_rest_at_degree_0(tmp_path):
    d = str(tmp_path)
    raw = _raw(5, 0)
    model = types.SimpleNamespace(**{k: (v.clone().requires_grad_(True) if torch.is_tensor(v) else v) for k, v in raw.items()})
    fio.write_inputs(d, model, _camera(0))                                                  # one camera, not in a list; parameters that require grad
    assert sorted(os.listdir(d)) == sorted(n + ".f32" for n in ("xyz", "scaling", "rotation", "opacity", "dc", "view", "proj", "campos", "scalars"))
    assert np.fromfile(os.path.join(d, "xyz.f32"), np.float32).tobytes() == raw["xyz"].numpy().tobytes()
    assert np.fromfile(os.path.join(d, "scalars.f32"), np.float32).size == 6


def test_read_and_read_rows_take_the_files_dump_rows_writes(tmp_path):
    d = str(tmp_path)
    g = torch.Generator().manual_seed(3)
    want = {}
    for M, tie in ((15, True), (0, False)):
        for f in os.listdir(d):
            os.remove(os.path.join(d, f))
        for n in fio.ROW_NAMES:
            if n == "rest" and M == 0:
                continue
            for pre in ("", "m_", "v_"):
                want[pre + n] = torch.randn(6, generator=g)
                want[pre + n].numpy().tofile(os.path.join(d, "out_" + pre + n + ".f32"))
        if tie:
            torch.arange(6, dtype=torch.int32).numpy().tofile(os.path.join(d, "out_tie.i32"))
        rows = fio.read_rows(d, M, tie=tie)
        assert len(rows) == (19 if tie else 15) and ("rest" in rows) == (M > 0) and ("tie" in rows) == tie
        assert all(t.dtype == torch.int32 and torch.equal(t, gh.bits(want[k])) for k, t in rows.items() if k != "tie")
    assert torch.equal(fio.read(d, "v_xyz.f32", np.float32), want["v_xyz"])
    with pytest.raises(FileNotFoundError):
        fio.read_rows(d, 15)
