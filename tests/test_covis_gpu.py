"""-m gpu: covisibility sets — the record kernel and the three queries (gslic_covis_*) against the numpy restatement of their rule
(tests/covis_ref.py), the recorded column of GraphedStep(keyframes=, covis=) against independent forwards, the carriage through prune / densify /
extend / resort against plain torch indexing, and the C++ host against the Python host.  Everything is an integer: every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

import covis_ref as ref
import fused_check_io as fio
import gradstats_ref as gr
import keyframe_ref as kref
from gpu_helpers import assert_same_state, gpu, guarded, guards_intact, model_state, raw_forward

pytestmark = pytest.mark.gpu

P_REC = 1000 + 37          # not a multiple of 64 or 256: the last workgroup of the record kernel is partial
P_BIG = 70_001             # 274 workgroups of the queries flush their counters


def _mods():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib, trainer
    return trainer, _lib


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu())


def _word(f):
    return torch.full((1,), int(f), dtype=torch.int32, device=gpu())


def _frames_of(F):
    return sorted({0, min(31, F - 1), min(32, F - 1), F - 1})


class _Rows:
    """What Covisibility needs of a model, for driving the object on rows of any count without a map."""

    def __init__(self, P):
        self.P, self.capacity, self.device = P, P, gpu()
        self.layout_version = self._rows_version = 0
        self._stats = []


def _object(P, F, B=None):
    trainer, _lib = _mods()
    cv = trainer.Covisibility(_Rows(P), F)
    if B is not None:
        cv._bits.copy_(_dev(ref.pack(B).view(np.int32)))
    return cv


def _record_raw(P, F, bits, radii=None, visible=None, word=None, skip=None, rows=(0, -1)):
    _trainer, _lib = _mods()
    _lib.check(_lib.lib().gslic_covis_record(P, F, _lib.ptr(bits), _lib.ptr(radii), _lib.ptr(visible), _lib.ptr(word), _lib.ptr(skip), rows[0], rows[1],
                                             _lib.current_stream_ptr()))


# ---------------------------------------------------------------------------------------------------- record
@pytest.mark.parametrize("F", ref.FRAME_COUNTS)
def test_record_is_the_rule_on_guarded_rows(F):
    """Every frame of the list on rows that start from a random pattern: the column is replaced (all rows, none, a random mask; again; cleared),
    every other bit of the row — the neighbouring words at Wd > 1 included — stays, and so do the guard words around the array."""
    P, Wd = P_REC, ref.words(F)
    rng = np.random.default_rng(100 + F)
    B = ref.random_matrix(P, F, 0.5, F)
    buf, words = guarded(P * Wd)
    words.copy_(_dev(ref.pack(B).view(np.int32)).reshape(-1))
    radii_sets = [np.ones(P, np.int32), np.zeros(P, np.int32), rng.integers(-3, 4, P).astype(np.int32), rng.integers(-3, 4, P).astype(np.int32)]
    for f in _frames_of(F):
        for radii in radii_sets + [None]:                                    # (the last: both inputs NULL clears the column)
            _record_raw(P, F, words, radii=None if radii is None else _dev(radii), word=_word(f))
            ref.record(B, f, radii)
            got = words.cpu().numpy().view(np.uint32).reshape(P, Wd)
            assert np.array_equal(got, ref.pack(B)), (f, "the column, or a bit outside it")
        _record_raw(P, F, words, radii=_dev(radii_sets[2]), word=_word(f))    # leave a mixed column behind for the next frame's check
        ref.record(B, f, radii_sets[2])
    assert np.array_equal(words.cpu().numpy().view(np.uint32).reshape(P, Wd), ref.pack(B)) and guards_intact(buf, P * Wd)
    assert B.any() and not B.all()


@pytest.mark.parametrize("F", [33, 128])
def test_record_respects_range_skip_and_frame_word(F):
    P, Wd = P_REC, ref.words(F)
    B = ref.random_matrix(P, F, 0.5, 3 * F)
    buf, words = guarded(P * Wd)
    words.copy_(_dev(ref.pack(B).view(np.int32)).reshape(-1))
    radii = _dev(np.random.default_rng(F).integers(-2, 3, P).astype(np.int32))
    start = words.clone()
    one, zero = _word(1), _word(0)
    _record_raw(P, F, words, radii=radii, word=_word(32), skip=one)          # a step that did not fit
    for bad in (-1, F, F + 31, 1 << 20):                                     # a frame word out of range
        _record_raw(P, F, words, radii=radii, word=_word(bad))
        _record_raw(P, F, words, word=_word(bad))
    assert torch.equal(words, start)
    for rows in ((0, 1), (255, 257), (P - 1, P), (300, 900), (0, -1)):       # only the rows of the range; skip = 0 records
        _record_raw(P, F, words, radii=radii, word=_word(32), skip=zero, rows=rows)
        ref.record(B, 32, radii.cpu().numpy(), rows=(rows[0], P if rows[1] < 0 else rows[1]))
        assert np.array_equal(words.cpu().numpy().view(np.uint32).reshape(P, Wd), ref.pack(B)), rows
    assert guards_intact(buf, P * Wd)


@pytest.mark.parametrize("F", [1, 40, 1024])
def test_object_record_takes_ints_words_radii_and_masks_alike(F):
    """Covisibility.record: a host int and a device word name the same column; radii, a bool mask and a uint8 mask give the same bits; clear."""
    P = P_REC
    radii = _dev(np.random.default_rng(9).integers(-2, 3, P).astype(np.int32))
    vis = radii > 0
    f = F - 1
    outs = []
    for frame, seen in ((f, radii), (_word(f), radii), (f, vis), (_word(f), vis.to(torch.uint8))):
        cv = _object(P, F, ref.random_matrix(P, F, 0.5, 5))
        cv.record(frame, seen)
        outs.append(cv.bits().clone())
    want = ref.random_matrix(P, F, 0.5, 5)
    ref.record(want, f, radii.cpu().numpy())
    assert all(torch.equal(o, outs[0]) for o in outs) and np.array_equal(outs[0].cpu().numpy().view(np.uint32), ref.pack(want))
    assert torch.equal(cv.rows_of(f), vis)
    cv.clear(f)
    ref.record(want, f, None)
    assert np.array_equal(cv.bits().cpu().numpy().view(np.uint32), ref.pack(want)) and not bool(cv.rows_of(f).any())


# ---------------------------------------------------------------------------------------------------- the queries
def _designed(P, F):
    """Row r is seen by frame f when f divides r + 1 (f >= 1) — frame 0 sees every third row: a matrix whose counts have a closed form."""
    r = np.arange(P)[:, None] + 1
    f = np.arange(F)[None, :]
    B = (r % np.maximum(f, 1)) == 0
    B[:, 0] = (r[:, 0] % 3) == 0
    return B


def _check_queries(B, F, pairs):
    P = B.shape[0]
    cv = _object(P, F, B)
    if pairs:
        got = cv.pair_counts()
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), ref.pair_counts(B))
        assert torch.equal(cv.pair_counts(), got)                            # two runs: the same bits
    for f in _frames_of(F):
        fc = cv.frame_counts(f)
        assert np.array_equal(fc.cpu().numpy(), ref.frame_counts(B, f)), f
        assert torch.equal(cv.frame_counts(_word(f)), fc) and torch.equal(cv.frame_counts(f), fc)
        own = ref.frame_counts(B, f)[f]
        want = ref.frame_counts(B, f).astype(np.float32) / np.float32(max(own, 1)) if own else np.zeros(F, np.float32)
        assert np.allclose(cv.overlap(f).cpu().numpy(), want, rtol=2.0 ** -22, atol=0.0), f   # (the one float: a float32 division by torch, within an ulp)
    assert not bool(cv.frame_counts(_word(F)).any()) and not bool(cv.frame_counts(_word(-1)).any())
    rng = np.random.default_rng(F)
    masks = [None, np.ones(F, bool), np.zeros(F, bool), rng.random(F) < 0.5, np.arange(F) == F - 1]
    for mask in masks:
        assert np.array_equal(cv.seen_count(mask).cpu().numpy(), ref.seen_count(B, mask))
        for min_others in (0, 2):
            red = cv.redundant(min_others, mask)
            assert np.array_equal(red.cpu().numpy(), ref.redundant(B, min_others, mask)), min_others
            assert torch.equal(cv.redundant(min_others, mask), red)
    assert np.array_equal(cv.seen_count(np.flatnonzero(masks[3])).cpu().numpy(), ref.seen_count(B, masks[3]))   # frame indices name the same mask
    assert np.array_equal(cv.seen_by_fewer_than(2).cpu().numpy(), ref.seen_count(B) < 2)
    assert np.array_equal(cv.bits().cpu().numpy().view(np.uint32), ref.pack(B))   # the queries wrote nothing into the rows


@pytest.mark.parametrize("F", [1, 33, 128])
def test_counts_on_a_designed_matrix(F):
    P = P_REC
    B = _designed(P, F)
    pair = ref.pair_counts(B)
    for f in range(1, min(F, 12)):                                           # the closed form: rows that f and g both divide
        for g in range(1, min(F, 12)):
            assert pair[f, g] == P // np.lcm(f, g)
    assert pair[0, 0] == P // 3
    _check_queries(B, F, pairs=True)


@pytest.mark.parametrize("density", [0.1, 0.9])
@pytest.mark.parametrize("F", [1, 33, 128])
def test_counts_on_random_matrices_over_many_workgroups(F, density):
    _check_queries(ref.random_matrix(P_BIG, F, density, 17 * F + int(10 * density)), F, pairs=True)


@pytest.mark.parametrize("P,density", [(P_REC, 0.5), (P_BIG // 10, 0.1)])
def test_frame_and_row_counts_at_1024_frames(P, density):
    _check_queries(ref.random_matrix(P, 1024, density, 1024 + P), 1024, pairs=False)


def test_stale_bits_above_the_frame_count_are_ignored():
    """Bits f >= F of the last word are no part of the state: a row array that holds some (loaded from elsewhere) counts as if they were clear."""
    P, F = 300, 33
    B = ref.random_matrix(P, F, 0.5, 8)
    cv = _object(P, F, B)
    cv._bits[:, 1] |= -2                                                     # every bit of word 1 above bit 0
    assert np.array_equal(cv.pair_counts().cpu().numpy(), ref.pair_counts(B))
    assert np.array_equal(cv.frame_counts(32).cpu().numpy(), ref.frame_counts(B, 32))
    assert np.array_equal(cv.seen_count().cpu().numpy(), ref.seen_count(B)) and np.array_equal(cv.redundant(1).cpu().numpy(), ref.redundant(B, 1))


def test_outputs_stay_inside_their_arrays():
    _trainer, _lib = _mods()
    L = _lib.lib()
    P, F = P_REC, 33
    B = ref.random_matrix(P, F, 0.5, 4)
    bits = _dev(ref.pack(B).view(np.int32))
    pb, pair = guarded(F * F, fill=7)
    fb, out = guarded(F, fill=7)
    nb, n_seen = guarded(P, fill=7)
    rb, red = guarded(F, fill=7)
    s = _lib.current_stream_ptr()
    _lib.check(L.gslic_covis_pair_counts(P, F, _lib.ptr(bits), _lib.ptr(pair), s))
    _lib.check(L.gslic_covis_frame_counts(P, F, _lib.ptr(bits), _lib.ptr(_word(32)), _lib.ptr(out), s))
    _lib.check(L.gslic_covis_row_counts(P, F, _lib.ptr(bits), None, _lib.ptr(n_seen), 1, _lib.ptr(red), s))
    assert np.array_equal(pair.cpu().numpy().reshape(F, F), ref.pair_counts(B)) and guards_intact(pb, F * F)      # (the calls zero their outputs)
    assert np.array_equal(out.cpu().numpy(), ref.frame_counts(B, 32)) and guards_intact(fb, F)
    assert np.array_equal(n_seen.cpu().numpy(), ref.seen_count(B)) and guards_intact(nb, P)
    assert np.array_equal(red.cpu().numpy(), ref.redundant(B, 1)) and guards_intact(rb, F)


# ---------------------------------------------------------------------------------------------------- GraphedStep on a 3-slot store
N_SLOTS, F_STEP = 3, 40                                                      # Wd = 2: the columns of the three slots share word 0, word 1 is a neighbour
ORDER = [0, 1, 2, 1]
VIEWS = (0, 3, 7)                                                            # synthetic_camera poses the three keyframes were taken from: yaw -14, -2 and
                                                                             # +14 degrees — on the 600-row scene their visible sets differ by 126 to 305 rows


def _model():
    trainer, _lib = _mods()
    m = trainer.GaussianModel(gr.scene(600, 3), gpu())
    m.training_setup()
    return m


@functools.lru_cache(maxsize=None)
def _step_inputs():
    from gaussian_lic_amd.camera import synthetic_camera
    trainer, _lib = _mods()
    W, H = gr.W, gr.H
    cams = [synthetic_camera(W, H, v).to_device(gpu()) for v in VIEWS]
    f, _mk = kref.random_frames(N_SLOTS, W, H, 50, masks=False)
    st = trainer.KeyframeStore(W, H, N_SLOTS, gpu())
    for s in range(N_SLOTS):
        assert st.add_u8(torch.from_numpy(f[s])) == s
    return cams, st, torch.zeros(3, device=gpu())


def _pose_set(cams):
    trainer, _lib = _mods()
    ps = trainer.PoseSet(N_SLOTS, cams[0], gpu(), lr_trans=2e-3, lr_rot=1e-3)
    for v, c in enumerate(cams):
        ps.load(v, c)
    return ps


def _prefilled(model):
    """A Covisibility of the model whose rows start from a random pattern, and that pattern."""
    trainer, _lib = _mods()
    cv = trainer.Covisibility(model, F_STEP)
    B0 = ref.random_matrix(model.P, F_STEP, 0.5, 77)
    cv._bits[:model.P].copy_(_dev(ref.pack(B0).view(np.int32)))
    return cv, B0


def _got(cv):
    return ref.unpack(cv.bits().cpu().numpy(), cv.n_frames)


@pytest.mark.parametrize("train_pose", [False, True])
@pytest.mark.parametrize("use_graph", [False, True])
def test_graphed_step_records_the_column_of_the_frame_it_trained_on(use_graph, train_pose):
    """Steps over frames 0, 1, 2, 1: column f is radii > 0 of an independent forward from frame f's camera (under train_pose: from the pose row as
    it stood) on the map as it stood before that step; every other bit is untouched; building and capturing the step recorded nothing; and the
    map (and the poses) are bit-identical to the same steps with covis=None."""
    trainer, _lib = _mods()
    cams, st, bg = _step_inputs()
    a, b, c = _model(), _model(), _model()
    cv, B0 = _prefilled(a)
    pa, pb, pc = (_pose_set(cams) if train_pose else None for _ in range(3))
    kw = dict(use_graph=use_graph, keyframes=st, frame=0)
    kw_a, kw_b = (dict(kw, poses=p, view=0, train_pose=True) if train_pose else kw for p in (pa, pb))
    ga = trainer.GraphedStep(a, cams[0], None, bg, covis=cv, **kw_a)
    gb = trainer.GraphedStep(b, cams[0], None, bg, **kw_b)
    assert np.array_equal(_got(cv), B0)                                      # warm-up and capture left no record behind
    for j in ORDER:
        if train_pose:
            ga.step(frame=j, view=j); gb.step(frame=j, view=j)
        else:
            ga.step(cams[j], frame=j); gb.step(cams[j], frame=j)
    assert ga.check() == 0 and gb.check() == 0
    assert_same_state(model_state(a), model_state(b))                        # recording changed nothing of the training
    if train_pose:
        for name in ("view", "proj", "campos", "m", "v", "steps"):
            assert torch.equal(getattr(pa, name), getattr(pb, name)), name
    # the reference: eager steps of the host paths on a third model, with a forward of its own in front of each
    want = B0.copy()
    for j in ORDER:
        cam_j = pc.camera(j) if train_pose else cams[j]
        radii = raw_forward(c, cam_j).state[2]
        want[:, j] = (radii > 0).cpu().numpy()
        if train_pose:
            trainer.training_step_with_pose(c, cams[0], st.target(j), bg, poses=pc, view=j, adam_in_backward=True)
        else:
            trainer.training_step_fused(c, cams[j], st.target(j), bg)
    assert_same_state(model_state(a), model_state(c))                        # (the reference ran the same training)
    got = _got(cv)
    assert np.array_equal(got[:, :N_SLOTS], want[:, :N_SLOTS]) and np.array_equal(got, want)
    assert all(0 < want[:, j].sum() < a.P for j in range(N_SLOTS))
    assert all((want[:, i] != want[:, j]).sum() > 50 for i, j in ((0, 1), (1, 2), (0, 2)))   # the three cameras see different rows
    assert torch.equal(cv.rows_of(1), ga.visible)                            # the last step trained frame 1


def test_a_step_that_did_not_fit_records_nothing_until_it_is_repeated():
    trainer, _lib = _mods()
    cams, st, bg = _step_inputs()
    a, c = _model(), _model()
    cv, B0 = _prefilled(a)
    small = max(64, raw_forward(a, cams[1]).state[0] // 2)                   # half the instances the view has: a declined step, not a fault
    ga = trainer.GraphedStep(a, cams[1], None, bg, keyframes=st, frame=1, cap_R=small, check_every=0, covis=cv)
    ga.step(cams[1], frame=1)
    assert np.array_equal(_got(cv), B0)                                      # the column is as it was
    assert ga.check() == 1                                                   # the repeat, on larger buffers, records
    want = B0.copy()
    want[:, 1] = (raw_forward(c, cams[1]).state[2] > 0).cpu().numpy()
    assert np.array_equal(_got(cv), want)


def test_graphed_step_refusals_and_the_unchanged_call_list():
    trainer, _lib = _mods()
    cams, st, bg = _step_inputs()
    m = _model()
    cv = trainer.Covisibility(m, F_STEP)
    with pytest.raises(ValueError, match="without keyframes"):
        trainer.GraphedStep(m, cams[0], st.target(0), bg, covis=cv)
    with pytest.raises(ValueError, match="column = slot"):
        trainer.GraphedStep(m, cams[0], None, bg, keyframes=st, frame=0, covis=trainer.Covisibility(m, N_SLOTS - 1))
    with pytest.raises(ValueError, match="Covisibility of the model"):
        trainer.GraphedStep(m, cams[0], None, bg, keyframes=st, frame=0, covis=trainer.Covisibility(_model(), F_STEP))

    class Calls:
        def __init__(self, real):
            self._real, self.names = real, []

        def __getattr__(self, sym):
            fn = getattr(self._real, sym)
            if not sym.startswith("gslic_"):
                return fn

            def call(*args):
                self.names.append(sym)
                return fn(*args)
            return call
    plain = trainer.GraphedStep(_model(), cams[0], None, bg, keyframes=st, frame=0)
    keyed = trainer.GraphedStep(m, cams[0], None, bg, keyframes=st, frame=0, covis=cv)
    real = _lib.lib()
    rec = Calls(real)
    _lib._lib = rec
    try:
        plain.step(cams[0], frame=1)
        n = len(rec.names)
        keyed.step(cams[0], frame=1)
    finally:
        _lib._lib = real
    first, second = rec.names[:n], rec.names[n:]
    assert first == ["gslic_keyframe_decode", "gslic_rasterize_forward_capacity", "gslic_l1_ssim_loss_forward_backward", "gslic_rasterize_backward_adam"]
    assert second == first + ["gslic_covis_record"]                          # one launch more, behind the backward; covis=None: the step as it was


# ---------------------------------------------------------------------------------------------------- carriage
def test_bits_follow_the_rows():
    """prune, densify (clone and split), extend and resort on a Morton model: rows_of(f) is the old mask moved by the edit's own index, new rows and
    split parents are zero — at a width (F = 70: three words) none of the map's own arrays has."""
    trainer, _lib = _mods()
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import lidar_scene
    dev, P, F = gpu(), 600, 70
    d = trainer.GaussianModel(gr.scene(P, 3), dev, order="morton", resort_fraction=None)
    d.training_setup()
    cams = [synthetic_camera(gr.W, gr.H, v).to_device(dev) for v in gr.VIEWS]
    cv = trainer.Covisibility(d, F)
    B = ref.random_matrix(P, F, 0.3, 21)
    for f in range(F):
        cv.record(f, _dev(B[:, f]))
    for k, f in enumerate((0, 33, 69)):                                      # three real views among the random columns
        radii = raw_forward(d, cams[k]).state[2]
        B[:, f] = (radii > 0).cpu().numpy()
        cv.record(f, radii)
    assert np.array_equal(_got(cv), B)
    stale = trainer.Covisibility(d, F)
    stale.detach()
    # prune: old[kept]
    drop = _dev(np.random.default_rng(3).random(P) < 0.25)
    n, kept = d.prune(drop=drop)
    B = B[kept.cpu().numpy()]
    assert n == int(drop.sum()) and np.array_equal(_got(cv), B) and not bool(cv._bits[d.P:].any())
    assert all(np.array_equal(cv.rows_of(f).cpu().numpy(), B[:, f]) for f in (0, 31, 32, 33, 69))
    with pytest.raises(RuntimeError, match="rows changed"):
        stale.rows_of(0)
    # densify: new rows and split parents zero, everything else as it was
    P0 = d.P
    grow = _dev(np.random.default_rng(4).random(P0) < 0.3)
    split_scale = float(torch.exp(d.scaling.detach()).max(1).values.median())
    over = (d.scaling.detach() > trainer.densify_threshold(split_scale)).any(1).cpu()
    k, n_split, parents = d.densify(grow, split_scale=split_scale)
    assert k > 0 and 0 < n_split < k and d.P == P0 + k
    split = torch.zeros(P0, dtype=torch.bool)
    split[parents.cpu()] = True
    split &= over
    assert int(split.sum()) == n_split
    B[split.numpy()] = False                                                 # child 0 has been seen by nothing yet; a clone's parent keeps its bits
    B = np.concatenate([B, np.zeros((k, F), bool)])
    assert np.array_equal(_got(cv), B)
    # extend: appended rows zero
    P0, cam = d.P, cams[0]
    frame = lidar_scene(300, gr.W, gr.H, sh_degree=0, seed=77)
    col = (frame["features_dc"].reshape(-1, 3) * 0.28209479177387814 + 0.5).to(dev)
    Rcw = torch.from_numpy(cam.world_view_transform[:3, :3].T.copy())
    tcw = torch.from_numpy(cam.world_view_transform[3, :3].copy())
    k = d.extend(cam, frame["xyz"].to(dev), col, frame["xyz"][:, 2].contiguous().to(dev), Rcw, tcw, (float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy)))
    assert k > 0 and d.P == P0 + k
    B = np.concatenate([B, np.zeros((k, F), bool)])
    assert np.array_equal(_got(cv), B)
    # resort: the permutation
    perm = d.resort().cpu().numpy()
    assert not np.array_equal(perm, np.arange(d.P))
    B = B[perm]
    assert np.array_equal(_got(cv), B) and np.array_equal(cv.pair_counts().cpu().numpy(), ref.pair_counts(B))
    # a state_dict survives the trip to another object of the same rows
    other = trainer.Covisibility(d, F)
    other.load_state_dict(cv.state_dict())
    assert torch.equal(other.bits(), cv.bits())


# ---------------------------------------------------------------------------------------------------- the C++ host
@pytest.mark.parametrize("order,F", [("insertion", 40), ("morton", 200)])
def test_fused_covis_cpp_host(tmp_path, order, F):
    """gslic::Covisibility behind gslic::FusedStep::set_covisibility issues the calls of the Python host: through steps recorded as changing
    frames, a densify(), a prune(), a clear and a resort(), the bits, the 19 row arrays and every query are bit-identical to the Python host's."""
    trainer, _lib = _mods()
    from gaussian_lic_amd.camera import synthetic_camera
    from gaussian_lic_amd.synthetic import gt_image
    exe = fio.build("fused_covis")
    P, iters, seed = 600, 2, 11
    m = trainer.GaussianModel(gr.scene(P, 3), gpu(), order=order, resort_fraction=None)
    m.training_setup()
    cams = [synthetic_camera(gr.W, gr.H, v).to_device(gpu()) for v in gr.VIEWS[:2]]
    gt = gt_image(gr.H, gr.W, seed=5).to(gpu())
    bg = torch.zeros(3, device=gpu())
    d = str(tmp_path)
    fio.write_inputs(d, m, cams, gt=gt, tie_rank=m.tie_rank)
    st, cv = trainer.GradientStats(m), trainer.Covisibility(m, F)
    count = [0, 0]

    def steps():
        for _ in range(iters):
            _terms, visible = trainer.training_step_fused(m, cams[count[0] % 2], gt, bg, grad_stats=st)
            count[1] = (5 * count[0]) % F
            cv.record(count[1], visible)
            count[0] += 1
    steps()
    grad_above = float(np.float32(st.mean_gradient()[st.n_seen() > 0].median().item()))
    split_scale = float(torch.exp(m.scaling.detach().double()).max(1).values.median())
    k, n_split, _parents = m.densify(st.grow_mask(grad_above), split_scale, seed=seed)
    assert 0 < n_split < k < P
    steps()
    rlim = int(st.max_radius()[st.n_seen() > 0].float().median())
    n, _kept = m.prune(drop=st.big_mask(rlim))
    assert 0 < n < m.P
    steps()
    cv.clear(0)
    m.to_morton_order(resort_fraction=None) if order == "insertion" else m.resort()
    steps()
    r = fio.run(exe, d, str(P), str(gr.W), str(gr.H), "3", str(iters), repr(grad_above), str(rlim), repr(split_scale), str(seed), str(F))
    assert f"densify added {k} splits {n_split} pruned {n} size {m.P}" in r.stdout, r.stdout
    rd = functools.partial(fio.read, d)
    Pn, last = m.P, count[1]
    assert torch.equal(rd("xyz.f32", np.int32), m._buf["xyz"][:Pn].contiguous().view(torch.int32).cpu().reshape(-1))   # the same map
    assert torch.equal(rd("covis_bits.i32", np.int32), cv.bits().cpu().reshape(-1)) and bool(cv.bits().any())
    assert torch.equal(rd("covis_frame.i64", np.int64), cv.frame_counts(last).cpu())
    assert torch.equal(rd("covis_seen.i32", np.int32), cv.seen_count().cpu())
    assert torch.equal(rd("covis_red.i64", np.int64), cv.redundant(1).cpu())
    assert torch.equal(rd("covis_fewer.u8", np.uint8), cv.seen_by_fewer_than(2).to(torch.uint8).cpu())
    assert torch.equal(rd("covis_overlap.f32", np.int32), cv.overlap(last).view(torch.int32).cpu())
    if F <= 128:
        assert torch.equal(rd("covis_pair.i64", np.int64), cv.pair_counts().cpu().reshape(-1))
    B = _got(cv)
    assert not B[:, 0].any() and B[:, last].any()                            # frame 0 was cleared and not recorded since
    assert np.array_equal(cv.seen_count().cpu().numpy(), ref.seen_count(B))
