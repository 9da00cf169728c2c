"""No GPU: the covisibility restatement (tests/covis_ref.py) on hand-made cases, its packing at every word-boundary frame count, the four
gslic_covis_* exports declared, bound and refusing bad arguments before any device work, and the bookkeeping of trainer.Covisibility on a CPU
model (its carriage operations that need no kernel, the queries that are torch, state_dict, the refusals)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import covis_ref as ref
import gradstats_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gslic_covis_record", "gslic_covis_pair_counts", "gslic_covis_frame_counts", "gslic_covis_row_counts")
vp = ctypes.c_void_p


def _libs():
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import _lib
    return _lib, _lib.lib()


# ---------------------------------------------------------------------------------------------------- the restatement
def test_restatement_on_a_hand_made_matrix():
    #               f0 f1 f2
    B = np.array([[1, 1, 0],
                  [1, 0, 0],
                  [0, 1, 1],
                  [1, 1, 1],
                  [0, 0, 0]], dtype=bool)
    assert ref.pair_counts(B).tolist() == [[3, 2, 1], [2, 3, 2], [1, 2, 2]]
    assert ref.frame_counts(B, 0).tolist() == [3, 2, 1] and ref.frame_counts(B, 2).tolist() == [1, 2, 2] and ref.frame_counts(B, 3).tolist() == [0, 0, 0]
    assert ref.seen_count(B).tolist() == [2, 1, 2, 3, 0]
    assert ref.seen_count(B, [True, False, True]).tolist() == [1, 1, 1, 2, 0]
    assert ref.redundant(B, 0).tolist() == [3, 3, 2]                       # every seen row counts: the diagonal
    assert ref.redundant(B, 1).tolist() == [2, 3, 2]                       # row 1 is seen by frame 0 alone
    assert ref.redundant(B, 2).tolist() == [1, 1, 1]
    assert ref.redundant(B, 1, [True, False, True]).tolist() == [1, 1, 1]  # only row 3 is seen by both of frames 0 and 2
    assert ref.pack(B).reshape(-1).tolist() == [3, 1, 6, 7, 0]


def test_record_replaces_clears_and_respects_range_skip_and_frame():
    B = np.zeros((4, 3), dtype=bool)
    ref.record(B, 1, np.array([5, 0, -2, 1]))
    assert B[:, 1].tolist() == [True, False, False, True] and not B[:, [0, 2]].any()
    ref.record(B, 1, np.array([0, 7, 0, 0]))                                # replaces, does not OR
    assert B[:, 1].tolist() == [False, True, False, False]
    ref.record(B, 1, np.array([1, 1, 1, 1]), rows=(2, 4))
    assert B[:, 1].tolist() == [False, True, True, True]
    before = B.copy()
    ref.record(B, 1, np.array([0, 0, 0, 0]), skip=1)
    ref.record(B, 3, np.array([1, 1, 1, 1]))
    ref.record(B, -1, np.array([1, 1, 1, 1]))
    assert np.array_equal(B, before)
    ref.record(B, 1, None)
    assert not B.any()


@pytest.mark.parametrize("F", ref.FRAME_COUNTS)
def test_packing_round_trips(F):
    assert ref.words(F) == -(-F // 32)
    B = ref.random_matrix(37, F, 0.5, F)
    bits = ref.pack(B)
    assert bits.shape == (37, ref.words(F)) and bits.dtype == np.uint32
    assert np.array_equal(ref.unpack(bits, F), B) and np.array_equal(ref.unpack(bits.view(np.int32), F), B)
    for f in {0, min(31, F - 1), min(32, F - 1), F - 1}:
        one = np.zeros((1, F), dtype=bool)
        one[0, f] = True
        w = ref.pack(one)[0]
        assert int(w[f >> 5]) == 1 << (f & 31) and int(w.astype(np.uint64).sum()) == 1 << (f & 31)
    if F & 31:                                                              # bits f >= F of the last word stay clear
        assert not (ref.pack(np.ones((1, F), dtype=bool))[0, -1] >> np.uint32(F & 31))


# ---------------------------------------------------------------------------------------------------- the exports
def test_exports_are_declared_bound_and_abi_stays():
    _lib, L = _libs()
    header = open(os.path.join(ROOT, "include", "gslic_hip.h")).read()
    assert L.gslic_abi_version() == 8
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name)
        decl = re.search(r"int %s\((.*?)\);" % name, header, re.S)
        assert decl is not None, name
        args = [a for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",") if a.strip()]
        assert len(args) == len(getattr(L, name).argtypes), name
    from gaussian_lic_amd import trainer
    assert "#define GSLIC_COVIS_MAX_FRAMES %d" % trainer.COVIS_MAX_FRAMES in header
    assert "#define GSLIC_COVIS_MAX_PAIR_FRAMES %d" % trainer.COVIS_MAX_PAIR_FRAMES in header


BITS, RADII, VIS, WORD, SKIP, OUT, MASK, NSEEN = (vp(0x100000 + 0x100000 * i) for i in range(8))   # dummies, far apart, never dereferenced


def _refused(L, fn, args, word):
    rc = fn(*args)
    msg = L.gslic_last_error().decode()
    assert rc == -1 and word in msg, (fn.__name__, args, rc, msg)


def test_record_refuses_bad_arguments_before_any_device_work():
    _lib, L = _libs()
    fn = L.gslic_covis_record
    P, F = 100, 40                                                          # Wd = 2: bits is 800 bytes

    def args(**kw):
        a = dict(P=P, F=F, bits=BITS, radii=RADII, visible=None, frame_word=WORD, skip=SKIP, row_begin=0, row_end=-1)
        a.update(kw)
        return [a[k] for k in ("P", "F", "bits", "radii", "visible", "frame_word", "skip", "row_begin", "row_end")] + [None]
    _refused(L, fn, args(P=-1), "P = -1")
    for bad in (0, -5, 1025):
        _refused(L, fn, args(F=bad), "F = %d" % bad)
    _refused(L, fn, args(bits=None), "bits is NULL")
    _refused(L, fn, args(frame_word=None), "frame_word is NULL")
    _refused(L, fn, args(visible=VIS), "both given")
    for r0, r1 in ((-1, 4), (5, 4), (0, 101), (101, -1)):
        _refused(L, fn, args(row_begin=r0, row_end=r1), "row range")
    inside = vp(BITS.value + 796)                                           # the last word of bits
    _refused(L, fn, args(radii=inside), "bits overlaps radii")
    _refused(L, fn, args(radii=None, visible=inside), "bits overlaps visible")
    _refused(L, fn, args(frame_word=inside), "bits overlaps frame_word")
    _refused(L, fn, args(skip=inside), "bits overlaps skip")
    _refused(L, fn, args(radii=vp(BITS.value - 4 * P + 4)), "bits overlaps radii")   # radii's last word is bits' first
    assert fn(*args(row_begin=7, row_end=7)) == 0                           # an empty range: nothing to do
    assert fn(*args(P=0, radii=None, skip=None)) == 0                       # no rows


def test_queries_refuse_bad_arguments_before_any_device_work():
    _lib, L = _libs()
    P = 100
    pair, frame, rows = L.gslic_covis_pair_counts, L.gslic_covis_frame_counts, L.gslic_covis_row_counts
    # pair counts: F <= 128
    _refused(L, pair, [-2, 64, BITS, OUT, None], "P = -2")
    for bad in (0, 129, 1024):
        _refused(L, pair, [P, bad, BITS, OUT, None], "F = %d" % bad)
    _refused(L, pair, [P, 64, None, OUT, None], "bits is NULL")
    _refused(L, pair, [P, 64, BITS, None, None], "pair is NULL")
    _refused(L, pair, [P, 64, BITS, vp(BITS.value + 799), None], "pair overlaps bits")
    _refused(L, pair, [P, 64, BITS, vp(BITS.value - 4 * 64 * 64 + 1), None], "pair overlaps bits")
    # frame counts: any F up to 1024
    _refused(L, frame, [-1, 64, BITS, WORD, OUT, None], "P = -1")
    for bad in (0, 1025):
        _refused(L, frame, [P, bad, BITS, WORD, OUT, None], "F = %d" % bad)
    _refused(L, frame, [P, 64, None, WORD, OUT, None], "bits is NULL")
    _refused(L, frame, [P, 64, BITS, None, OUT, None], "frame_word is NULL")
    _refused(L, frame, [P, 64, BITS, WORD, None, None], "out is NULL")
    _refused(L, frame, [P, 64, BITS, WORD, vp(BITS.value + 4), None], "out overlaps bits")
    _refused(L, frame, [P, 64, BITS, WORD, vp(WORD.value - 252), None], "out overlaps frame_word")
    # row counts
    _refused(L, rows, [-1, 64, BITS, MASK, NSEEN, 0, OUT, None], "P = -1")
    for bad in (0, 1025):
        _refused(L, rows, [P, bad, BITS, MASK, NSEEN, 0, OUT, None], "F = %d" % bad)
    _refused(L, rows, [P, 64, None, MASK, NSEEN, 0, OUT, None], "bits is NULL")
    _refused(L, rows, [P, 64, BITS, MASK, None, 0, OUT, None], "n_seen is NULL")
    _refused(L, rows, [P, 64, BITS, MASK, NSEEN, -1, OUT, None], "min_others = -1")
    _refused(L, rows, [P, 64, BITS, MASK, vp(BITS.value + 796), 0, OUT, None], "n_seen overlaps bits")
    _refused(L, rows, [P, 64, BITS, MASK, vp(MASK.value + 4), 0, OUT, None], "n_seen overlaps frame_mask")
    _refused(L, rows, [P, 64, BITS, MASK, NSEEN, 0, vp(BITS.value), None], "redundant overlaps bits")
    _refused(L, rows, [P, 64, BITS, MASK, NSEEN, 0, vp(MASK.value + 4), None], "redundant overlaps frame_mask")
    _refused(L, rows, [P, 64, BITS, MASK, NSEEN, 0, vp(NSEEN.value + 396), None], "redundant overlaps n_seen")


# ---------------------------------------------------------------------------------------------------- the Python object, on a CPU model
def _cpu_model(P=96, capacity=200):
    import gaussian_lic_amd  # noqa: F401
    from gaussian_lic_amd import trainer
    return trainer, trainer.GaussianModel(gr.scene(P, 3), torch.device("cpu"), capacity=capacity)


def _load(cv, B):
    cv._bits[:B.shape[0]] = torch.from_numpy(ref.pack(B).view(np.int32))


@pytest.mark.parametrize("F", [1, 33, 128])
def test_object_on_a_cpu_model_tracks_the_rows(F):
    trainer, m = _cpu_model()
    cv = trainer.Covisibility(m, F)
    W = ref.words(F)
    assert cv.n_frames == F and cv.words == W
    assert [(tuple(a.shape), a.dtype, w) for a, w in cv._arrays()] == [((200, W), torch.int32, W)] and not bool(cv._bits.any())
    assert m._attached_stats() == [cv]
    B = ref.random_matrix(96, F, 0.4, 7 + F)
    _load(cv, B)
    assert cv.bits().shape == (96, W)
    for f in {0, F - 1, min(31, F - 1), min(32, F - 1)}:
        assert cv.rows_of(f).dtype == torch.bool and np.array_equal(cv.rows_of(f).numpy(), B[:, f]), f
    with pytest.raises(IndexError):
        cv.rows_of(F)
    # the carriage that needs no kernel: a permutation by torch indexing (GSLIC_RESORT=torch), zeroed split parents, appended rows
    perm = torch.randperm(96, generator=torch.Generator().manual_seed(3))
    cv._permute(perm)
    B = B[perm.numpy()]
    assert np.array_equal(ref.unpack(cv.bits().numpy(), F), B)
    cv._zero_rows(torch.tensor([0, 95]))
    B[[0, 95]] = False
    assert np.array_equal(ref.unpack(cv.bits().numpy(), F), B)
    cv._bits[96:100] = -1                                                   # what stale storage behind P could hold
    m.P = 100
    cv._appended(96, 4)
    assert np.array_equal(ref.unpack(cv.bits().numpy(), F), np.concatenate([B, np.zeros((4, F), bool)]))
    m.P = 96
    cv._sync()
    # state_dict round trip, and its refusals
    state = cv.state_dict()
    assert state["n_frames"] == F and tuple(state["bits"].shape) == (96, W)
    other = trainer.Covisibility(m, F)
    other.load_state_dict(state)
    assert torch.equal(other.bits(), cv.bits())
    with pytest.raises(ValueError, match="load_state_dict"):
        other.load_state_dict(dict(n_frames=F + 1, bits=state["bits"]))
    with pytest.raises(ValueError, match="load_state_dict"):
        other.load_state_dict(dict(n_frames=F, bits=state["bits"][:-1]))
    cv.reset()
    assert not bool(cv._bits.any())
    cv.detach()
    assert m._attached_stats() == [other]
    m._rows_version += 1
    with pytest.raises(RuntimeError, match="Covisibility: the model's rows changed"):
        cv.rows_of(0)
    with pytest.raises(RuntimeError, match="rows changed"):
        cv.record(0, None)


def test_object_refusals():
    trainer, m = _cpu_model()
    for bad in (0, -1, 1025):
        with pytest.raises(ValueError, match="n_frames"):
            trainer.Covisibility(m, bad)
    cv = trainer.Covisibility(m, 200)
    with pytest.raises(ValueError, match="above 128"):
        cv.pair_counts()
    with pytest.raises(IndexError):
        cv.record(200, None)
    with pytest.raises(ValueError, match="frame word"):
        cv.record(torch.zeros(1, dtype=torch.int64), None)
    with pytest.raises(ValueError, match="seen must be"):
        cv.record(0, torch.zeros(96, dtype=torch.float32))
    with pytest.raises(ValueError, match="seen must be"):
        cv.record(0, torch.zeros(95, dtype=torch.int32))
    with pytest.raises(ValueError, match="min_others"):
        cv.redundant(-1)
    with pytest.raises(ValueError, match="frame mask must have"):
        cv.seen_count(np.ones(199, dtype=bool))
    # the frame mask words
    assert cv._mask_words(None) is None
    got = cv._mask_words([0, 31, 32, 199]).numpy().view(np.uint32)
    want = np.zeros(200, dtype=bool)
    want[[0, 31, 32, 199]] = True
    assert np.array_equal(got, ref.pack(want[None])[0]) and np.array_equal(cv._mask_words(want).numpy().view(np.uint32), got)
    # GraphedStep's argument checks
    assert trainer._covis_for_step(None, m, None) is None
    with pytest.raises(ValueError, match="without keyframes"):
        trainer._covis_for_step(cv, m, None)
    _t, m2 = _cpu_model(8, 8)
    with pytest.raises(ValueError, match="Covisibility of the model"):
        trainer._covis_for_step(trainer.Covisibility(m2, 4), m, None)
    store = trainer.KeyframeStore(8, 4, 201, torch.device("cpu"))
    with pytest.raises(ValueError, match="column = slot"):
        trainer._covis_for_step(cv, m, store)
    assert trainer._covis_for_step(cv, m, trainer.KeyframeStore(8, 4, 200, torch.device("cpu"))) is cv


def test_single_gpu_only(monkeypatch):
    trainer, m = _cpu_model()
    monkeypatch.setattr(trainer, "_dist_on", lambda: True)
    with pytest.raises(NotImplementedError, match="single-GPU"):
        trainer.Covisibility(m, 8)
