"""-m gpu: the keyframe store's depth slabs — the decode and encode kernels (gslic_keyframe_decode_depth / gslic_keyframe_encode_depth) against the
numpy restatement of their rules (tests/keyframe_depth_ref.py) bit for bit, the frame word, the LiDAR pyramid (one stored range image serves every
level), the store through GraphedStep (eager and captured, with trainable poses) and the C++ host.  Bit comparisons: no tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch

import fused_check_io as fio
import keyframe_depth_ref as ref
import keyframe_ref as kref
from conftest import make_scene
from gpu_helpers import SENTINEL, assert_same_state, bits, gpu, guarded, guards_intact, model_state, raw_forward, scene_model, training_model

pytestmark = pytest.mark.gpu

# the colour tests' shapes: (4,1) and (64,2) take the four-pixel path (level 0, and level 1 of 64 x 2), every other width the one-pixel path;
# (130,33): more than one workgroup on either path, remainders at every level
SHAPES = [(4, 1), (5, 3), (7, 5), (64, 2), (67, 9), (130, 33)]
N_SLOTS = 3
STEP = float(ref.DEFAULT_STEP)
LAMBDA_D, HUBER = 0.4, 0.05


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu())


def _i32(t):
    return t.cpu().numpy().view(np.int32)


@functools.lru_cache(maxsize=None)
def _frames(W, H, kind):
    """Three float depth frames and weights of a shape, their codes, and every level's reference with and without weights, computed once and left
    unchanged.  kind: "random", "zeros" (nothing measured), "far" (every pixel at code 65535)."""
    if kind == "random":
        d, w = ref.random_depth_frames(N_SLOTS, W, H, 1000 * H + W)
    else:
        d = np.full((N_SLOTS, H, W), 0.0 if kind == "zeros" else 65535 * STEP, np.float32)
        w = np.ones((N_SLOTS, H, W), np.float32)
    codes, wc = ref.encode(d), ref.encode_weight(w)
    levels = kref.levels(W, H, top=3)
    want = {(s, l, ws): ref.decode(codes[s], wc[s] if ws else None, l) for s in range(N_SLOTS) for l in levels for ws in (False, True)}
    return d, w, codes, wc, levels, want


def _store(W, H, d, w=None, capacity=N_SLOTS, masks=False):
    from gaussian_lic_amd import trainer
    st = trainer.KeyframeStore(W, H, capacity, gpu(), masks=masks, depths=True, depth_weights=w is not None)
    colour = kref.random_frames(d.shape[0], W, H, 7)[0]
    for s in range(d.shape[0]):
        assert st.add_u8(torch.from_numpy(colour[s]), depth=_dev(d[s]), depth_weight=None if w is None else _dev(w[s])) == s
    return st


def _guarded_pair(Wl, Hl, weights):
    db, dw = guarded(Hl * Wl)
    wb, ww = guarded(Hl * Wl) if weights else (None, None)
    return db, dw.view(torch.float32).view(Hl, Wl), wb, (ww.view(torch.float32).view(Hl, Wl) if weights else None)


def _codes(st, s=None):
    a = st.depth.cpu().numpy()
    return a if s is None else a[s]


# ---------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("W,H", SHAPES)
def test_decode_is_the_rule_bit_for_bit(W, H, weights):
    for kind in ("random", "zeros", "far"):
        d, w, codes, wc, levels, want = _frames(W, H, kind)
        st = _store(W, H, d, w if weights else None)
        assert st.n == N_SLOTS and st.nbytes == N_SLOTS * H * W * (6 if weights else 5) and st.has_depths and st.has_depth_weights == weights
        assert np.array_equal(_codes(st), codes) and (not weights or np.array_equal(st.dweight.cpu().numpy(), wc))
        for l in levels:
            Wl, Hl = kref.level_size(W, H, l)
            for s in (0, N_SLOTS - 1):
                db, dep, wb, wgt = _guarded_pair(Wl, Hl, weights)
                got = st.depth_target(s, l, out=(dep, wgt) if weights else dep)
                assert (got[0] if weights else got) is dep
                exp = want[(s, l, weights)]
                assert np.array_equal(_i32(dep), (exp[0] if weights else exp).view(np.int32)), (kind, l, s)
                assert guards_intact(db, Hl * Wl)
                if weights:
                    assert np.array_equal(_i32(wgt), exp[1].view(np.int32)), (kind, l, s)
                    assert guards_intact(wb, Hl * Wl)
                if kind == "zeros":
                    assert not dep.any() and (not weights or not wgt.any())
                if kind == "far":   # the last code at every level: 65535 * step, weight d(255)
                    assert bool((dep == 65535 * STEP).all()) and (not weights or bool((bits(wgt) == int(np.float32(255 * kref.C0).view(np.int32))).all()))
        assert np.array_equal(_codes(st), codes) and (not weights or np.array_equal(st.dweight.cpu().numpy(), wc))   # a decode writes no slot


def test_shapes_reach_both_paths_and_more_than_one_workgroup():
    fast = [(W, H, l) for W, H in SHAPES for l in kref.levels(W, H, 3) if W % (4 << l) == 0]
    slow = [(W, H, l) for W, H in SHAPES for l in kref.levels(W, H, 3) if W % (4 << l) != 0]
    assert fast == [(4, 1, 0), (64, 2, 0), (64, 2, 1)]
    assert (5, 3, 0) in slow and (67, 9, 3) in slow and (130, 33, 0) in slow and {l for _w, _h, l in slow} == {0, 1, 2, 3}
    assert 130 * 33 > 256 and (130 >> 1) * (33 >> 1) > 256 and 64 * 2 // 4 < 256   # KF_THREADS = 256 pixels (groups) per workgroup
    assert any(W % (1 << l) and H % (1 << l) for W, H, l in slow)                 # remainder columns and rows together


def test_a_wide_image_on_the_four_pixel_path_at_every_level():
    """512 x 24: W % (4 << l) == 0 up to level 4 — the 8- and 16-byte loads of codes, the 4-, 8- and 16-byte loads of weights and several source rows
    per lane — on more than one workgroup."""
    W, H = 512, 24
    d, w = ref.random_depth_frames(2, W, H, 77)
    codes, wc = ref.encode(d), ref.encode_weight(w)
    for weights in (False, True):
        st = _store(W, H, d, w if weights else None, capacity=2)
        for l in range(5):
            assert W % (4 << l) == 0 and (W >> l) * (H >> l) // 4 > (256 if l < 2 else 0)
            got = st.depth_target(1, l)
            exp = ref.decode(codes[1], wc[1] if weights else None, l)
            if weights:
                assert np.array_equal(_i32(got[0]), exp[0].view(np.int32)) and np.array_equal(_i32(got[1]), exp[1].view(np.int32)), l
            else:
                assert np.array_equal(_i32(got), exp.view(np.int32)), l


@pytest.mark.parametrize("W,H", [(67, 9), (64, 2)])   # one pixel per lane; four (H * W % 4 == 0)
def test_encode_is_the_rule_on_the_edge_values_and_leaves_the_other_slots(W, H):
    edges = np.concatenate(list(ref.edge_depths().values())).astype(np.float32)
    wvals = kref.edge_values()[0]
    assert edges.size <= H * W
    rng = np.random.default_rng(4)
    d, w = ref.random_depth_frames(N_SLOTS, W, H, 9)
    st = _store(W, H, d, w)
    before = (st.depth.clone(), st.dweight.clone())
    depth = np.resize(edges, H * W).reshape(H, W).astype(np.float32)                  # every edge depth, several times over
    weight = np.resize(wvals[rng.permutation(wvals.size)], H * W).reshape(H, W).astype(np.float32)
    assert st.put_depth(1, _dev(depth), _dev(weight)) == 1 and st.serial(1) == 1 and st.serial(0) == 0
    assert np.array_equal(_codes(st, 1), ref.encode(depth)) and np.array_equal(st.dweight[1].cpu().numpy(), ref.encode_weight(weight))
    got = st.depth_target(1)
    assert np.array_equal(_i32(got[0]), ref.quantised(depth).view(np.int32))           # decode_0(encode(D)) == the code-rounded D
    for s in (0, 2):
        assert np.array_equal(_codes(st, s), before[0][s].cpu().numpy()) and torch.equal(st.dweight[s], before[1][s])
    # no weight given: every weight 255; no depth given (put over a slot that had depth): nothing measured
    st.put_depth(2, _dev(depth))
    assert np.array_equal(_codes(st, 2), ref.encode(depth)) and int(st.dweight[2].min()) == 255
    colour = torch.from_numpy(kref.random_frames(1, W, H, 3)[0][0])
    st.put(1, u8=colour)
    assert not _codes(st, 1).any() and st.serial(1) == 2
    dep, wgt = st.depth_target(1)
    assert not dep.any() and not wgt.any()
    assert np.array_equal(_codes(st, 0), before[0][0].cpu().numpy())


@pytest.mark.parametrize("W,H,level", [(64, 2, 0), (67, 9, 1)])
def test_a_frame_word_out_of_range_writes_nothing(W, H, level):
    d, w, codes, wc, _levels, want = _frames(W, H, "random")
    st = _store(W, H, d, w)
    Wl, Hl = kref.level_size(W, H, level)
    for word in (-1, N_SLOTS, 2 ** 31 - 1):
        db, dep, wb, wgt = _guarded_pair(Wl, Hl, True)
        st._decode_depth(torch.tensor([word], dtype=torch.int32, device=gpu()), level, dep, wgt)
        torch.cuda.synchronize()
        assert bool((db == SENTINEL).all()) and bool((wb == SENTINEL).all()), word
    db, dep, wb, wgt = _guarded_pair(Wl, Hl, True)                       # the last valid word writes
    st._decode_depth(torch.tensor([N_SLOTS - 1], dtype=torch.int32, device=gpu()), level, dep, wgt)
    assert np.array_equal(_i32(dep), want[(N_SLOTS - 1, level, True)][0].view(np.int32)) and guards_intact(db, Hl * Wl)


def test_store_refusals():
    from gaussian_lic_amd import trainer
    W, H = 7, 5
    colour = torch.from_numpy(kref.random_frames(1, W, H, 3)[0][0])
    depth = torch.ones(H, W)
    plain = trainer.KeyframeStore(W, H, 2, gpu())
    with pytest.raises(ValueError, match="without depths"):
        plain.add_u8(colour, depth=depth)
    assert plain.n == 0
    plain.add_u8(colour)
    with pytest.raises(ValueError, match="without depths"):
        plain.put_depth(0, depth)
    with pytest.raises(ValueError, match="without depths"):
        plain.depth_target(0)
    st = trainer.KeyframeStore(W, H, 2, gpu(), depths=True)
    with pytest.raises(ValueError, match="without depth weights"):
        st.add_u8(colour, depth=depth, depth_weight=depth)
    with pytest.raises(ValueError, match="given to a store of"):
        st.add_u8(colour, depth=torch.ones(H, W + 1))
    assert st.add(torch.zeros(3, H, W), depth=depth) == 0 and float(st.depth_target(0)[0, 0]) == 1.0
    with pytest.raises(IndexError):
        st.put_depth(1, depth)
    with pytest.raises(ValueError, match="no level"):
        st.depth_target(0, 3)


# ---------------------------------------------------------------------------------------------------- the LiDAR pyramid
@pytest.mark.parametrize("level", [1, 2])
def test_one_stored_range_image_serves_the_level_cameras(level):
    """decode_l of the encoded level-0 LiDAR image == the code-rounded LiDAR image of camera.at_level(l) (the scene of
    test_keyframes_gpu.py::test_lidar_image_of_the_level_camera_is_the_positive_minimum_pool)."""
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    W, H = 64, 48
    cam = synthetic_camera(W, H, "se3_c").to_device(gpu())
    rng = np.random.default_rng(30 + level)
    pts = np.concatenate([rng.uniform(-4, 4, (6000, 2)), rng.uniform(0.5, 8.0, (6000, 1))], axis=1).astype(np.float32)
    pts = _dev(pts @ cam.R_wc.T.astype(np.float32) + cam.t_wc.astype(np.float32))
    st = trainer.KeyframeStore(W, H, 1, gpu(), depths=True)
    s = st.add(torch.zeros(3, H, W), depth=trainer.lidar_depth_image(cam, pts))
    want = ref.quantised(trainer.lidar_depth_image(cam.at_level(level), pts).cpu().numpy())
    got = st.depth_target(s, level)
    assert tuple(got.shape) == (H >> level, W >> level) and int((want > 0).sum()) > 100
    assert np.array_equal(_i32(got), want.view(np.int32))


# ---------------------------------------------------------------------------------------------------- GraphedStep
FRAMES_ORDER = [0, 2, 1, 2]


class _Calls:
    """Stands in front of the loaded library and records the name of every entry point that is called."""

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


def _step_setup(weights, masks=False, depths=True):
    from gaussian_lic_amd import trainer
    _m, cam = scene_model("a")
    W, H = cam.image_width, cam.image_height
    f, mk = kref.random_frames(N_SLOTS, W, H, 50, masks=True)
    d, w = ref.random_depth_frames(N_SLOTS, W, H, 51)
    d = np.where(d > 0, np.float32(2.0) + d * np.float32(0.05), d).astype(np.float32)   # metres in front of the scene's camera; the edge values stay
    st = trainer.KeyframeStore(W, H, N_SLOTS, gpu(), masks=masks, depths=depths, depth_weights=weights)
    for s in range(N_SLOTS):
        kw = dict(depth=_dev(d[s]), depth_weight=_dev(w[s]) if weights else None) if depths else {}
        st.add_u8(torch.from_numpy(f[s]), torch.from_numpy(mk[s]) if masks else None, **kw)
    return cam, st, torch.zeros(3, device=gpu())


def _model():
    m, _cam = scene_model("a")
    m.training_setup()
    return m


def _depth_of(st, j, level):
    t = st.depth_target(j, level)
    return t if st.has_depth_weights else (t, None)


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("use_graph", [False, True])
def test_graphed_step_on_a_depth_store_equals_the_step_given_the_decoded_tensors(use_graph, level, weights):
    from gaussian_lic_amd import trainer
    cam, st, bg = _step_setup(weights)
    a, b = _model(), _model()
    start = model_state(a)
    lcam = cam.at_level(level)
    d0, w0 = _depth_of(st, 0, level)
    ga = trainer.GraphedStep(a, cam, None, bg, use_graph=use_graph, keyframes=st, frame=0, level=level, lambda_depth=LAMBDA_D, depth_huber=HUBER)
    gb = trainer.GraphedStep(b, lcam, st.target(0, level), bg, use_graph=use_graph, gt_depth=d0, lambda_depth=LAMBDA_D, depth_weight=w0, depth_huber=HUBER)
    assert ga.use_depth and ga._kf_depth and (ga.depth_weight is not None) == weights and tuple(ga.gt_depth.shape) == (lcam.image_height, lcam.image_width)
    assert_same_state(start, model_state(a))                                 # building the step (warm-up, capture) left the map as it was
    for j in FRAMES_ORDER:
        dj, wj = _depth_of(st, j, level)
        ta = ga.step(cam, frame=j).clone()
        tb = gb.step(lcam, st.target(j, level), gt_depth=dj, depth_weight=wj).clone()
        assert ta.numel() == 3 and torch.equal(bits(ta), bits(tb)), j
        assert torch.equal(bits(ga.gt_depth), bits(dj)) and (not weights or torch.equal(bits(ga.depth_weight), bits(wj))), j
        assert int((dj > 0).sum()) > 100
    assert ga.check() == 0 and gb.check() == 0
    assert_same_state(model_state(a), model_state(b))
    assert not torch.equal(model_state(a)["xyz"], start["xyz"])              # the map moved
    ta, tb = ga.step().clone(), gb.step().clone()                            # the same frame again without naming it: the loaded word stays
    assert torch.equal(bits(ta), bits(tb))


def test_graphed_step_on_a_depth_store_trains_poses():
    from gaussian_lic_amd import trainer
    cam, st, bg = _step_setup(True)
    a, b = _model(), _model()
    pa, pb = (trainer.PoseSet(2, cam, gpu(), lr_trans=2e-3, lr_rot=1e-3) for _ in range(2))
    d0, w0 = _depth_of(st, 0, 0)
    ga = trainer.GraphedStep(a, cam, None, bg, keyframes=st, frame=0, lambda_depth=LAMBDA_D, depth_huber=HUBER, poses=pa, view=0, train_pose=True)
    gb = trainer.GraphedStep(b, cam, st.target(0), bg, gt_depth=d0, lambda_depth=LAMBDA_D, depth_weight=w0, depth_huber=HUBER, poses=pb, view=0,
                             train_pose=True)
    for k, j in enumerate(FRAMES_ORDER):
        dj, wj = _depth_of(st, j, 0)
        ta = ga.step(frame=j, view=k % 2).clone()
        tb = gb.step(gt_image=st.target(j), gt_depth=dj, depth_weight=wj, view=k % 2).clone()
        assert torch.equal(bits(ta), bits(tb)), j
    assert ga.check() == 0 and gb.check() == 0
    assert_same_state(model_state(a), model_state(b))
    for name in ("view", "proj", "campos", "m", "v", "steps"):
        assert torch.equal(getattr(pa, name), getattr(pb, name)), name
    assert not torch.equal(pa.view[0], trainer.PoseSet(2, cam, gpu()).view[0])   # the pose moved


def test_the_recorded_call_lists():
    from gaussian_lic_amd import _lib, trainer
    cam, st, bg = _step_setup(True)
    _cam, nodepth, _bg = _step_setup(False, depths=False)
    d1, w1 = _depth_of(st, 1, 0)
    given = trainer.GraphedStep(_model(), cam, st.target(1), bg, gt_depth=d1, lambda_depth=LAMBDA_D, depth_weight=w1, depth_huber=HUBER)
    keyed = trainer.GraphedStep(_model(), cam, None, bg, keyframes=st, frame=1, lambda_depth=LAMBDA_D, depth_huber=HUBER)
    colour = trainer.GraphedStep(_model(), cam, None, bg, keyframes=st, frame=1)                                  # lambda_depth == 0
    plain = trainer.GraphedStep(_model(), cam, None, bg, keyframes=nodepth, frame=1, gt_depth=d1, lambda_depth=LAMBDA_D)   # a store without depths
    bare = trainer.GraphedStep(_model(), cam, st.target(1), bg, gt_depth=d1, lambda_depth=LAMBDA_D)                        # ... and no store at all
    real = _lib.lib()
    rec = _Calls(real)
    _lib._lib = rec
    lists = []
    try:
        for run in (lambda: given.step(cam, st.target(2), gt_depth=d1, depth_weight=w1), lambda: keyed.step(cam, frame=2), lambda: colour.step(cam, frame=2),
                    lambda: plain.step(cam, frame=2, gt_depth=d1), lambda: bare.step(cam, gt_depth=d1)):
            rec.names.clear()
            run()
            lists.append([n for n in rec.names])
    finally:
        _lib._lib = real
    print(lists)
    tensors, on_store, no_lambda, no_depths, no_store = lists
    tensors = [n for n in tensors if n != "gslic_keyframe_decode"]            # (st.target(2) of the first run is the test's own call)
    assert tensors[0] == "gslic_rasterize_forward_depth_capacity" and tensors[-1] == "gslic_rasterize_backward_depth_adam"
    assert "gslic_depth_loss_weighted_forward_backward" in tensors
    assert on_store == ["gslic_keyframe_decode", "gslic_keyframe_decode_depth"] + tensors
    today = ["gslic_keyframe_decode", "gslic_rasterize_forward_capacity", "gslic_l1_ssim_loss_forward_backward", "gslic_rasterize_backward_adam"]
    assert no_lambda == today and "gslic_keyframe_decode_depth" not in no_lambda
    assert no_store[0] == "gslic_rasterize_forward_depth_capacity" and "gslic_depth_l1_loss_forward_backward" in no_store
    assert no_depths == ["gslic_keyframe_decode"] + no_store                 # a store without depths under gt_depth=: today's depth step


def test_graphed_step_refusals_and_the_stale_depth_repeat():
    from gaussian_lic_amd import trainer
    cam, st, bg = _step_setup(True)
    _cam, unweighted, _bg = _step_setup(False)
    m = _model()
    d0, w0 = _depth_of(st, 0, 0)
    kw = dict(keyframes=st, frame=0, lambda_depth=LAMBDA_D)
    with pytest.raises(ValueError, match="gt_depth given together with a keyframe store that has depths"):
        trainer.GraphedStep(m, cam, None, bg, gt_depth=d0, **kw)
    with pytest.raises(ValueError, match="depth_weight given together with a keyframe store that has depth weights"):
        trainer.GraphedStep(m, cam, None, bg, depth_weight=w0, **kw)
    gs = trainer.GraphedStep(m, cam, None, bg, **kw)
    with pytest.raises(ValueError, match="gt_depth given to a step whose keyframe store has depths"):
        gs.step(cam, frame=1, gt_depth=d0)
    with pytest.raises(ValueError, match="depth_weight given to a step whose keyframe store has depth weights"):
        gs.step(cam, frame=1, depth_weight=w0)
    # a depth store WITHOUT depth weights takes depth_weight= from the host as ever: the step equals the one given all three tensors
    a, b = _model(), _model()
    du = unweighted.depth_target(1)
    ga = trainer.GraphedStep(a, cam, None, bg, keyframes=unweighted, frame=1, lambda_depth=LAMBDA_D, depth_weight=w0)
    gb = trainer.GraphedStep(b, cam, unweighted.target(1), bg, gt_depth=du, lambda_depth=LAMBDA_D, depth_weight=w0)
    w2 = _depth_of(st, 2, 0)[1]
    ta, tb = ga.step(cam, frame=1, depth_weight=w2).clone(), gb.step(cam, depth_weight=w2).clone()
    assert torch.equal(bits(ta), bits(tb))
    assert_same_state(model_state(a), model_state(b))
    # lambda_depth == 0 on a depth store, and a store without depths, still take gt_depth= tensors
    trainer.GraphedStep(_model(), cam, None, bg, keyframes=st, frame=0, gt_depth=d0).step(cam, frame=1)
    # capacities too small for the scene: every step is a no-op until check() grows the buffers and repeats it on ITS frame's depth
    a, b = _model(), _model()
    small = max(64, raw_forward(a, cam, depth=True).state[0] // 2)            # half the instances the view has
    ga = trainer.GraphedStep(a, cam, None, bg, cap_R=small, check_every=0, keyframes=st, frame=0, lambda_depth=LAMBDA_D, depth_huber=HUBER)
    for j in (2, 1):
        ga.step(cam, frame=j)
    assert ga.check() == 2
    for j in (2, 1):
        dj, wj = _depth_of(st, j, 0)
        trainer.training_step_fused(b, cam, st.target(j), bg, gt_depth=dj, lambda_depth=LAMBDA_D, depth_weight=wj, depth_huber=HUBER)
    assert_same_state(model_state(a), model_state(b))                        # the repeats ran on frames 2 and 1, in that order
    # a depth replaced after its step was issued: the repeat fails loudly
    ga = trainer.GraphedStep(_model(), cam, None, bg, cap_R=small, check_every=0, keyframes=st, frame=0, lambda_depth=LAMBDA_D)
    ga.step(cam, frame=1)
    st.put_depth(1, d0)
    with pytest.raises(RuntimeError, match="was replaced"):
        ga.check()


# ---------------------------------------------------------------------------------------------------- the C++ host
P_, W_, H_, DEG = 1536, 160, 120, 3


@pytest.mark.parametrize("level,level2,slot,weights", [(0, 2, 0, False), (1, 0, 1, True)])
def test_keyframe_depth_store_cpp_host(tmp_path, level, level2, slot, weights):
    """gslic::KeyframeStore with depths issues the C-ABI calls of trainer.KeyframeStore: the slabs, the decoded depth (and weight) at two levels,
    the step's terms and the 19 row arrays after one FusedStep::step on the targets are bit-identical to the Python host's."""
    from gaussian_lic_amd import trainer
    exe = fio.build("fused_keyframe_depth")
    raw, sc, camd, cam = make_scene("random", P_, W_, H_, DEG, 5)
    lcam = cam.at_level(level).to_device(gpu())
    f, _mk = kref.random_frames(N_SLOTS, W_, H_, 60)
    d, w = ref.random_depth_frames(N_SLOTS + 1, W_, H_, 61)
    d = np.where(d > 0, np.float32(1.0) + d * np.float32(0.05), d).astype(np.float32)
    dd = str(tmp_path)
    fio.write_inputs(dd, raw, lcam, scalars_extra=(LAMBDA_D, HUBER, STEP), depths=d[:N_SLOTS], late=d[N_SLOTS])
    f.tofile(dd + "/frames.u8")
    if weights:
        fio.write(dd, "dweights", w[:N_SLOTS])
    fio.run(exe, dd, str(P_), str(W_), str(H_), str(DEG), str(level), str(level2), str(slot), str(N_SLOTS), str(int(weights)))
    st = trainer.KeyframeStore(W_, H_, N_SLOTS, gpu(), depths=True, depth_weights=weights)
    for s in range(N_SLOTS - 1):
        st.add_u8(torch.from_numpy(f[s]), depth=_dev(d[s]), depth_weight=_dev(w[s]) if weights else None)
    st.add_u8(torch.from_numpy(f[N_SLOTS - 1]))
    st.put_depth(0, _dev(d[N_SLOTS]))
    assert np.array_equal(np.fromfile(dd + "/out_depth_slab.u16", np.uint16), _codes(st).reshape(-1)) and not _codes(st, N_SLOTS - 1).any()
    assert np.array_equal(_codes(st, 0), ref.encode(d[N_SLOTS]))
    if weights:
        assert np.array_equal(np.fromfile(dd + "/out_dweight_slab.u8", np.uint8), st.dweight.cpu().numpy().reshape(-1)) and int(st.dweight[0].min()) == 255
    for tag, l in (("", level), ("2", level2)):
        dep, wgt = _depth_of(st, slot, l)
        assert torch.equal(fio.read(dd, f"depth{tag}.f32", np.int32), bits(dep.cpu()).reshape(-1)), l
        if weights:
            assert torch.equal(fio.read(dd, f"dweight{tag}.f32", np.int32), bits(wgt.cpu()).reshape(-1)), l
    dep, wgt = _depth_of(st, slot, level)
    model = training_model(raw)
    terms = trainer.training_step_fused(model, lcam, st.target(slot, level), torch.zeros(3, device=gpu()), gt_depth=dep, lambda_depth=LAMBDA_D,
                                        depth_weight=wgt, depth_huber=HUBER)[0]
    assert torch.equal(fio.read(dd, "terms.f32", np.int32), bits(terms.cpu()).reshape(-1))
    rows = fio.read_rows(dd, 15)
    for name, p in [("xyz", model.xyz), ("scaling", model.scaling), ("rotation", model.rotation), ("opacity", model.opacity), ("dc", model.features_dc),
                    ("rest", model.features_rest)]:
        full = "features_" + name if name in ("dc", "rest") else name
        assert torch.equal(rows[name], bits(p.detach().cpu()).reshape(-1)), name
        assert torch.equal(rows["m_" + name], bits(model._m[full][:model.P].cpu()).reshape(-1)), "m_" + name
        assert torch.equal(rows["v_" + name], bits(model._v[full][:model.P].cpu()).reshape(-1)), "v_" + name
