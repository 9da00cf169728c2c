"""-m gpu: the keyframe store — the decode and encode kernels (gslic_keyframe_decode / gslic_keyframe_encode) against the numpy restatement of their
rules (tests/keyframe_ref.py) bit for bit, the frame word, Camera.at_level against the library's LiDAR range images, and the store through
GraphedStep (eager and captured) and the C++ host.  Bit comparisons: no tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch

import fused_check_io as fio
import keyframe_ref as ref
from conftest import make_scene
from gpu_helpers import SENTINEL, assert_same_state, bits, gpu, guarded, guards_intact, model_state, raw_forward, scene_model, training_model

pytestmark = pytest.mark.gpu

# (4,1) and (64,2): W % (4 << l) == 0, a lane owns four pixels (level 0, and level 1 of 64 x 2); every other width takes the one-pixel path;
# (130,33): more than one workgroup on either path, remainders at every level
SHAPES = [(4, 1), (5, 3), (7, 5), (64, 2), (67, 9), (130, 33)]
N_SLOTS = 3


def _L():
    from gaussian_lic_amd import _lib
    return _lib


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu())


@functools.lru_cache(maxsize=None)
def _frames(W, H, kind):
    """Three frames and masks of a shape, and every level's reference, computed once and left unchanged.  kind: "random", "zeros" (all 0), "ones"
    (all 255)."""
    if kind == "random":
        f, m = ref.random_frames(N_SLOTS, W, H, 1000 * H + W, masks=True)
    else:
        v = 0 if kind == "zeros" else 255
        f, m = np.full((N_SLOTS, H, W, 3), v, np.uint8), np.full((N_SLOTS, H, W), v, np.uint8)
    levels = ref.levels(W, H, top=3)
    want = {(s, l): (ref.decode(f[s], l), ref.decode(m[s], l)) for s in range(N_SLOTS) for l in levels}
    return f, m, levels, want


def _store(W, H, f, m=None, capacity=N_SLOTS):
    from gaussian_lic_amd import trainer
    st = trainer.KeyframeStore(W, H, capacity, gpu(), masks=m is not None)
    for s in range(f.shape[0]):
        assert st.add_u8(torch.from_numpy(f[s]), None if m is None else torch.from_numpy(m[s])) == s
    return st


def _guarded_target(Wl, Hl, masks):
    ib, iw = guarded(3 * Hl * Wl)
    wb, ww = guarded(Hl * Wl) if masks else (None, None)
    return ib, iw.view(torch.float32).view(3, Hl, Wl), wb, (ww.view(torch.float32).view(Hl, Wl) if masks else None)


# ---------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("masks", [False, True])
@pytest.mark.parametrize("W,H", SHAPES)
def test_decode_is_the_rule_bit_for_bit(W, H, masks):
    for kind in ("random", "zeros", "ones"):
        f, m, levels, want = _frames(W, H, kind)
        st = _store(W, H, f, m if masks else None)
        assert st.n == N_SLOTS and st.nbytes == N_SLOTS * H * W * (4 if masks else 3)
        slab = (st.color.clone(), st.mask.clone() if masks else None)
        for l in levels:
            Wl, Hl = ref.level_size(W, H, l)
            for s in (0, N_SLOTS - 1):
                ib, img, wb, wgt = _guarded_target(Wl, Hl, masks)
                got = st.target(s, l, out=(img, wgt) if masks else img)
                assert (got[0] if masks else got) is img
                assert np.array_equal(img.cpu().numpy().view(np.int32), want[(s, l)][0].view(np.int32)), (kind, l, s)
                assert guards_intact(ib, 3 * Hl * Wl)
                if masks:
                    assert np.array_equal(wgt.cpu().numpy().view(np.int32), want[(s, l)][1].view(np.int32)), (kind, l, s)
                    assert guards_intact(wb, Hl * Wl)
        assert torch.equal(st.color, slab[0]) and (not masks or torch.equal(st.mask, slab[1]))   # a decode writes no slot
        if kind == "ones":   # a full block of 255 decodes to d(255) at every level: the scaling is exact
            assert all(torch.equal(bits(st.target(0, l)[0] if masks else st.target(0, l)), bits(torch.full((3, H >> l, W >> l), float(ref.C0 * np.float32(255)), device=gpu())))
                       for l in levels)


def test_shapes_reach_both_paths_and_more_than_one_workgroup():
    fast = [(W, H, l) for W, H in SHAPES for l in ref.levels(W, H, 3) if W % (4 << l) == 0]
    slow = [(W, H, l) for W, H in SHAPES for l in ref.levels(W, H, 3) if W % (4 << l) != 0]
    assert (4, 1, 0) in fast and (64, 2, 1) in fast and (5, 3, 0) in slow and {l for _w, _h, l in slow} == {0, 1, 2, 3}
    assert 130 * 33 > 256 and (130 >> 1) * (33 >> 1) > 256 and 64 * 2 // 4 < 256   # KF_THREADS = 256 pixels (groups) per workgroup
    assert any(W % (1 << l) and H % (1 << l) for W, H, l in slow)                 # remainder columns and rows together


def test_a_wide_image_on_the_four_pixel_path_at_every_level():
    """512 x 24: W % (4 << l) == 0 up to level 4 — the 4-, 8- and 16-byte loads and several source rows per lane — on more than one workgroup."""
    W, H = 512, 24
    f, m = ref.random_frames(2, W, H, 77, masks=True)
    st = _store(W, H, f, m, capacity=2)
    for l in range(5):
        img, wgt = st.target(1, l)
        assert np.array_equal(img.cpu().numpy().view(np.int32), ref.decode(f[1], l).view(np.int32)), l
        assert np.array_equal(wgt.cpu().numpy().view(np.int32), ref.decode(m[1], l).view(np.int32)), l


def test_encode_is_the_rule_on_the_edge_values_and_leaves_the_other_slots():
    from gaussian_lic_amd import trainer
    W, H = 67, 9
    vals, want = ref.edge_values()
    rng = np.random.default_rng(4)
    img = rng.uniform(-0.2, 1.2, (3, H, W)).astype(np.float32)
    msk = rng.uniform(-0.2, 1.2, (H, W)).astype(np.float32)
    assert vals.size >= 3 * H * W                                        # more edge values than the image holds: two images take them all
    f, m = ref.random_frames(N_SLOTS, W, H, 9, masks=True)
    for half in (0, 1):
        st = _store(W, H, f, m)
        chunk = vals[half * 3 * H * W:(half + 1) * 3 * H * W]
        at = rng.permutation(3 * H * W)[:chunk.size]
        img.reshape(-1)[at] = chunk
        if half:
            msk = np.resize(vals[::-1], H * W).reshape(H, W).astype(np.float32)   # the mask takes the edge values too
        before = (st.color.clone(), st.mask.clone())
        assert st.put(1, image=_dev(img), mask=_dev(msk)) == 1 and st.serial(1) == 1 and st.serial(0) == 0
        assert np.array_equal(st.color[1].cpu().numpy(), ref.encode(img)) and np.array_equal(st.mask[1].cpu().numpy(), ref.encode(msk))
        got = st.color[1].cpu().numpy().transpose(2, 0, 1).reshape(-1)[at]
        assert np.array_equal(got, want[half * 3 * H * W:half * 3 * H * W + chunk.size])   # ... and the exact-arithmetic expectation of every edge value
        for s in (0, 2):
            assert torch.equal(st.color[s], before[0][s]) and torch.equal(st.mask[s], before[1][s])
    # the four-pixel path of the encode (H * W % 4 == 0) gives the same bytes
    W4, H4 = 64, 2
    x = np.resize(vals, 3 * H4 * W4).reshape(3, H4, W4).astype(np.float32)
    st = trainer.KeyframeStore(W4, H4, 2, gpu(), masks=True)
    st.add(_dev(np.zeros_like(x)))
    assert st.add(_dev(x), _dev(x[1])) == 1
    assert np.array_equal(st.color[1].cpu().numpy(), ref.encode(x)) and np.array_equal(st.mask[1].cpu().numpy(), ref.encode(x[1]))
    assert int(st.color[0].max()) == 0 and int(st.mask[0].min()) == 255   # a slot added without a mask weighs every pixel 1


def test_add_then_target_is_the_rounded_value_by_the_rule():
    from gaussian_lic_amd import trainer
    W, H = 67, 9
    x = np.random.default_rng(12).uniform(0.0, 1.0, (3, H, W)).astype(np.float32)
    x.reshape(-1)[:256] = np.arange(256, dtype=np.float32) * ref.C0                       # every decoded value comes back as itself
    x.reshape(-1)[256:512] = np.arange(256, dtype=np.float32) / np.float32(255.0)         # ... and so does every float32 quotient v / 255
    st = trainer.KeyframeStore(W, H, 1, gpu())
    got = st.target(st.add(_dev(x))).cpu().numpy()
    want = ref.decode(ref.encode(x))
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    d = (np.arange(256, dtype=np.float32) * ref.C0).view(np.int32)
    assert np.array_equal(got.reshape(-1)[:256].view(np.int32), d) and np.array_equal(got.reshape(-1)[256:512].view(np.int32), d)
    assert float(np.abs(got.astype(np.float64) - x.astype(np.float64)).max()) <= 0.5 / 255 + 2.0 ** -24   # half a level, and the rounding of x * 255
    with pytest.raises(RuntimeError, match="slots are filled"):
        st.add(_dev(x))
    with pytest.raises(IndexError):
        st.target(1)
    with pytest.raises(ValueError, match="no level"):
        st.target(0, 4)


@pytest.mark.parametrize("W,H,level", [(64, 2, 0), (67, 9, 1)])
def test_a_frame_word_out_of_range_writes_nothing(W, H, level):
    f, m, _levels, _want = _frames(W, H, "random")
    st = _store(W, H, f, m)
    Wl, Hl = ref.level_size(W, H, level)
    for word in (-1, N_SLOTS, 2 ** 31 - 1):
        ib, img, wb, wgt = _guarded_target(Wl, Hl, True)
        st._decode(torch.tensor([word], dtype=torch.int32, device=gpu()), level, img, wgt)
        torch.cuda.synchronize()
        assert bool((ib == SENTINEL).all()) and bool((wb == SENTINEL).all()), word
    ib, img, wb, wgt = _guarded_target(Wl, Hl, True)                     # the last valid word writes
    st._decode(torch.tensor([N_SLOTS - 1], dtype=torch.int32, device=gpu()), level, img, wgt)
    assert np.array_equal(img.cpu().numpy().view(np.int32), ref.decode(f[N_SLOTS - 1], level).view(np.int32)) and guards_intact(ib, 3 * Hl * Wl)


def test_add_u8_takes_bgr_and_host_tensors():
    W, H = 7, 5
    f, _m = ref.random_frames(2, W, H, 21)
    st = _store(W, H, f[:1], capacity=2)
    assert st.add_u8(torch.from_numpy(f[1][:, :, ::-1].copy()), bgr=True) == 1
    assert np.array_equal(st.color[1].cpu().numpy(), f[1])
    with pytest.raises(ValueError, match="without masks"):
        st.put(0, u8=torch.from_numpy(f[0]), mask=torch.zeros(H, W, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        st.put(0, u8=torch.zeros(H, W, 3))


# ---------------------------------------------------------------------------------------------------- the camera rule and the range images
@pytest.mark.parametrize("level", [1, 2])
def test_lidar_image_of_the_level_camera_is_the_positive_minimum_pool(level):
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.camera import synthetic_camera
    W, H = 64, 48
    cam = synthetic_camera(W, H, "se3_c").to_device(gpu())
    rng = np.random.default_rng(30 + level)
    pts = np.concatenate([rng.uniform(-4, 4, (6000, 2)), rng.uniform(0.5, 8.0, (6000, 1))], axis=1).astype(np.float32)
    pts = _dev(pts @ cam.R_wc.T.astype(np.float32) + cam.t_wc.astype(np.float32))   # camera-frame points moved into the world
    full = trainer.lidar_depth_image(cam, pts)
    low = trainer.lidar_depth_image(cam.at_level(level), pts)
    want = ref.positive_min_pool(full.cpu().numpy(), level)
    assert tuple(low.shape) == (H >> level, W >> level) and int((want > 0).sum()) > 100
    assert np.array_equal(low.cpu().numpy().view(np.int32), want.view(np.int32))


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


def _step_setup(masks):
    m, cam = scene_model("a")
    W, H = cam.image_width, cam.image_height
    f, mk = ref.random_frames(N_SLOTS, W, H, 50, masks=True)
    return cam, _store(W, H, f, mk if masks else None), torch.zeros(3, device=gpu())


def _model():
    m, _cam = scene_model("a")
    m.training_setup()
    return m


@pytest.mark.parametrize("masks", [False, True])
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("use_graph", [False, True])
def test_graphed_step_on_a_store_equals_the_step_given_the_decoded_target(use_graph, level, masks):
    from gaussian_lic_amd import trainer
    cam, st, bg = _step_setup(masks)
    a, b = _model(), _model()
    start = model_state(a)
    lcam = cam.at_level(level)
    first = st.target(0, level)
    kw = dict(weight=first[1]) if masks else {}
    ga = trainer.GraphedStep(a, cam, None, bg, use_graph=use_graph, keyframes=st, frame=0, level=level)
    gb = trainer.GraphedStep(b, lcam, first[0] if masks else first, bg, use_graph=use_graph, **kw)
    assert (ga.W, ga.H) == (lcam.image_width, lcam.image_height) and ga.use_weight == masks
    assert_same_state(start, model_state(a))                                 # building the step (warm-up, capture) left the map as it was
    for j in FRAMES_ORDER:
        t = st.target(j, level)
        ta = ga.step(cam if j != 1 else lcam, frame=j).clone()              # a full-size camera and one of the level's size are the same step
        tb = (gb.step(lcam, t[0], weight=t[1]) if masks else gb.step(lcam, t)).clone()
        assert torch.equal(bits(ta), bits(tb)), j
        assert torch.equal(bits(ga.gt), bits(t[0] if masks else t)) and (not masks or torch.equal(bits(ga.weight), bits(t[1])))
    assert ga.check() == 0 and gb.check() == 0
    assert_same_state(model_state(a), model_state(b))
    moved = model_state(a)
    assert not torch.equal(moved["xyz"], start["xyz"])
    # the same frame again without naming it: the loaded word stays
    ta, tb = ga.step().clone(), gb.step().clone()
    assert torch.equal(bits(ta), bits(tb))


def test_graphed_step_refusals_and_the_stale_slot_repeat():
    from gaussian_lic_amd import trainer
    cam, st, bg = _step_setup(True)
    m = _model()
    gt = st.target(0)[0]
    with pytest.raises(ValueError, match="together with keyframes"):
        trainer.GraphedStep(m, cam, gt, bg, keyframes=st, frame=0)
    with pytest.raises(ValueError, match="without keyframes"):
        trainer.GraphedStep(m, cam, gt, bg, frame=0)
    with pytest.raises(ValueError, match="has masks"):
        trainer.GraphedStep(m, cam, None, bg, keyframes=st, frame=0, weight=st.target(0)[1])
    with pytest.raises(IndexError):
        trainer.GraphedStep(m, cam, None, bg, keyframes=st, frame=N_SLOTS)
    plain = trainer.GraphedStep(m, cam, gt, bg)
    with pytest.raises(ValueError, match="built without a keyframe store"):
        plain.step(cam, frame=1)
    # capacities too small for the scene: every step is a no-op until check() grows the buffers and repeats it on ITS frame
    a, b = _model(), _model()
    small = max(64, raw_forward(a, cam).state[0] // 2)                       # half the instances the view has
    ga = trainer.GraphedStep(a, cam, None, bg, keyframes=st, frame=0, cap_R=small, check_every=0)
    with pytest.raises(ValueError, match="built on a keyframe store"):
        ga.step(cam, gt, frame=1)
    with pytest.raises(IndexError):
        ga.step(cam, frame=N_SLOTS)
    for j in (2, 1):
        ga.step(cam, frame=j)
    assert ga.check() == 2
    for j in (2, 1):
        t = st.target(j)
        trainer.training_step_fused(b, cam, t[0], bg, weight=t[1])
    assert_same_state(model_state(a), model_state(b))                        # the repeats ran on frames 2 and 1, in that order
    # a slot replaced after its step was issued: the repeat fails loudly
    ga = trainer.GraphedStep(_model(), cam, None, bg, keyframes=st, frame=0, cap_R=small, check_every=0)
    ga.step(cam, frame=1)
    st.put(1, u8=st.color[2])
    with pytest.raises(RuntimeError, match="was replaced"):
        ga.check()


def test_a_step_without_keyframes_issues_the_calls_it_always_did():
    from gaussian_lic_amd import _lib, trainer
    cam, st, bg = _step_setup(False)
    gt = st.target(1)
    plain = trainer.GraphedStep(_model(), cam, gt, bg)
    keyed = trainer.GraphedStep(_model(), cam, None, bg, keyframes=st, frame=1)
    real = _lib.lib()
    rec = _Calls(real)
    _lib._lib = rec
    try:
        plain.step(cam, gt)
        n = len(rec.names)
        keyed.step(cam, frame=2)
    finally:
        _lib._lib = real
    first, second = rec.names[:n], rec.names[n:]
    print("plain step:", first, " step on a store:", second)
    # the parent's eager capacity-mode step: forward, the two-launch loss, the backward with Adam inside — and nothing of the store
    assert first == ["gslic_rasterize_forward_capacity", "gslic_l1_ssim_loss_forward_backward", "gslic_rasterize_backward_adam"]
    assert second == ["gslic_keyframe_decode"] + first


# ---------------------------------------------------------------------------------------------------- the C++ host
P_, W_, H_, DEG = 1536, 160, 120, 3


@pytest.mark.parametrize("level,slot,masks", [(0, 0, False), (1, 2, True)])
def test_keyframe_store_cpp_host(tmp_path, level, slot, masks):
    """gslic::KeyframeStore issues the C-ABI calls of trainer.KeyframeStore: the re-encoded slot, the decoded target (and weight), the step's terms
    and the 19 row arrays after one FusedStep::step on the target are bit-identical to the Python host's."""
    from gaussian_lic_amd import trainer
    exe = fio.build("fused_keyframe")
    raw, sc, camd, cam = make_scene("random", P_, W_, H_, DEG, 5)
    lcam = cam.at_level(level).to_device(gpu())
    f, mk = ref.random_frames(N_SLOTS, W_, H_, 60, masks=True)
    image = np.random.default_rng(61).uniform(-0.1, 1.1, (3, H_, W_)).astype(np.float32)
    d = str(tmp_path)
    fio.write_inputs(d, raw, lcam, image=image)
    f.tofile(d + "/frames.u8")
    if masks:
        mk.tofile(d + "/masks.u8")
    fio.run(exe, d, str(P_), str(W_), str(H_), str(DEG), str(level), str(slot), str(N_SLOTS), str(int(masks)))
    st = _store(W_, H_, f, mk if masks else None)
    st.put(0, image=_dev(image))
    assert np.array_equal(np.fromfile(d + "/out_slot0.u8", np.uint8), st.color[0].cpu().numpy().reshape(-1))
    assert np.array_equal(st.color[0].cpu().numpy(), ref.encode(image))
    t = st.target(slot, level)
    img, wgt = t if masks else (t, None)
    assert torch.equal(fio.read(d, "target.f32", np.int32), bits(img.cpu()).reshape(-1))
    if masks:
        assert torch.equal(fio.read(d, "weight.f32", np.int32), bits(wgt.cpu()).reshape(-1))
    model = training_model(raw)
    terms = trainer.training_step_fused(model, lcam, img, torch.zeros(3, device=gpu()), weight=wgt)[0]
    assert torch.equal(fio.read(d, "terms.f32", np.int32), bits(terms.cpu()).reshape(-1))
    rows = fio.read_rows(d, 15)
    for name, p in [("xyz", model.xyz), ("scaling", model.scaling), ("rotation", model.rotation), ("opacity", model.opacity), ("dc", model.features_dc),
                    ("rest", model.features_rest)]:
        full = "features_" + name if name in ("dc", "rest") else name
        assert torch.equal(rows[name], bits(p.detach().cpu()).reshape(-1)), name
        assert torch.equal(rows["m_" + name], bits(model._m[full][:model.P].cpu()).reshape(-1)), "m_" + name
        assert torch.equal(rows["v_" + name], bits(model._v[full][:model.P].cpu()).reshape(-1)), "v_" + name
