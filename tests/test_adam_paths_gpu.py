"""-m gpu: every path that applies the masked Adam — adam.hip's float4 body, scalar tail, unaligned fallback, runtime row width, grid-stride
second trip and ninth-and-later groups; SparseGaussianAdam.step(rows=, grad_addr=); gslic_sh_grad_from_rgb_adam; gslic_sh_grad_from_rgb_adam_all;
the update inside the per-Gaussian backward — against tests/adam_ref.py on the same inputs, on BITS (.view(np.uint32)) of param, exp_avg and
exp_avg_sq.  The inputs come from tests/adam_cases.py; tests/test_adam_ref_cpu.py has checked on the CPU that none of them reaches below 2^-126.

Buffers of the adam.hip cases are carved out of larger allocations: 64 guard words in front and behind, filled with one NaN payload, that must
come back unchanged (a float4 store past a tail or from an unaligned base lands there), and 64 guard bytes of 1 around the visibility bytes (a
wrong row index then reads "visible" and an element moves that the reference keeps).  The models of cases (g) - (j) carry 64 spare rows of that
payload behind every parameter and moment array."""
import ctypes

import numpy as np
import pytest
import torch

import adam_cases as ac
from adam_ref import adam_ref, same_bits

pytestmark = pytest.mark.gpu

G = 64                      # guard words / bytes on either side
PAYLOAD = 0x7FC5A5A5        # a quiet NaN no kernel computes
NAMES = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")


def _dev():
    return torch.device("cuda:0")


class Carved:
    """float32 data at `off` floats past a 16-byte-aligned address, between guard words."""

    def __init__(self, data, off=0):
        data = np.ascontiguousarray(data, np.float32)
        self.shape, self.n, self.start = data.shape, data.size, G + off
        host = np.full(self.start + self.n + G + 4, PAYLOAD, np.uint32)
        host[self.start:self.start + self.n] = data.reshape(-1).view(np.uint32)
        self.host = host
        self.dev = torch.from_numpy(host.view(np.int32)).to(_dev())
        assert self.dev.data_ptr() % 16 == 0
        self.ptr = self.dev.data_ptr() + 4 * self.start
        assert (self.ptr % 16 != 0) == (off % 4 != 0)

    def result(self, what):
        back = self.dev.cpu().numpy().view(np.uint32)
        inside = np.zeros(back.size, bool)
        inside[self.start:self.start + self.n] = True
        assert (back[~inside] == PAYLOAD).all(), f"{what}: a guard word was written"
        return back[inside].view(np.float32).reshape(self.shape)

    def unchanged(self, what):
        assert np.array_equal(self.dev.cpu().numpy().view(np.uint32), self.host), f"{what} was written"


class CarvedBytes:
    def __init__(self, vis, guard=1):
        vis = np.ascontiguousarray(vis, np.uint8)
        self.host = np.concatenate([np.full(G, guard, np.uint8), vis, np.full(G, guard, np.uint8)])
        self.dev = torch.from_numpy(self.host.copy()).to(_dev())
        self.ptr = self.dev.data_ptr() + G
        self.n = vis.size

    def unchanged(self, what):
        assert np.array_equal(self.dev.cpu().numpy(), self.host), f"{what} was written"


def _assert_bits(got, ref, what):
    bad = ~same_bits(got, ref)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ from the reference, the first at flat index {int(np.flatnonzero(bad.ravel())[0])}"


def run_groups(groups, vis, N, single_entry=False):
    """groups: [(p, g, m, v, lr, (off_p, off_g, off_m, off_v))] through gslic_adam_update_groups (single_entry: the one group through
    gslic_adam_update), every buffer carved.  Returns [(p', m', v')]; guards, gradients and visibility bytes are checked here."""
    from gaussian_lic_amd import _lib
    L = _lib.lib()
    bufs, descs = [], []
    for p, g, m, v, lr, offs in groups:
        c = [Carved(x, o) for x, o in zip((p, g, m, v), offs)]
        bufs.append(c)
        descs.append(_lib.AdamGroup(c[0].ptr, c[1].ptr, c[2].ptr, c[3].ptr, lr, p.shape[1]))
    cv = CarvedBytes(vis)
    vp = ctypes.c_void_p
    if single_entry:
        (c, d), = zip(bufs, descs)
        _lib.check(L.gslic_adam_update(vp(c[0].ptr), vp(c[1].ptr), vp(c[2].ptr), vp(c[3].ptr), vp(cv.ptr), d.lr, ac.B1, ac.B2, ac.EPS, N, d.M,
                                       _lib.current_stream_ptr()))
    else:
        arr = (_lib.AdamGroup * len(descs))(*descs)
        _lib.check(L.gslic_adam_update_groups(arr, len(descs), vp(cv.ptr), ac.B1, ac.B2, ac.EPS, N, _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    cv.unchanged("the visibility array")
    out = []
    for i, c in enumerate(bufs):
        c[1].unchanged(f"group {i}: the gradient")
        out.append(tuple(c[k].result(f"group {i}: {n}") for k, n in ((0, "param"), (2, "exp_avg"), (3, "exp_avg_sq"))))
    return out


def check_one(p, g, m, v, vis, lr=ac.LR, offs=(0, 0, 0, 0), single_entry=False, what=""):
    rp, rm, rv, sub = adam_ref(p, g, m, v, vis, lr, ac.B1, ac.B2, ac.EPS)
    assert not sub.any()
    (tp, tm, tv), = run_groups([(p, g, m, v, lr, offs)], vis, p.shape[0], single_entry)
    for got, ref, n in ((tp, rp, "param"), (tm, rm, "exp_avg"), (tv, rv, "exp_avg_sq")):
        _assert_bits(got, ref, f"{what} {n}")
    return tp, tm, tv


# ------------------------------------------------------------------------------------------------------------------------------------------------
# adam.hip

@pytest.mark.parametrize("which", ac.A_WHICH)
@pytest.mark.parametrize("N,M", ac.A_SHAPES)
def test_a_unaligned_bases(N, M, which):
    """One base, or all four, 1 / 2 / 3 floats past a 16-byte boundary: the scalar path for the whole group (2100 elements: the 256-thread
    stride loops more than once within a block's share, and several blocks run)."""
    t = ac.tensors(N, M, seed=N * 100 + M)
    for off in (1, 2, 3):
        check_one(*t, ac.mask(N, seed=N + M + off), offs=ac.a_offsets(which, off), what=f"{which} +{off}:")


@pytest.mark.parametrize("N,M", ac.B_SHAPES)
def test_b_tails_behind_an_aligned_base(N, M):
    """Every instantiation (M = 1, 3, 45, 4 and the runtime-M adam_span<0>) with N*M % 4 in {1, 2, 3} ((3, 4) and (9, 64): whole quads only),
    through the single-group entry point."""
    check_one(*ac.tensors(N, M, seed=N * 100 + M), ac.mask(N, seed=N + M), single_entry=True)


@pytest.mark.parametrize("pattern", ac.C_PATTERNS)
@pytest.mark.parametrize("M", ac.C_WIDTHS)
def test_c_quads_across_rows_of_different_visibility(M, pattern):
    vis = ac.vis_pattern(pattern, ac.C_N)
    p, g, m, v = ac.tensors(ac.C_N, M, seed=ac.C_N * 100 + M)
    tp, tm, tv = check_one(p, g, m, v, vis)
    keep = vis == 0
    for got, start in ((tp, p), (tm, m), (tv, v)):       # (what the reference says too: spelled out for the rows that must keep their bits)
        assert same_bits(got, start)[keep].all()


@pytest.mark.parametrize("N,M", ac.D_SHAPES)
def test_d_grid_stride_second_trip(N, M):
    """More than 8192 * 256 quads: the first blocks' threads loop twice ((186501, 45): with a scalar tail behind)."""
    check_one(*ac.tensors(N, M, seed=N * 100 + M), ac.mask(N, seed=N + M))


def test_e_eleven_groups_in_one_call():
    """Two launches of eight and three groups, each group with its own learning rate and width (M = 1 in a grid sized for M = 45), groups 2 and 9
    on unaligned bases."""
    vis = ac.mask(ac.E_N, seed=50)
    groups = ac.e_groups()
    refs = []
    for p, g, m, v, lr in groups:
        *r, sub = adam_ref(p, g, m, v, vis, lr, ac.B1, ac.B2, ac.EPS)
        assert not sub.any()
        refs.append(r)
    got = run_groups([grp + (ac.E_OFFSETS.get(i, (0, 0, 0, 0)),) for i, grp in enumerate(groups)], vis, ac.E_N)
    for i, (t, r) in enumerate(zip(got, refs)):
        for x, y, n in zip(t, r, ("param", "exp_avg", "exp_avg_sq")):
            _assert_bits(x, y, f"group {i} (M = {ac.E_WIDTHS[i]}) {n}")


@pytest.mark.parametrize("scale", ac.F_SCALES)
def test_f_value_edges(scale):
    """g = m = v = 0 (p keeps its bits), v = 0 with m != 0, -0.0 gradients, at magnitudes 1e-12, 1 and 1e4."""
    p, g, m, v = ac.f_tensors(scale)
    tp, _tm, _tv = check_one(p, g, m, v, np.ones(p.shape[0], np.uint8))
    assert same_bits(tp.ravel()[ac.F_ZERO], p.ravel()[ac.F_ZERO]).all()


def test_f_nan_and_inf_gradients_stay_in_their_element():
    p, g, m, v = ac.f_tensors(1.0, nonfinite=True)
    vis = np.ones(p.shape[0], np.uint8)
    rp, rm, rv, sub = adam_ref(p, g, m, v, vis, **ac.HYPER)
    assert not sub.any()
    (tp, tm, tv), = run_groups([(p, g, m, v, ac.LR, (0, 0, 0, 0))], vis, p.shape[0])
    for got, ref, n in ((tp, rp, "param"), (tm, rm, "exp_avg"), (tv, rv, "exp_avg_sq")):
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref)), n
        assert int((~np.isfinite(ref)).sum()) == 2
        clean = np.isfinite(ref)            # the other three scalars of both quads among them
        _assert_bits(got[clean], ref[clean], n)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the other three paths, on a model (single process, no collectives)

def _model(deg, P=ac.MODEL_P, W=96, H=64, seed=71):
    """A GaussianModel with 64 spare rows of PAYLOAD behind every array, seeded moments, its optimizer; also the camera."""
    from conftest import make_scene
    from gaussian_lic_amd import trainer
    raw, _sc, _camd, cam = make_scene("random", P, W, H, deg, seed)
    m = trainer.GaussianModel({k: (v.clone() if torch.is_tensor(v) else v) for k, v in raw.items()}, _dev(), capacity=P + G)
    m.training_setup()
    widths = tuple(getattr(m, n).numel() // P for n in NAMES)
    for n, mv in zip(NAMES, ac.moments(P, widths, 72)):
        for d, k in ((m._buf, None), (m._m, 0), (m._v, 1)):
            d[n][P:].view(torch.int32).fill_(PAYLOAD)
            if k is not None and mv is not None:
                d[n][:P].copy_(torch.from_numpy(mv[k]).view(d[n][:P].shape))
    return m, cam


def _state(m):
    """[(param, exp_avg, exp_avg_sq)] per group as numpy [P, M]; the spare rows are checked on the way."""
    P, out = m.P, []
    for i, n in enumerate(NAMES):
        for d in (m._buf, m._m, m._v):
            assert bool((d[n][P:].view(torch.int32) == PAYLOAD).all()), f"{n}: a row past P was written"
        st = m.optimizer.state[i]
        assert st["exp_avg"].data_ptr() == m._m[n].data_ptr() and getattr(m, n).data_ptr() == m._buf[n].data_ptr()
        out.append(tuple(t.detach().cpu().numpy().reshape(P, t.numel() // P).copy() for t in (getattr(m, n), st["exp_avg"], st["exp_avg_sq"])))
    return out


def _expect(start, grads, vis, opt, groups, skip_subnormal=False):
    """adam_ref per group of `groups` on the state `start`; the other groups unchanged.  Returns ([(p, m, v)], [comparable elements])."""
    out, ok = list(start), [np.ones(s[0].shape, bool) for s in start]
    for i in groups:
        p, m, v = start[i]
        if p.size == 0:
            continue
        rp, rm, rv, sub = adam_ref(p, grads[i].reshape(p.shape), m, v, vis, opt.lrs[i], opt.betas[0], opt.betas[1], opt.eps)
        if skip_subnormal:
            ok[i] = ~sub
        else:
            assert not sub.any()
        out[i] = (rp, rm, rv)
    return out, ok


def _assert_state(got, ref, what, ok=None):
    for i, (a, b) in enumerate(zip(got, ref)):
        for x, y, n in zip(a, b, ("param", "exp_avg", "exp_avg_sq")):
            sel = slice(None) if ok is None else ok[i]
            _assert_bits(x[sel], y[sel], f"{what}: {NAMES[i]} {n}")


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def test_g_chunked_small_groups_equal_the_whole_step():
    """step(only=[0, 3, 4, 5], rows=, grad_addr=) chunk by chunk, the gradients laid out as _ChunkedExchange lays them out — the last chunk has
    n = 37 rows, so its opacity / scaling / rotation gradients start 12 n, 16 n, 28 n bytes in: off 16-byte alignment — against step(grads) once
    and against the reference."""
    from gaussian_lic_amd import trainer
    P = ac.MODEL_P
    a, _ = _model(3)
    b, _ = _model(3)
    start = _state(a)
    vis = ac.mask(P, seed=70)
    small = ac.small_grads(P, 73)
    cx = trainer._ChunkedExchange(P, 1, ac.CHUNKS, _dev())
    assert cx.bounds[-1] == (1024, 1061) and all(p0 % 256 == 0 for p0, _ in cx.bounds) and len(cx.bounds) == 5
    for c, (p0, p1) in enumerate(cx.bounds):
        block = np.concatenate([x[p0:p1].ravel() for x in small])
        cx.small[cx.small_off[c]:cx.small_off[c] + 11 * (p1 - p0)].copy_(_t(block))
    tvis = _t(vis)
    a.optimizer.set_visibility_and_N(tvis, P)
    unaligned = 0
    for c, (p0, p1) in enumerate(cx.bounds):
        n = p1 - p0
        sm = cx.small.data_ptr() + 4 * cx.small_off[c]
        addr = {0: sm, 3: sm + 12 * n, 4: sm + 16 * n, 5: sm + 28 * n}
        unaligned += sum(x % 16 != 0 for x in addr.values())
        a.optimizer.step(None, only=[0, 3, 4, 5], rows=(p0, p1), grad_addr=addr)
    assert unaligned == 2      # n = 37: sm + 12 n and sm + 28 n
    b.optimizer.set_visibility_and_N(tvis, P)
    gx, go, gs, gr = (_t(x) for x in small)
    b.optimizer.step([gx, None, None, go, gs, gr])
    torch.cuda.synchronize()
    grads = {0: small[0], 3: small[1], 4: small[2], 5: small[3]}
    ref, _ = _expect(start, grads, vis, a.optimizer, (0, 3, 4, 5))
    sa, sb = _state(a), _state(b)
    _assert_state(sa, sb, "chunked against whole")
    _assert_state(sa, ref, "chunked against the reference")
    _assert_state(sb, ref, "whole against the reference")


def _chunk_payload(rgb, campos, p0, p1):
    """The all-gathered payload of rows [p0, p1) as training_step_rank1_chunked sees it: per view {dRGB [n,3], camera centre [3], n mask bytes,
    padding}; returns (bytes [n_views, nbytes], view stride in floats)."""
    n = p1 - p0
    nbytes = (12 * n + 12 + n + 3) // 4 * 4
    pa = np.zeros((rgb.shape[0], nbytes), np.uint8)
    for v in range(rgb.shape[0]):
        pa[v, :12 * n] = np.ascontiguousarray(rgb[v, p0:p1]).view(np.uint8).ravel()
        pa[v, 12 * n:12 * n + 12] = campos[v].view(np.uint8)
    return _t(pa), nbytes // 4


def _sh_rows(m, rgb, campos, deg):
    """The library's own gslic_sh_grad_from_rgb rows for the model's positions: {1: dL_ddc [P,3], 2: dL_dsh [P,45]}."""
    from gaussian_lic_amd import rasterizer as rz
    ddc, dsh = torch.full_like(m.features_dc.detach(), float("nan")), torch.full_like(m.features_rest.detach(), float("nan"))
    rz.sh_grad_from_rgb(m.xyz.detach(), _t(campos), _t(rgb), deg, ddc, dsh)
    torch.cuda.synchronize()
    return {1: ddc.cpu().numpy().reshape(m.P, 3), 2: dsh.cpu().numpy().reshape(m.P, dsh.numel() // m.P)}


@pytest.mark.parametrize("deg", [3, 0])
def test_h_sh_from_rgb_adam_chunk_by_chunk(deg):
    """step_sh_from_rgb(rows=) over the chunks of case (g) == the whole call == gslic_sh_grad_from_rgb's rows through the reference."""
    from gaussian_lic_amd import trainer
    P = ac.MODEL_P
    a, _ = _model(deg)
    b, _ = _model(deg)
    start = _state(a)
    rgb, campos, masks = ac.view_payload(P, 3, 77)
    vis = masks.max(0)
    tvis = _t(vis)
    bounds = trainer._ChunkedExchange(P, 1, ac.CHUNKS, _dev()).bounds
    a.optimizer.set_visibility_and_N(tvis, P)
    for p0, p1 in bounds:
        pa, stride = _chunk_payload(rgb, campos, p0, p1)
        n = p1 - p0
        a.optimizer.step_sh_from_rgb(a.xyz.detach(), pa[0, 12 * n:12 * n + 12].view(torch.float32), pa[0, :12 * n].view(torch.float32), deg, n_views=3,
                                     view_stride=stride, rows=(p0, p1))
    b.optimizer.set_visibility_and_N(tvis, P)
    b.optimizer.step_sh_from_rgb(b.xyz.detach(), _t(campos), _t(rgb), deg)
    torch.cuda.synchronize()
    ref, _ = _expect(start, _sh_rows(a, rgb, campos, deg), vis, a.optimizer, (1, 2))
    sa, sb = _state(a), _state(b)
    _assert_state(sa, sb, "chunked against whole")
    _assert_state(sa, ref, "chunked against the reference")
    assert not same_bits(sa[1][0], start[1][0])[vis != 0].all()       # the update did something


@pytest.mark.parametrize("n_views", [1, 3])
@pytest.mark.parametrize("deg", [3, 0])
def test_i_whole_step_from_the_exchange(deg, n_views):
    """gslic_sh_grad_from_rgb_adam_all on a hand-built payload (view and mask strides wider than the dense layout; rows seen by no view, by each
    view alone, by all): the OR, groups 1 and 2 from the library's rebuilt rows and groups 0, 3, 4, 5 from the given gradients through the
    reference, rows nobody sees untouched in all 18 arrays, and the same bits as step_sh_from_rgb + step(only=[0, 3, 4, 5])."""
    from gaussian_lic_amd import _lib
    P = ac.MODEL_P
    a, _ = _model(deg)
    b, _ = _model(deg)
    start = _state(a)
    rgb, campos, masks = ac.view_payload(P, n_views, 74 + n_views)
    seen = masks.max(0)
    counts = masks.sum(0)
    assert (counts == 0).any() and (counts == n_views).any() and all(((counts == 1) & (masks[v] == 1)).any() for v in range(n_views))
    small = ac.small_grads(P, 73)
    grads = {0: small[0], 3: small[1], 4: small[2], 5: small[3]}
    grads.update(_sh_rows(a, rgb, campos, deg))       # (before the step moves the positions the rows are rebuilt from)
    view_stride = 3 * P + 3 + 5                    # floats: dRGB, the camera centre, five floats of something else
    pay = np.full((n_views, view_stride), np.float32(777.0), np.float32)
    for v in range(n_views):
        pay[v, :3 * P] = rgb[v].ravel()
        pay[v, 3 * P:3 * P + 3] = campos[v]
    cpay = Carved(pay)
    vis_stride = P + 11
    vbytes = np.ones((n_views, vis_stride), np.uint8)          # the bytes between two views' masks read "visible"
    vbytes[:, :P] = masks
    cvis = CarvedBytes(vbytes.ravel())
    cout = CarvedBytes(np.full(P, 0x77, np.uint8), guard=0x5A)
    cs = [Carved(x) for x in small]
    d = a.optimizer.fused_descriptor()
    M = a.features_rest.shape[1]
    assert M == (15 if deg else 0)
    vp = ctypes.c_void_p
    _lib.check(_lib.lib().gslic_sh_grad_from_rgb_adam_all(P, deg, M, n_views, vp(a.xyz.data_ptr()), vp(cpay.ptr + 12 * P), vp(cpay.ptr), 0, vp(cvis.ptr),
                                                          vis_stride, vp(cout.ptr), ctypes.byref(d), vp(cs[0].ptr), vp(cs[1].ptr), vp(cs[2].ptr),
                                                          vp(cs[3].ptr), view_stride, _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    cpay.unchanged("the payload"); cvis.unchanged("the views' masks")
    for c in cs:
        c.unchanged("a small gradient")
    back = cout.dev.cpu().numpy()
    assert (back[:G] == 0x5A).all() and (back[G + P:] == 0x5A).all()
    assert np.array_equal(back[G:G + P], seen)                 # the OR, as 0 / 1
    ref, _ = _expect(start, grads, seen, a.optimizer, range(6))
    sa = _state(a)
    _assert_state(sa, ref, "one launch against the reference")
    for (x, y) in zip(sa, start):
        for u, w in zip(x, y):
            assert same_bits(u, w)[seen == 0].all()
    assert not same_bits(sa[0][0], start[0][0])[seen != 0].all()
    tvis = _t(seen)
    b.optimizer.set_visibility_and_N(tvis, P)
    b.optimizer.step_sh_from_rgb(b.xyz.detach(), _t(campos), _t(rgb), deg)
    b.optimizer.step([_t(small[0]), None, None, _t(small[1]), _t(small[2]), _t(small[3])], only=[0, 3, 4, 5])
    torch.cuda.synchronize()
    _assert_state(sa, _state(b), "one launch against the two calls")


def test_j_adam_inside_the_backward():
    """gslic_rasterize_backward_adam leaves parameters and moments at (gslic_rasterize_backward's gradients -> the reference with radii > 0);
    rows with radii <= 0 keep their bits.  (test_fused_gpu.py::test_adam_inside_backward_is_bit_identical holds it against the separate launch.)
    The gradients are the kernels' own here, not a generator's: an element whose update passes below 2^-126 is left out of the comparison —
    its share is printed, and must stay under 1 % (a guard on the scene, 96x64 with a few thousand Gaussians, not on the kernel)."""
    from gaussian_lic_amd import trainer
    from gaussian_lic_amd.synthetic import gt_image
    P, W, H = 3000, 96, 64
    a, cam = _model(3, P, W, H, seed=75)
    b, _ = _model(3, P, W, H, seed=75)
    cam.to_device(_dev())
    gt, bg = gt_image(H, W).to(_dev()), torch.zeros(3, device=_dev())
    start = _state(a)
    _terms, visible = trainer.training_step_fused(a, cam, gt, bg, do_step=False)
    torch.cuda.synchronize()
    grads = {i: g.detach().cpu().numpy().reshape(P, g.numel() // P) for i, g in enumerate(a._grad_slab.grads(a))}
    vis = visible.cpu().numpy().astype(np.uint8)
    assert 0 < int(vis.sum()) < P
    _assert_state(_state(a), start, "do_step=False")
    _terms, visible_b = trainer.training_step_fused(b, cam, gt, bg, adam_in_backward=True)
    torch.cuda.synchronize()
    assert np.array_equal(visible_b.cpu().numpy().astype(np.uint8), vis)
    ref, ok = _expect(start, grads, vis, a.optimizer, range(6), skip_subnormal=True)
    left_out = sum(int((~o).sum()) for o in ok) / float(sum(o.size for o in ok))
    print(f"fused backward: {left_out:.2e} of the elements left out as subnormal")
    assert left_out < 0.01
    sb = _state(b)
    _assert_state(sb, ref, "fused backward against the reference", ok)
    for x, y in zip(sb, start):
        for u, w in zip(x, y):
            assert same_bits(u, w)[vis == 0].all()
    assert not same_bits(sb[2][0], start[2][0])[vis != 0].all()
