"""-m gpu: the bits of every output of every loss entry point (fused SSIM, L1 + SSIM, its weighted form, the depth L1 and its weighted / Huber form),
pinned to a recording: tests/golden/loss_pinned_bits.npz holds seeded inputs and the int32 views of what the library computed from them at the commit
before the loss kernels were folded (one forward body, one depth pair, one block reduction).  Compared with integer equality (NaN-safe).

    python tests/test_loss_pinned_bits_gpu.py        records the fixture (on the GPU; under pytest the module only compares)

Shapes are the smallest that reach each path of the tiling: 32 x 32 colour tiles at (1, 1), (33, 65) (2 x 3 tiles with partial edge tiles) and (70, 45);
the drop-in SSIM pair at B = 2, (33, 17); 2048-pixel depth workgroups at (1, 1), (37, 53) (one partial workgroup) and (45, 91) (two and a tail).
Where the header promises the same bits from two entry points (the derivative maps, terms and dL_dimg of the split and the fused colour calls; the
gradient of the depth entry and of the weighted one without weight and threshold), both are held to ONE recorded array; the recorder refuses to
write a fixture in which they differ.  Scratch (`partials`) is zeroed before each call and recorded whole, so a write past the documented layout
shows too."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]

from gpu_helpers import gpu  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(HERE, "golden", "loss_pinned_bits.npz")
F = np.float32
LAM = 0.2          # lambda_dssim
LAMBDA_D = 0.5     # lambda_depth
COLOUR = [(1, 1), (33, 65), (70, 45)]
SSIM = (2, 3, 33, 17)
DEPTH = [(1, 1), (37, 53), (45, 91)]
DELTAS = [0.0, 0.3]


# ------------------------------------------------------------------------------------------------------------ inputs (recorded, not regenerated)
def _sprinkle(rng, a, values):
    """Put each of `values` at a few random places of the flat array (as many as it has room for)."""
    idx = iter(rng.permutation(a.size))
    for v in values:
        for _ in range(3):
            i = next(idx, None)
            if i is not None:
                a.flat[i] = v
    return a


def _make_inputs():
    rng = np.random.default_rng(20260)
    inp = {}
    for H, W in COLOUR:
        s = f"colour_{H}x{W}"
        gt = (rng.integers(0, 256, (3, H, W)) / 255.0).astype(F)                    # an 8-bit image
        img = np.clip(gt + (rng.random((3, H, W)).astype(F) - F(0.5)) * F(0.4), 0, 1).astype(F)
        tie = rng.random((3, H, W)) < 0.1
        img[tie] = gt[tie]                                                          # exact ties: sign(0) in the L1 branch
        w = rng.random((H, W)).astype(F)
        w[rng.random((H, W)) < 0.2] = 0.0
        _sprinkle(rng, w, [np.nan, -0.5, 1.75, np.inf, 1.0])
        if H * W == 1:
            w[0, 0] = 0.625
        inp[s + "/img"], inp[s + "/gt"], inp[s + "/weight"] = img, gt, w
    B, CH, H, W = SSIM
    inp["ssim/img1"] = rng.random((B, CH, H, W)).astype(F)
    img2 = rng.random((B, CH, H, W)).astype(F)
    tie = rng.random((B, CH, H, W)) < 0.1
    img2[tie] = inp["ssim/img1"][tie]
    inp["ssim/img2"] = img2
    inp["ssim/dL_dmap"] = (rng.standard_normal((B, CH, H, W)) * 1e-3).astype(F)
    for H, W in DEPTH:
        s = f"depth_{H}x{W}"
        gt = (rng.random((H, W)) * 10.0 + 0.01).astype(F)
        gt[rng.random((H, W)) < 0.4] = 0.0                                          # unmeasured pixels
        depth = (gt + (rng.random((H, W)).astype(F) - F(0.5)) * F(1.0)).astype(F)   # residuals on both sides of delta = 0.3
        tie = rng.random((H, W)) < 0.1
        depth[tie] = gt[tie]                                                        # exact ties: sign(0)
        w = (rng.integers(0, 49, (H, W)) / 16.0).astype(F)                          # 0 ... 3 in sixteenths
        _sprinkle(rng, w, [np.nan, -2.0, 7.5, np.inf])
        if H * W == 1:
            gt[0, 0], depth[0, 0], w[0, 0] = 2.0, 2.125, 1.75
        inp[s + "/depth"], inp[s + "/gt"], inp[s + "/weight"] = depth, gt, w
    return inp


# ------------------------------------------------------------------------------------------------------------ the entry points
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu())


def _call(name, *args):
    from gaussian_lic_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(*args, _lib.current_stream_ptr()))
    torch.cuda.synchronize()


def _empty(*shape):
    return torch.full(shape, float("nan"), device=gpu())


def _colour(inp, H, W, which):
    from gaussian_lic_amd import _lib, loss
    L, p = _lib.lib(), _lib.ptr
    s = f"colour_{H}x{W}"
    img, gt, w = (_dev(inp[f"{s}/{k}"]) for k in ("img", "gt", "weight"))
    d = [_empty(3, H, W) for _ in range(3)]
    dL = _empty(3, H, W)
    if which == "weighted":
        partials = torch.zeros(int(L.gslic_l1_ssim_loss_weighted_partials_count(3, H, W)), device=gpu())
        terms = _empty(3)
        _call("gslic_l1_ssim_loss_weighted_forward_backward", 3, H, W, loss.C1, loss.C2, LAM, p(img), p(gt), p(w), p(d[0]), p(d[1]), p(d[2]),
              p(partials), p(terms), p(dL))
        return {s + "/d1": d[0], s + "/d2": d[1], s + "/d3": d[2], s + "/w_terms": terms, s + "/w_partials": partials, s + "/w_dL": dL}
    partials = torch.zeros(int(L.gslic_loss_partials_count(1, 3, H, W)), device=gpu())
    terms = _empty(2)
    if which == "split":
        _call("gslic_l1_ssim_loss_forward", 1, 3, H, W, loss.C1, loss.C2, p(img), p(gt), p(d[0]), p(d[1]), p(d[2]), p(partials), p(terms))
        _call("gslic_l1_ssim_loss_backward", 1, 3, H, W, LAM, p(img), p(gt), p(d[0]), p(d[1]), p(d[2]), p(dL))
    else:
        _call("gslic_l1_ssim_loss_forward_backward", 1, 3, H, W, loss.C1, loss.C2, LAM, p(img), p(gt), p(d[0]), p(d[1]), p(d[2]), p(partials), p(terms),
              p(dL))
    return {s + "/d1": d[0], s + "/d2": d[1], s + "/d3": d[2], s + "/terms": terms, s + "/partials": partials, s + "/dL": dL}


def _ssim(inp, train):
    from gaussian_lic_amd import _lib, loss
    p = _lib.ptr
    B, CH, H, W = SSIM
    a, b, g = (_dev(inp["ssim/" + k]) for k in ("img1", "img2", "dL_dmap"))
    m = _empty(B, CH, H, W)
    if not train:
        _call("gslic_fusedssim_forward", B, CH, H, W, loss.C1, loss.C2, p(a), p(b), p(m), None, None, None)
        return {"ssim/map": m}
    d = [_empty(B, CH, H, W) for _ in range(3)]
    dL = _empty(B, CH, H, W)
    _call("gslic_fusedssim_forward", B, CH, H, W, loss.C1, loss.C2, p(a), p(b), p(m), p(d[0]), p(d[1]), p(d[2]))
    _call("gslic_fusedssim_backward", B, CH, H, W, loss.C1, loss.C2, p(a), p(b), p(g), p(d[0]), p(d[1]), p(d[2]), p(dL))
    return {"ssim/map": m, "ssim/d1": d[0], "ssim/d2": d[1], "ssim/d3": d[2], "ssim/dL": dL}


def _depth(inp, H, W, which, use_weight=False, delta=0.0):
    from gaussian_lic_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    s = f"depth_{H}x{W}"
    depth, gt, w = (_dev(inp[f"{s}/{k}"]) for k in ("depth", "gt", "weight"))
    dL = _empty(H, W)
    if which == "plain":
        partials = torch.zeros(int(L.gslic_depth_l1_loss_partials_count(H, W)), device=gpu())
        term = _empty(1)
        _call("gslic_depth_l1_loss_forward_backward", H, W, LAMBDA_D, p(depth), p(gt), p(partials), p(term), p(dL))
        return {s + "/dL_w0_d0": dL, s + "/term": term, s + "/partials": partials}
    partials = torch.zeros(int(L.gslic_depth_loss_weighted_partials_count(H, W)), device=gpu())
    terms = _empty(2)
    _call("gslic_depth_loss_weighted_forward_backward", H, W, LAMBDA_D, float(delta), p(depth), p(gt), p(w) if use_weight else None, p(partials),
          p(terms), p(dL))
    tag = f"_w{int(use_weight)}_d{int(delta > 0)}"   # (dL_w0_d0: the header's promise — the bits of the plain entry point)
    return {s + "/dL" + tag: dL, s + "/terms" + tag: terms, s + "/partials" + tag: partials}


CASES = {}
for _H, _W in COLOUR:
    for _which in ("split", "fused", "weighted"):
        CASES[f"colour_{_H}x{_W}-{_which}"] = functools.partial(_colour, H=_H, W=_W, which=_which)
CASES["ssim-train"] = functools.partial(_ssim, train=True)
CASES["ssim-map_only"] = functools.partial(_ssim, train=False)
for _H, _W in DEPTH:
    CASES[f"depth_{_H}x{_W}-plain"] = functools.partial(_depth, H=_H, W=_W, which="plain")
    for _uw in (False, True):
        for _delta in DELTAS:
            CASES[f"depth_{_H}x{_W}-weighted-w{int(_uw)}-delta{_delta}"] = functools.partial(_depth, H=_H, W=_W, which="weighted", use_weight=_uw,
                                                                                            delta=_delta)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


@functools.lru_cache(maxsize=None)
def _fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", sorted(CASES))
def test_outputs_have_the_recorded_bits(case):
    fix = _fixture()
    inp = {k[3:]: v for k, v in fix.items() if k.startswith("in/")}
    out = CASES[case](inp)
    assert out
    for name, t in out.items():
        want, got = fix["out/" + name], _bits(t)
        assert want.dtype == np.int32 and got.shape == want.shape, name
        assert np.array_equal(got, want), (name, int((got != want).sum()), "words differ")


def record():
    inp = _make_inputs()
    store = {"in/" + k: v for k, v in inp.items()}
    for case in sorted(CASES):
        for name, t in CASES[case](inp).items():
            b = _bits(t)
            if "out/" + name in store:
                assert np.array_equal(store["out/" + name], b), f"{case}: {name} differs from the entry point that shares it"
            store["out/" + name] = b
    np.savez_compressed(FIXTURE, **store)
    print(f"{FIXTURE}: {len(store)} arrays, {os.path.getsize(FIXTURE)} bytes")


if __name__ == "__main__":
    record()
