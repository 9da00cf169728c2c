"""Reference of gslic_lidar_zbuffer_resolve_weighted (include/gslic_hip.h): a plain numpy restatement of the rule, with loops.  Per pixel it scans
the cells of the clipped (2r+1) x (2r+1) window by brute force — for the minimum key, then for the smallest dx^2 + dy^2 among the cells whose OWN
key equals it — and takes the four weight steps as np.float32 scalars, each ONE IEEE float32 operation rounded on its own.  It knows nothing of
rows, columns or tiles.  Nothing here calls the library.  test_lidar_weight_cpu.py pins it against trainer.range_weight on CPU tensors and against
tests/lidar_depth_ref.py."""
import numpy as np

F = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)

SIZES = [(5, 3), (64, 16), (37, 23), (130, 35)]   # window larger than the image; one tile; 1 x 2 tiles, ragged; 3 x 3 tiles, ragged
FOOTPRINTS = [0, 1, 3, 8]
FALLOFFS = [0.0, 0.25, 1e30]
SIGMAS = [(0.05, 0.02), (0.05, 0.0)]


def key_of(z, index):
    """The z-buffer key of a return at camera depth z (> 0) from point `index`."""
    return (np.uint64(F(z).view(np.uint32)) << np.uint64(32)) | np.uint64(index)


def weight_of(d, s2, sigma_abs, sigma_rel, falloff):
    """The four steps of the header for one measured pixel: np.float32 scalars in, np.float32 out."""
    sa, sr, fo = F(sigma_abs), F(sigma_rel), F(falloff)
    with np.errstate(all="ignore"):
        a = F(sa + F(sr * F(d)))
        rw = F(sa / a)
        f = F(F(1.0) / F(F(1.0) + F(fo * F(s2))))
        return F(rw * f)


def resolve_weighted(zbuf, W, H, footprint=0, sigma_abs=1.0, sigma_rel=0.0, falloff=0.0):
    """dict(key uint64 [H,W], depth float32, index int32, dist2 int32, weight float32, n_measured int) of a z-buffer of W * H uint64 keys."""
    z2 = np.asarray(zbuf, np.uint64).reshape(H, W)
    r = int(footprint)
    # every cell (x + dx, y + dy) of the window, one at a time, for all pixels at once; a cell outside the image is no cell of the CLIPPED window:
    # it is marked by a flag of its own, not by the empty key, so the scan does not lean on "empty never matches"
    cells = []
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            k = np.full((H, W), EMPTY, np.uint64)
            inside = np.zeros((H, W), bool)
            ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
            if ys.start < ys.stop and xs.start < xs.stop:
                k[ys, xs] = z2[ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
                inside[ys, xs] = True
            cells.append((k, inside, dx * dx + dy * dy))
    key = np.full((H, W), EMPTY, np.uint64)
    for k, inside, _s in cells:
        key = np.where(inside & (k < key), k, key)
    hit = key != EMPTY
    s2 = np.full((H, W), 2 * r * r + 1, np.int64)
    for k, inside, s in cells:
        s2 = np.where(inside & hit & (k == key) & (s < s2), s, s2)
    assert bool((s2[hit] <= 2 * r * r).all())                         # one such cell always exists
    depth = np.where(hit, (key >> np.uint64(32)).astype(np.uint32).view(F), F(0))
    index = np.where(hit, (key & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32), np.int32(-1)).astype(np.int32)
    dist2 = np.where(hit, s2, -1).astype(np.int32)
    sa, sr, fo = F(sigma_abs), F(sigma_rel), F(falloff)
    with np.errstate(all="ignore"):                                   # (float32 arrays: every line below is ONE float32 operation per pixel)
        prod = sr * depth
        a = sa + prod
        rw = sa / a
        fs = fo * np.where(hit, s2, 0).astype(F)
        den = F(1.0) + fs
        f = F(1.0) / den
        w = rw * f
    assert all(v.dtype == F for v in (prod, a, rw, fs, den, f, w))
    weight = np.where(hit, w, F(0)).astype(F)
    return dict(key=key, depth=depth.astype(F), index=index, dist2=dist2, weight=weight, n_measured=int(hit.sum()))


def empty(W, H):
    return np.full(W * H, EMPTY, np.uint64)


# ----------------------------------------------------------------------------------------------------------------- hand-written z-buffers
def planted_buffers(W, H):
    """{name: z-buffer uint64 [H*W]} of the hand-written cases, each fitted to the image (cells outside it are left out)."""
    out = {}

    def put(zb, x, y, z, index):
        if 0 <= x < W and 0 <= y < H:
            zb[y * W + x] = key_of(z, index)

    for name, (x, y) in dict(corner00=(0, 0), corner10=(W - 1, 0), corner01=(0, H - 1), corner11=(W - 1, H - 1), centre=(W // 2, H // 2)).items():
        zb = empty(W, H)
        put(zb, x, y, 2.0, 7)
        out[name] = zb
    zb = empty(W, H)                                   # the tile seams: x = 63 | 64 and y = 15 | 16, nearer returns on the far side of each
    put(zb, 63, 2, 3.0, 1); put(zb, 64, 9, 2.5, 2); put(zb, 5, 15, 4.0, 3); put(zb, 20, 16, 1.5, 4); put(zb, 63, 15, 6.0, 5); put(zb, 64, 16, 5.0, 6)
    out["seams"] = zb
    zb = empty(W, H)                                   # equal z, different index, symmetric about (cx, cy): the lower index wins on every pixel
    cx, cy = min(W - 2, 9), min(H - 1, 1)              # that sees both; a farther return NEARER to (cx + 1, cy) loses to it
    put(zb, cx - 1, cy, 2.0, 11); put(zb, cx + 1, cy, 2.0, 10)
    out["equal_z"] = zb
    zb = empty(W, H)                                   # a pixel whose own return is farther than its neighbour's: dist2 > 0 on a measured pixel
    px, py = min(W - 2, 3), min(H - 1, 2)
    put(zb, px, py, 5.0, 0); put(zb, px + 1, py, 1.25, 1)
    out["overruled"] = zb
    zb = empty(W, H)                                   # the SAME key in two pixels (a reused index_base): the nearer copy counts
    put(zb, 1, 0, 2.0, 3); put(zb, min(W - 1, 4), min(H - 1, 2), 2.0, 3)
    out["same_key_twice"] = zb
    out["empty"] = empty(W, H)
    return out
