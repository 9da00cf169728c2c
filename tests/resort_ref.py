"""The key rule of gslic_morton_order (include/gslic_hip.h) transcribed into numpy float32 — every step one IEEE float32 operation rounded on
its own, as the header states it — and the permutation it defines: a stable argsort of the keys.  The yardstick of tests/test_resort_*.py."""
import numpy as np

F = np.float32


def spread10(u):
    """10 bits -> every third bit (uint32 arrays)."""
    u = u.astype(np.uint32)
    u = (u | (u << np.uint32(16))) & np.uint32(0x030000FF)
    u = (u | (u << np.uint32(8))) & np.uint32(0x0300F00F)
    u = (u | (u << np.uint32(4))) & np.uint32(0x030C30C3)
    u = (u | (u << np.uint32(2))) & np.uint32(0x09249249)
    return u


def axis_cells(x, lo, hi):
    """u_k of the rule for one axis: x float32 [P], lo / hi float32 scalars -> uint32 [P] in 0..1023."""
    x = np.asarray(x, dtype=F)
    lo, hi = F(lo), F(hi)
    with np.errstate(all="ignore"):
        e = F(hi - lo)
        d = e if e > F(1e-30) else F(1e-30)                     # max(hi - lo, 1e-30f); a NaN extent reads as 1e-30f
        t = ((x - lo).astype(F) / d).astype(F)
        c = np.where(t > F(0), np.where(t < F(1), t, F(1)), F(0)).astype(F)   # min(max(t, 0), 1); NaN -> 0
        return np.trunc((c * F(1023.0)).astype(F)).astype(np.uint32)


def morton_keys(xyz, box):
    """uint32 [P]: xyz float32 [P,3], box float32 [6] = (lo xyz, hi xyz)."""
    xyz = np.ascontiguousarray(xyz, dtype=F).reshape(-1, 3)
    box = np.asarray(box, dtype=F).reshape(6)
    u = [spread10(axis_cells(xyz[:, k], box[k], box[3 + k])) for k in range(3)]
    return (u[0] | (u[1] << np.uint32(1)) | (u[2] << np.uint32(2))).astype(np.uint32)


def morton_perm(xyz, box):
    """(perm, keys_sorted): perm[s] = the old row that becomes row s — ascending keys, equal keys in storage order."""
    keys = morton_keys(xyz, box)
    perm = np.argsort(keys, kind="stable").astype(np.uint32)
    return perm, keys[perm]
