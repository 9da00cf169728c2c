"""The covisibility rule of include/gslic_hip.h (gslic_covis_*) restated in numpy on a bool matrix B [P, F]: B[r, f] = "frame f, when last
recorded, saw row r".  Everything is an integer: the tests compare with exact equality."""
import numpy as np

FRAME_COUNTS = (1, 31, 32, 33, 64, 65, 128, 1024)   # every word-boundary case of Wd = ceil(F / 32), the pair limit and the frame limit


def words(F):
    return (int(F) + 31) // 32


def pack(B):
    """bool [P, F] -> uint32 [P, Wd]: bit f of row r is bit f & 31 of word f >> 5."""
    B = np.asarray(B, dtype=bool)
    P, F = B.shape
    out = np.zeros((P, words(F)), dtype=np.uint32)
    for f in range(F):
        out[:, f >> 5] |= B[:, f].astype(np.uint32) << np.uint32(f & 31)
    return out


def unpack(bits, F):
    """uint32 (or int32) [P, Wd] -> bool [P, F]."""
    bits = np.asarray(bits).view(np.uint32) if np.asarray(bits).dtype == np.int32 else np.asarray(bits, dtype=np.uint32)
    f = np.arange(F)
    return ((bits[:, f >> 5] >> (f & 31).astype(np.uint32)) & 1).astype(bool)


def record(B, frame, seen, skip=0, rows=None):
    """The record rule on B in place: column `frame` of the rows of the range is REPLACED by seen (None clears); a frame outside [0, F) or a
    nonzero skip touches nothing."""
    P, F = B.shape
    if skip != 0 or not 0 <= frame < F:
        return B
    b, e = (0, P) if rows is None else rows
    B[b:e, frame] = False if seen is None else np.asarray(seen)[b:e] > 0
    return B


def pair_counts(B):
    """int64 [F, F]: B^T B (through float64, whose sums of zeros and ones are exact far beyond any row count; the integer product has no BLAS)."""
    B = np.asarray(B, dtype=np.float64)
    return (B.T @ B).astype(np.int64)


def frame_counts(B, frame):
    """int64 [F]: rows with bit `frame` and bit g; zeros for a frame outside [0, F)."""
    B = np.asarray(B, dtype=np.int64)
    if not 0 <= frame < B.shape[1]:
        return np.zeros(B.shape[1], dtype=np.int64)
    return B[B[:, frame] != 0].sum(0)


def seen_count(B, mask=None):
    """int64 [P]: popcount(row & mask), mask bool [F] or None = all."""
    B = np.asarray(B, dtype=np.int64)
    return (B if mask is None else B[:, np.asarray(mask, dtype=bool)]).sum(1)


def redundant(B, min_others, mask=None):
    """int64 [F]: rows with bit f (masked or not) and seen_count(mask) >= 1 + min_others."""
    B = np.asarray(B, dtype=np.int64)
    return B[seen_count(B, mask) >= 1 + min_others].sum(0)


def random_matrix(P, F, density, seed):
    return np.random.default_rng(seed).random((P, F)) < density
