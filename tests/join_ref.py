"""The definitions of include/sf_join.h restated: the reference of the join tests. np.float32 with one expression per
operation, keys and ranks in uint64 / uint32, winners by a dictionary. It imports neither the product nor the oracle."""
import numpy as np

EMPTY = (1 << 64) - 1
MASK64 = (1 << 64) - 1
HASH_MUL = 0x9E3779B97F4A7C15
Q_LIMIT = np.float32(1048576.0)  # 2^20
COUNT_FIELDS = ("n_in", "n_outside", "n_voxels", "n_below", "n_shared", "n_out")


def inverse_cell(cell):
    with np.errstate(all="ignore"):
        return np.float32(1.0) / np.float32(cell)


def voxel_keys(pos, cell):
    """(keys as uint64, inside as bool) of n positions (n x 3, float32); the key of a position outside the grid is EMPTY"""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    inv = inverse_cell(cell)
    with np.errstate(all="ignore"):
        scaled = pos * inv
        assert scaled.dtype == np.float32
        q = np.floor(scaled)
        inside = np.isfinite(pos).all(axis=1) & np.isfinite(q).all(axis=1) & (np.abs(q) < Q_LIMIT).all(axis=1)
    qi = np.where(inside[:, None], q, np.float32(0)).astype(np.int64) + (1 << 20)
    keys = (qi[:, 0].astype(np.uint64) << np.uint64(42)) | (qi[:, 1].astype(np.uint64) << np.uint64(21)) | qi[:, 2].astype(np.uint64)
    keys[~inside] = np.uint64(EMPTY)
    return keys, inside


def voxel_key(pos, cell):
    """the key of one position as a Python int, or None outside the grid"""
    keys, inside = voxel_keys(np.asarray(pos, np.float32).reshape(1, 3), cell)
    return int(keys[0]) if inside[0] else None


def ranks(conf):
    u = np.ascontiguousarray(conf, np.float32).view(np.uint32)
    r = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    r[(u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)] = 0
    return r


def table_slots(count):
    slots = 64
    while slots < 2 * count:
        slots *= 2
    return slots


def hash_slot(key, slots):
    log2 = slots.bit_length() - 1
    assert 1 << log2 == slots
    return ((int(key) * HASH_MUL) & MASK64) >> (64 - log2)


def counts(**kw):
    c = dict.fromkeys(COUNT_FIELDS, 0)
    c.update(kw)
    return c


def thin(surfels, cell):
    """(the surfels kept, counts, the mask)"""
    s = np.ascontiguousarray(surfels, np.float32).reshape(-1, 12)
    keys, inside = voxel_keys(s[:, 0:3], cell)
    rk = ranks(s[:, 3])
    best = {}  # key -> (rank, index): the highest rank, among equal ranks the lowest index
    for e in np.flatnonzero(inside).tolist():
        k, r = int(keys[e]), int(rk[e])
        if k not in best or r > best[k][0]:
            best[k] = (r, e)
    keep = ~inside
    for _, e in best.values():
        keep[e] = True
    n_outside = int((~inside).sum())
    assert int(keep.sum()) == len(best) + n_outside
    return s[keep], counts(n_in=s.shape[0], n_outside=n_outside, n_voxels=len(best), n_out=int(keep.sum())), keep


def transform_rows(M, xyz, translate):
    """rows of M (4 x 4, the matrix itself: M[r, c] = T[4 c + r]) applied to n vectors in the order of the header"""
    M = np.asarray(M, np.float32)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out = np.empty_like(xyz)
    with np.errstate(all="ignore"):
        for r in range(3):
            a = M[r, 0] * x
            b = M[r, 1] * y
            c = M[r, 2] * z
            ab = a + b
            abc = ab + c
            out[:, r] = abc + M[r, 3] if translate else abc
    assert out.dtype == np.float32
    return out


def merge(dst, src, M=None, cell=0.02, min_confidence=0.0, stamp=-1):
    """(the destination afterwards, counts); M None: the identity, through the same arithmetic"""
    d = np.ascontiguousarray(dst, np.float32).reshape(-1, 12)
    s = np.ascontiguousarray(src, np.float32).reshape(-1, 12)
    M = np.eye(4, dtype=np.float32) if M is None else np.asarray(M, np.float32)
    dkeys, dinside = voxel_keys(d[:, 0:3], cell)
    occupied = set(dkeys[dinside].tolist())
    with np.errstate(all="ignore"):
        passes = (s[:, 3] >= np.float32(min_confidence)) if np.float32(min_confidence) > 0 else np.ones(s.shape[0], bool)
    moved = s.copy()
    moved[:, 0:3] = transform_rows(M, s[:, 0:3], True)
    moved[:, 8:11] = transform_rows(M, s[:, 8:11], False)
    if stamp >= 0:
        moved[:, 6] = moved[:, 7] = np.float32(stamp)
    skeys, sinside = voxel_keys(moved[:, 0:3], cell)
    shared = passes & sinside & np.array([int(k) in occupied for k in skeys.tolist()], bool).reshape(-1)
    outside = passes & ~sinside
    add = passes & ~shared
    c = counts(n_in=s.shape[0], n_outside=int(outside.sum()), n_voxels=len(occupied), n_below=int((~passes).sum()), n_shared=int(shared.sum()),
               n_out=int(add.sum()))
    assert c["n_out"] == c["n_in"] - c["n_below"] - c["n_shared"]
    return np.concatenate([d, moved[add]]), c
