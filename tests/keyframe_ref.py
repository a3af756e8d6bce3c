"""The definitions of include/sf_keyframes.h in NumPy, one expression per operation, np.float32 for the two quantisations:
the thumbnail of a frame, fern codes and their packing, the distance of two codes, the (distance, slot) order of a query, the
novelty rule of an add call and the generator of the default ferns. What the GPU tests compare with, integer for integer."""
import numpy as np

from staticfusion_amd import keyframes
from staticfusion_amd.synth import LCG64

F = np.float32
FERN_DTYPE = keyframes.FERN_DTYPE  # (cell, t_grey, t_depth, reserved), int32 each


def grid(rows, cols, cell):
    return rows // cell, cols // cell


def thumbnail(depth, grey, cell):
    """(n, Z, G) per cell, each an int64 array of gr * gc entries in the order c = cv + cu * gr, of (rows, cols) images"""
    depth, grey = np.asarray(depth, F), np.asarray(grey, F)
    gr, gc = grid(depth.shape[0], depth.shape[1], cell)
    z, g = depth[:gr * cell, :gc * cell], grey[:gr * cell, :gc * cell]  # the remainder is never read
    with np.errstate(invalid="ignore"):
        valid = z > F(0)  # false for a NaN
        zq = np.rint(np.fmin(z, F(32)) * F(1024))
        gq = np.rint(np.fmin(np.fmax(g, F(0)), F(1)) * F(4096))  # fmax / fmin return the other operand for a NaN
    zq = np.where(valid, zq, F(0)).astype(np.int64)
    gq = gq.astype(np.int64)

    def cells(a):
        return a.reshape(gr, cell, gc, cell).sum(axis=(1, 3)).ravel(order="F")

    return cells(valid.astype(np.int64)), cells(zq), cells(gq)


def nibbles(thumb, ferns, cell):
    """the 4-bit code of every fern on a thumbnail"""
    n, Z, G = thumb
    a = cell * cell
    c = ferns["cell"].astype(np.int64)
    bit0 = G[c] > ferns["t_grey"].astype(np.int64) * a
    bit1 = (n[c] > 0) & (Z[c] > ferns["t_depth"].astype(np.int64) * n[c])
    bit2 = 2 * n[c] >= a
    return bit0.astype(np.uint32) | (bit1.astype(np.uint32) << 1) | (bit2.astype(np.uint32) << 2)


def pack(nib):
    """fern f in bits 4 * (f % 8) .. + 3 of word f / 8; unused nibbles 0"""
    words = (nib.shape[0] + 7) // 8
    out = np.zeros(words, np.uint32)
    for f, v in enumerate(nib):
        out[f // 8] |= np.uint32(int(v) << (4 * (f % 8)))
    return out


def unpack(code, n_ferns):
    f = np.arange(n_ferns)
    return (np.asarray(code, np.uint32)[f // 8] >> (4 * (f % 8)).astype(np.uint32)) & np.uint32(15)


def encode(depth, grey, ferns, cell):
    return pack(nibbles(thumbnail(depth, grey, cell), ferns, cell))


def distance(a, b, n_ferns):
    """the number of ferns whose nibbles differ"""
    return int((unpack(a, n_ferns) != unpack(b, n_ferns)).sum())


def query(db_codes, db_tags, code, tag, m, n_ferns):
    """the m smallest (distance, slot) pairs in ascending lexicographic order over the slots considered (every slot for
    tag < 0, else those whose tag equals it), padded with (-1, -1): a list of m (slot, distance)"""
    pairs = sorted((distance(c, code, n_ferns), s) for s, (c, t) in enumerate(zip(db_codes, db_tags)) if tag < 0 or t == tag)
    return [(s, d) for d, s in pairs[:m]] + [(-1, -1)] * max(m - len(pairs), 0)


def add(db_codes, db_tags, codes, tags, min_distance, n_ferns):
    """the novelty rule on lists: entry q is novel when no slot with its tag exists or the smallest distance to the slots with
    its tag is >= min_distance; novel entries are appended in the order of q. Returns (slots, nearest) and extends the lists."""
    assert len(set(tags)) == len(tags) and min(tags) >= 0
    nearest = [query(db_codes, db_tags, c, t, 1, n_ferns)[0] for c, t in zip(codes, tags)]  # all against the state before the call
    slots = []
    for c, t, (s, d) in zip(codes, tags, nearest):
        if s < 0 or d >= min_distance:
            slots.append(len(db_codes))
            db_codes.append(np.array(c, np.uint32))
            db_tags.append(int(t))
        else:
            slots.append(-1)
    return slots, nearest


def default_ferns(n_ferns, seed, n_cells):
    g = LCG64(seed)

    def nxt():
        return g.next_u64() >> 33

    out = np.zeros(n_ferns, FERN_DTYPE)
    for f in range(n_ferns):
        out[f] = (nxt() % n_cells, 410 + nxt() % 3277, 512 + nxt() % 6656, 0)
    return out
