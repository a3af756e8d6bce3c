"""The definition of include/sf_closure.h in np.float32, one expression per operation, on top of the NumPy renderer of
tests/view_ref.py (the two draws): SAMPLES, PER SAMPLE, COUNTS and the output order. The reference of the closure tests. It
imports nothing of the product; views and parameters are anything with the members of sfv_view and sfc_params."""
import numpy as np

import view_ref

F = np.float32
RECORD = np.dtype([("src", np.float32, 3), ("dst", np.float32, 3), ("time", np.float32), ("weight", np.float32)])
COUNT_FIELDS = ("n_samples", "n_new", "n_old", "n_both", "n_near", "n_apart", "n_links", "n_pins", "n_dropped", "first", "sum_dz", "sum_shift")
BOTH, NEAR, APART, LINK, PIN, LINK_DROPPED, PIN_DROPPED = 1, 2, 4, 8, 16, 32, 64
DEFAULTS = dict(stride=4, pins=1, gate_abs=0.1, gate_rel=0.05, min_time_gap=0.0, w_link=1.0, w_pin=1.0)


def sample_positions(extent, stride):
    """SAMPLES along one axis: s2 + i * s < extent"""
    return list(range(stride // 2, extent, stride))


def max_records(rows, cols, stride):
    return 2 * len(sample_positions(rows, stride)) * len(sample_positions(cols, stride))


def _finite(rec):
    return np.all(np.isfinite(rec["src"]), axis=-1) & np.all(np.isfinite(rec["dst"]), axis=-1) & np.isfinite(rec["time"])


def link_samples(has_a, sa, has_o, so, zA, zO, T, P, p):
    """PER SAMPLE for N samples at once: (mask (N,), links (N,) RECORD, pins (N,) RECORD, q_dz (N,), q_shift (N,)); a record
    counts only with its bit. has_a / has_o: (N,) bool; sa / so: (N, 12) surfel records (any value where nothing is drawn);
    T = inverse(view_from.pose) and P = view_to.pose as 16 column-major float32; p: the parameters."""
    with np.errstate(all="ignore"):
        has_a, has_o = np.asarray(has_a, bool), np.asarray(has_o, bool)
        sa, so = np.asarray(sa, np.float32).reshape(-1, 12), np.asarray(so, np.float32).reshape(-1, 12)
        zA, zO = np.asarray(zA, np.float32), np.asarray(zO, np.float32)
        T, P = np.asarray(T, np.float32), np.asarray(P, np.float32)
        both = has_a & has_o
        dz = np.abs(zA - zO)
        gate = F(p.gate_abs) + F(p.gate_rel) * zO
        near = both & (dz <= gate)
        apart = near & (sa[:, 6] - so[:, 6] > F(p.min_time_gap))
        q = lambda v: np.rint(np.fmin(v, F(32)) * F(16384)).astype(np.float64)  # noqa: E731
        q_dz = np.where(near, q(dz), 0).astype(np.int64)
        x, y, z = sa[:, 0], sa[:, 1], sa[:, 2]
        h = [((T[r] * x + T[4 + r] * y) + T[8 + r] * z) + T[12 + r] for r in range(3)]
        links = np.zeros(sa.shape[0], RECORD)
        links["src"] = sa[:, 0:3]
        for r in range(3):
            links["dst"][:, r] = ((P[r] * h[0] + P[4 + r] * h[1]) + P[8 + r] * h[2]) + P[12 + r]
        links["time"], links["weight"] = sa[:, 6], F(p.w_link)
        link = apart & _finite(links)
        d = links["dst"] - links["src"]
        q_shift = np.where(link, q(np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])), 0).astype(np.int64)
        pins = np.zeros(sa.shape[0], RECORD)
        pins["src"] = pins["dst"] = so[:, 0:3]
        pins["time"], pins["weight"] = so[:, 6], F(p.w_pin)
        want_pin = apart if p.pins == 1 else (has_o if p.pins == 2 else np.zeros_like(has_o))
        pin = want_pin & _finite(pins)
        mask = (BOTH * both + NEAR * near + APART * apart + LINK * link + PIN * pin + LINK_DROPPED * (apart & ~link) + PIN_DROPPED * (want_pin & ~pin)).astype(np.int32)
    return mask, links, pins, q_dz, q_shift


def ordered(mask, links, pins):
    """OUTPUT ORDER: sample order, at one sample the LINK before the PIN"""
    pair = np.stack([links, pins], axis=1)
    keep = np.stack([(mask & LINK) != 0, (mask & PIN) != 0], axis=1)
    return pair[keep]


def link_sample(sa, so, zA, zO, T, P, p):
    """PER SAMPLE for one sample: (mask, the records made); sa / so: a surfel record or None"""
    zero = np.zeros(12, np.float32)
    mask, links, pins, _, _ = link_samples([sa is not None], zero if sa is None else sa, [so is not None], zero if so is None else so, [zA], [zO], T, P, p)
    return int(mask[0]), ordered(mask, links, pins)


def build_entry(surf_new, tick_new, surf_old, tick_old, view_from, view_to, p, first=0):
    """(records, counts dict) of one entry"""
    surf_new = np.ascontiguousarray(surf_new, np.float32).reshape(-1, 12)
    surf_old = np.ascontiguousarray(surf_old, np.float32).reshape(-1, 12)
    A = view_ref.render(surf_new, view_from, tick=tick_new)
    O = view_ref.render(surf_old, view_to, tick=tick_old)
    T = view_ref.invert_pose(view_from.pose[:])
    P = np.array(view_to.pose[:], np.float32)
    ys, xs = sample_positions(int(view_from.rows), int(p.stride)), sample_positions(int(view_from.cols), int(p.stride))
    c = dict.fromkeys(COUNT_FIELDS, 0)
    c["first"] = first
    if not ys or not xs:
        return np.zeros(0, RECORD), c
    Y, X = (g.ravel() for g in np.meshgrid(ys, xs, indexing="ij"))  # y in the outer loop, x in the inner
    a, o = A["index"][Y, X].astype(np.int64), O["index"][Y, X].astype(np.int64)
    pick = lambda surf, i: surf[np.maximum(i, 0)] if surf.shape[0] else np.zeros((i.shape[0], 12), np.float32)  # noqa: E731
    mask, links, pins, q_dz, q_shift = link_samples(a >= 0, pick(surf_new, a), o >= 0, pick(surf_old, o), A["depth"][Y, X], O["depth"][Y, X], T, P, p)
    bit = lambda b: int(((mask & b) != 0).sum())  # noqa: E731
    c.update(n_samples=int(Y.shape[0]), n_new=int((a >= 0).sum()), n_old=int((o >= 0).sum()), n_both=bit(BOTH), n_near=bit(NEAR), n_apart=bit(APART),
             n_links=bit(LINK), n_pins=bit(PIN), n_dropped=bit(LINK_DROPPED) + bit(PIN_DROPPED), sum_dz=int(q_dz.sum()), sum_shift=int(q_shift.sum()))
    return ordered(mask, links, pins), c


def build(entries):
    """entries: (surf_new, tick_new, surf_old, tick_old, view_from, view_to, params) each; (records of all, [counts]) with
    `first` chaining"""
    recs, counts, first = [], [], 0
    for e in entries:
        r, c = build_entry(*e, first=first)
        recs.append(r)
        counts.append(c)
        first += r.shape[0]
    return (np.concatenate(recs) if recs else np.zeros(0, RECORD)), counts


def same_records(a, b):
    """np.array_equal on the bytes of two RECORD arrays (a NaN never reaches a record: dropped)"""
    a, b = np.asarray(a, RECORD), np.asarray(b, RECORD)
    return a.shape == b.shape and all(np.array_equal(a[k], b[k]) for k in RECORD.names)
