"""The definitions of include/sf_regions.h in NumPy / Python, one expression per float operation, all of them np.float32:
the mask, the link test, components as the classes of a plain union-find over the links, the numbering by `first`, the label
image, the records and the summary. What the GPU tests compare with, integer for integer. Imports neither the product nor
the oracle."""
import numpy as np

F = np.float32
REGION_FIELDS = ("n", "first", "v_min", "v_max", "u_min", "u_max", "z_min", "z_max", "sum_v", "sum_u", "sum_z", "sum_b")
REGION_DTYPE = np.dtype([(k, np.int32) for k in REGION_FIELDS[:8]] + [(k, np.int64) for k in REGION_FIELDS[8:]])
SUMMARY_FIELDS = ("n_mask", "n_components", "n_regions", "n_written")
SUMMARY_DTYPE = np.dtype([(k, np.int32) for k in SUMMARY_FIELDS] + [("reserved", np.int32, (4,))])

DEFAULTS = dict(z_max=8.0, b_max=0.5, dz_abs=0.05, dz_rel=0.02, connectivity=8, min_pixels=16, use_b=1)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def mask(depth, b, p):
    z = np.asarray(depth, F)
    with np.errstate(invalid="ignore"):
        m = (z > F(0)) & (z <= F(p["z_max"]))  # false for a NaN; +inf fails the second
        if p["use_b"]:
            m = m & (np.asarray(b, F) < F(p["b_max"]))
    return m


def linked(zp, zq, p):
    """the link test of two depths (arrays or scalars) that are both in the mask"""
    zp, zq = np.asarray(zp, F), np.asarray(zq, F)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = zp - zq
        lhs = np.abs(diff)
        near = np.fmin(zp, zq)
        prod = F(p["dz_rel"]) * near
        rhs = F(p["dz_abs"]) + prod
        return lhs <= rhs


def links(depth, m, p):
    """pairs (i, j) of linked pixel indices v + u * rows"""
    z = np.asarray(depth, F)
    rows, cols = z.shape
    idx = np.arange(rows)[:, None] + np.arange(cols)[None, :] * rows
    steps = [(1, 0), (0, 1)] + ([(1, 1), (1, -1)] if p["connectivity"] == 8 else [])
    out = []
    for dv, du in steps:
        # p = (v, u), q = (v + dv, u + du)
        if du >= 0:
            ps, qs = (slice(0, rows - dv), slice(0, cols - du)), (slice(dv, rows), slice(du, cols))
        else:
            ps, qs = (slice(0, rows - dv), slice(1, cols)), (slice(dv, rows), slice(0, cols - 1))
        both = m[ps] & m[qs]
        ok = both & linked(np.where(both, z[ps], F(1)), np.where(both, z[qs], F(1)), p)
        out.append(np.stack([idx[ps][ok], idx[qs][ok]], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 2), np.int64)


def components(depth, m, p):
    """root (the smallest index of its component) per pixel index, -1 outside the mask"""
    rows, cols = m.shape
    parent = list(range(rows * cols))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for i, j in links(depth, m, p).tolist():
        a, c = find(i), find(j)
        if a != c:
            if a < c:
                parent[c] = a
            else:
                parent[a] = c
    par = np.array(parent, np.int64)
    while True:  # every pixel to its root
        nxt = par[par]
        if np.array_equal(nxt, par):
            break
        par = nxt
    return np.where(m.ravel(order="F"), par, -1)


def label(depth, b, p, max_regions, root=None):
    """(summary record, max_regions region records, (rows, cols) int32 label image) of one frame; root: what components()
    gave for the same frame and the same parameters but min_pixels, which it does not read"""
    z = np.asarray(depth, F)
    rows, cols = z.shape
    m = mask(z, b, p)
    if root is None:
        root = components(z, m, p)
    inside = root >= 0
    firsts, sizes = np.unique(root[inside], return_counts=True)  # ascending first
    big = sizes >= p["min_pixels"]
    number = np.zeros(rows * cols, np.int64)  # at a root: its region number, 0 for a small component
    number[firsts[big]] = np.arange(1, int(big.sum()) + 1)
    lab = np.zeros(rows * cols, np.int64)
    lab[inside] = np.where(number[root[inside]] > 0, number[root[inside]], -1)
    r_total = int(big.sum())
    written = min(r_total, max_regions)
    summ = np.zeros((), SUMMARY_DTYPE)
    summ["n_mask"], summ["n_components"], summ["n_regions"], summ["n_written"] = int(m.sum()), len(firsts), r_total, written
    zf = z.ravel(order="F")
    with np.errstate(invalid="ignore", over="ignore"):
        zq = np.where(inside, np.rint(np.where(inside, zf, F(0)) * F(1024)), 0).astype(np.int64)
        if p["use_b"]:
            bf = np.asarray(b, F).ravel(order="F")
            clipped = np.fmin(np.fmax(np.where(inside, bf, F(0)), F(0)), F(1))
            bq = np.rint(clipped * F(4096)).astype(np.int64)
        else:
            bq = np.zeros(rows * cols, np.int64)
    i = np.arange(rows * cols)
    v, u = i % rows, i // rows
    rec = np.zeros(max_regions, REGION_DTYPE)
    s = (lab >= 1) & (lab <= written)
    k = lab[s] - 1  # the record of every pixel that has one
    head = rec[:written]
    head["n"] = np.bincount(k, minlength=written)
    for name, val in (("first", i), ("v_min", v), ("u_min", u), ("z_min", zq)):
        lo = np.full(written, np.iinfo(np.int64).max)
        np.minimum.at(lo, k, val[s])
        head[name] = lo
    for name, val in (("v_max", v), ("u_max", u), ("z_max", zq)):
        hi = np.full(written, -1)
        np.maximum.at(hi, k, val[s])
        head[name] = hi
    for name, val in (("sum_v", v), ("sum_u", u), ("sum_z", zq), ("sum_b", bq)):
        total = np.zeros(written, np.int64)
        np.add.at(total, k, val[s])
        head[name] = total
    return summ, rec, lab.reshape(cols, rows).T.astype(np.int32)
