"""The definition of include/sf_carve.h in np.float32, one expression per operation in the written order: OBSERVE for all surfels
of a map against one entry at once, DECIDE, the counts, the packed votes and the stable partition. The reference of the carve
tests. It imports nothing of the product; views and parameters are anything with the members of sfv_view and sfe_params. Images
are (rows, cols) arrays: element (v, u) is the frame's zf[v + u * rows]."""
import numpy as np

import view_ref

F = np.float32
UNSEEN, THROUGH, SUPPORTED, OCCLUDED = 0, 1, 2, 3
COUNT_FIELDS = ("n_in", "n_judged", "n_through", "n_supported", "n_occluded", "n_carved", "n_out")
DEFAULTS = dict(tol_abs=0.02, tol_rel=0.01, z_max=8.0, min_cos=0.2, window=1, min_pixels=5, min_votes=2, max_support=0, dry_run=0)


def pdot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def observe(surfels, tick, view, depth, p, centre_depth=False):
    """OBSERVE: (class (N,) int32, found (N, 3) int32: through, near, front) of the (N, 12) surfels of a map at `tick` against
    `view` and the (rows, cols) depth image. centre_depth=True is NOT the rule: it compares with h.z instead of the depth of
    the pixel's ray on the surfel's plane (what tests/test_carve_reference_cpu.py shows to be wrong on a grazing floor)."""
    s = np.ascontiguousarray(surfels, np.float32).reshape(-1, 12)
    n = s.shape[0]
    rows, cols = int(view.rows), int(view.cols)
    zf = np.asarray(depth, np.float32)
    assert zf.shape == (rows, cols)
    T = view_ref.invert_pose(view.pose[:])
    T = np.asarray(T, np.float32)
    cx, cy, fx, fy = F(view.cx), F(view.cy), F(view.fx), F(view.fy)
    max_depth, min_conf = F(view.max_depth), F(view.min_confidence)
    tol_abs, tol_rel, z_max, min_cos = F(p.tol_abs), F(p.tol_rel), F(p.z_max), F(p.min_cos)
    w = int(p.window)
    with np.errstate(all="ignore"):
        h = [((T[k] * s[:, 0] + T[4 + k] * s[:, 1]) + T[8 + k] * s[:, 2]) + T[12 + k] for k in range(3)]
        m = [(T[k] * s[:, 8] + T[4 + k] * s[:, 9]) + T[8 + k] * s[:, 10] for k in range(3)]
        culled = (h[2] > max_depth) | (h[2] < F(0.4)) | (s[:, 3] < min_conf)
        if int(view.max_age) >= 0:
            culled |= ~(F(int(tick)) - s[:, 7] <= F(int(view.max_age)))
        d, mm, hh = pdot(m, h), pdot(m, m), pdot(h, h)
        facing = (d < 0) & (d * d >= (min_cos * min_cos) * (mm * hh))
        qx = ((fx * h[0]) / h[2] + cx) + F(0.5)
        qy = ((fy * h[1]) / h[2] + cy) + F(0.5)
        inside = (qx >= 0) & (qx < F(cols)) & (qy >= 0) & (qy < F(rows))
        live = ~culled & facing & inside
        i = np.where(live, np.floor(qx), 0).astype(np.int64)
        j = np.where(live, np.floor(qy), 0).astype(np.int64)
        found = np.zeros((n, 3), np.int32)
        for di in range(-w, w + 1):
            for dj in range(-w, w + 1):
                ii, jj = i + di, j + dj
                ok = live & (ii >= 0) & (ii < cols) & (jj >= 0) & (jj < rows)
                z = zf[np.clip(jj, 0, rows - 1), np.clip(ii, 0, cols - 1)]
                valid = ok & (z > 0) & (z <= z_max)
                lx = (ii.astype(np.float32) - cx) / fx
                ly = (jj.astype(np.float32) - cy) / fy
                den = (lx * m[0] + ly * m[1]) + m[2]
                zp = h[2] if centre_depth else d / den
                valid &= (zp >= F(0.4)) & (zp <= max_depth)
                tol = tol_abs + tol_rel * zp
                r = z - zp
                found[:, 0] += valid & (r > tol)
                found[:, 1] += valid & (np.abs(r) <= tol)
                found[:, 2] += valid & (r < -tol)
    cls = np.where(found[:, 1] > 0, SUPPORTED, np.where(found[:, 0] >= int(p.min_pixels), THROUGH, np.where(found[:, 2] > 0, OCCLUDED, UNSEEN))).astype(np.int32)
    return cls, found


def decide(v_through, v_support, p):
    """DECIDE"""
    return (np.asarray(v_through) >= int(p.min_votes)) & (np.asarray(v_support) <= int(p.max_support))


def carve_map(surfels, tick, p, entries):
    """one map against its entries [(view, depth image)]: dict(classes (n_entries, N), votes (N,) uint32 packed, carved (N,)
    bool, counts, out: the surfels that stay, in their old order -- the input itself under dry_run or with nothing carved)"""
    s = np.ascontiguousarray(surfels, np.float32).reshape(-1, 12)
    n = s.shape[0]
    classes = np.zeros((len(entries), n), np.int32)
    for q, (view, depth) in enumerate(entries):
        classes[q] = observe(s, tick, view, depth, p)[0]
    v_through = (classes == THROUGH).sum(0).astype(np.int64)
    v_support = (classes == SUPPORTED).sum(0).astype(np.int64)
    carved = decide(v_through, v_support, p)
    any_of = lambda c: int((classes == c).any(0).sum())  # noqa: E731
    counts = dict(n_in=n, n_judged=int((classes != UNSEEN).any(0).sum()), n_through=any_of(THROUGH), n_supported=any_of(SUPPORTED), n_occluded=any_of(OCCLUDED),
                  n_carved=int(carved.sum()), n_out=n - int(carved.sum()))
    out = s if (int(p.dry_run) or not carved.any()) else s[~carved]
    return dict(classes=classes, votes=(v_through | (v_support << 16)).astype(np.uint32), carved=carved, counts=counts, out=out)


def carve(maps, params, entries):
    """a call: maps [(surfels, tick)], params one per map, entries [(map index, view, depth image)]; one carve_map dict per map"""
    return [carve_map(s, tick, params[m], [(v, d) for k, v, d in entries if k == m]) for m, (s, tick) in enumerate(maps)]
