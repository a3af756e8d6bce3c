"""The definitions of include/sf_tracks.h in NumPy / Python, one expression per float operation, all of them np.float32 but
`relative`, which is np.float64 with one rounding per entry: the relative transform, the warp, the overlap table, the greedy
assignment, the ids, the track records with their world-frame boxes and sums, the summary, the id image and the slot a tracker
keeps. Step 1, the regions of a frame, is region_ref. What the GPU tests compare with, integer for integer. Imports neither
the product nor the oracle."""
import numpy as np

import region_ref as rr

F = np.float32
TRACK_FIELDS = ("id", "region", "prev_region", "birth_frame", "age", "overlap", "n", "first", "v_min", "v_max", "u_min", "u_max", "z_min", "z_max")
TRACK_DTYPE = np.dtype([(k, np.int32) for k in TRACK_FIELDS] + [("qmin", np.int32, (3,)), ("qmax", np.int32, (3,))]
                       + [(k, np.int64) for k in ("sum_v", "sum_u", "sum_z", "sum_b")] + [("sum_q", np.int64, (3,))])
SUMMARY_FIELDS = ("n_regions", "n_tracked", "n_matched", "n_born", "n_ended", "n_untracked", "n_warped", "next_id")
SUMMARY_DTYPE = np.dtype([(k, np.int32) for k in SUMMARY_FIELDS])

DEFAULTS = dict(min_overlap=1, min_share=256, use_depth_gate=1, dz_abs=0.10, dz_rel=0.05)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def camera(pose=None, cx=0.0, cy=0.0, fx=1.0, fy=1.0):
    """pose: 4x4 (row, col) camera-to-world"""
    return dict(pose=np.array(np.eye(4) if pose is None else pose, F).reshape(4, 4), cx=F(cx), cy=F(cy), fx=F(fx), fy=F(fy))


def relative(pose0, pose1):
    """D of the header as a 4x4 (row, col) float32 array, or None for a non-finite entry; bit-equal poses give the identity"""
    p0, p1 = np.asarray(pose0, F).reshape(4, 4), np.asarray(pose1, F).reshape(4, 4)
    if not (np.isfinite(p0).all() and np.isfinite(p1).all()):
        return None
    D = np.eye(4, dtype=F)
    if p0.tobytes() == p1.tobytes():
        return D
    a0, a1 = p0.astype(np.float64), p1.astype(np.float64)
    d = [a0[r, 3] - a1[r, 3] for r in range(3)]
    for i in range(3):
        for j in range(3):
            a = a1[0, i] * a0[0, j]
            b = a1[1, i] * a0[1, j]
            c = a1[2, i] * a0[2, j]
            ab = a + b
            D[i, j] = F(ab + c)
        a = a1[0, i] * d[0]
        b = a1[1, i] * d[1]
        c = a1[2, i] * d[2]
        ab = a + b
        D[i, 3] = F(ab + c)
    return D


def back_project(cam, v, u, z):
    """P of the header for pixel arrays v, u (integers) with depths z"""
    du = u.astype(F) - cam["cx"]
    dv = v.astype(F) - cam["cy"]
    xu = du * z
    yv = dv * z
    return xu / cam["fx"], yv / cam["fy"], z


def transform(T, x, y, z):
    """the three rows of a 4x4 (row, col) transform applied to points, in the header's order"""
    T = np.asarray(T, F)
    out = []
    for i in range(3):
        a = T[i, 0] * x
        b = T[i, 1] * y
        c = T[i, 2] * z
        ab = a + b
        abc = ab + c
        out.append(abc + T[i, 3])
    return out


def warp(D, cam0, cam1, v, u, z, rows, cols):
    """(kept, vi, ui, hz) of previous pixels (v, u) with depths z: integer targets where kept"""
    with np.errstate(all="ignore"):
        x, y, zz = back_project(cam0, v, u, np.asarray(z, F))
        hx, hy, hz = transform(D, x, y, zz)
        front = hz > F(0)
        nu = cam1["fx"] * hx
        nv = cam1["fy"] * hy
        qu = nu / hz
        qv = nv / hz
        uf = qu + cam1["cx"]
        vf = qv + cam1["cy"]
        ui = np.floor(uf + F(0.5))
        vi = np.floor(vf + F(0.5))
        kept = front & (ui >= F(0)) & (ui < F(cols)) & (vi >= F(0)) & (vi < F(rows))
    return kept, np.where(kept, vi, 0).astype(np.int64), np.where(kept, ui, 0).astype(np.int64), hz


def candidate(o, n_prev, n_cur, min_overlap, min_share):
    return int(o) >= min_overlap and 1024 * int(o) >= min_share * min(int(n_prev), int(n_cur))


def assign(O, n_prev, n_cur, min_overlap, min_share):
    """(prev_of_cur, cur_of_prev, matched): 1-based partners, 0 for none"""
    kp, k = len(n_prev), len(n_cur)
    O = np.asarray(O, np.int64).reshape(kp, k)
    cand = [(-int(O[t, c]), t, c) for t in range(kp) for c in range(k) if candidate(O[t, c], n_prev[t], n_cur[c], min_overlap, min_share)]
    cand.sort()
    prev_of_cur, cur_of_prev, matched = np.zeros(k, np.int32), np.zeros(kp, np.int32), 0
    for _, t, c in cand:
        if cur_of_prev[t] == 0 and prev_of_cur[c] == 0:
            cur_of_prev[t], prev_of_cur[c] = c + 1, t + 1
            matched += 1
    return prev_of_cur, cur_of_prev, matched


class Slot:
    """what a tracker keeps for one followed camera"""

    def __init__(self):
        self.frames, self.next_id, self.has_prev = 0, 1, False
        self.labels = self.depth = self.cam = None
        self.ids, self.births, self.counts = [], [], []

    def reset(self, restart_ids):
        self.has_prev, self.ids, self.births, self.counts = False, [], [], []
        if restart_ids:
            self.frames, self.next_id = 0, 1

    def info(self):
        return dict(frames=self.frames, next_id=self.next_id, n_tracks=len(self.ids) if self.has_prev else 0)


def overlap(slot, L, depth, cam, tp, K):
    """(O of shape (K_prev, K), n_warped) of a slot that holds a previous frame"""
    rows, cols = depth.shape
    kp = len(slot.ids)
    O = np.zeros((kp, K), np.int64)
    if kp == 0:
        return O, 0
    D = relative(slot.cam["pose"], cam["pose"])
    idx = np.nonzero(slot.labels > 0)[0]
    t = slot.labels[idx]
    kept, vi, ui, hz = warp(D, slot.cam, cam, idx % rows, idx // rows, slot.depth[idx], rows, cols)
    at = (vi + ui * rows)[kept]
    k = L.ravel(order="F")[at]
    zc = np.asarray(depth, F).ravel(order="F")[at]
    h = hz[kept]
    counts = (k >= 1) & (k <= K)
    if tp["use_depth_gate"]:
        with np.errstate(all="ignore"):
            diff = h - zc
            nearer = np.fmin(h, zc)
            rel = F(tp["dz_rel"]) * nearer
            bound = F(tp["dz_abs"]) + rel
            counts = counts & (np.abs(diff) <= bound)
    np.add.at(O, (t[kept][counts] - 1, k[counts] - 1), 1)
    return O, int(kept.sum())


def update(slot, depth, b, cam, rp, tp, max_tracks):
    """one update of `slot`: (summary record, max_tracks track records, (rows, cols) int32 id image, O); commits the slot"""
    depth = np.asarray(depth, F)
    rows, cols = depth.shape
    rsum, rrec, L = rr.label(depth, b, rp, max_tracks)
    R, K = int(rsum["n_regions"]), int(rsum["n_written"])
    kp = len(slot.ids) if slot.has_prev else 0
    O, n_warped = overlap(slot, L, depth, cam, tp, K) if slot.has_prev else (np.zeros((0, K), np.int64), 0)
    n_cur = [int(rrec["n"][c]) for c in range(K)]
    prev_of_cur, cur_of_prev, matched = assign(O, slot.counts[:kp], n_cur, tp["min_overlap"], tp["min_share"])
    trk = np.zeros(max_tracks, TRACK_DTYPE)
    next_id = slot.next_id
    for c in range(K):
        t = int(prev_of_cur[c])
        r = trk[c]
        if t:
            r["id"], r["birth_frame"], r["overlap"] = slot.ids[t - 1], slot.births[t - 1], O[t - 1, c]
        else:
            r["id"], r["birth_frame"], r["overlap"] = next_id, slot.frames, 0
            next_id += 1
        r["region"], r["prev_region"], r["age"] = c + 1, t, slot.frames - int(r["birth_frame"])
        for f in rr.REGION_FIELDS:
            r[f] = rrec[f][c]
    # the world-frame box and sums
    Lf = L.ravel(order="F").astype(np.int64)
    clipped = np.where((Lf >= 1) & (Lf <= K), Lf, 0)
    idx = np.nonzero(clipped)[0]
    if K:
        with np.errstate(all="ignore"):
            x, y, z = back_project(cam, idx % rows, idx // rows, depth.ravel(order="F")[idx])
            W = transform(cam["pose"], x, y, z)
            q = []
            for j in range(3):
                lo = np.fmax(W[j], F(-2048))
                cl = np.fmin(lo, F(2048))
                q.append(np.rint(cl * F(1024)).astype(np.int64))
        row = clipped[idx] - 1
        for j in range(3):
            lo, hi, total = np.full(K, np.iinfo(np.int64).max), np.full(K, np.iinfo(np.int64).min), np.zeros(K, np.int64)
            np.minimum.at(lo, row, q[j])
            np.maximum.at(hi, row, q[j])
            np.add.at(total, row, q[j])
            trk["qmin"][:K, j], trk["qmax"][:K, j], trk["sum_q"][:K, j] = lo, hi, total
    ids = np.zeros(rows * cols, np.int32)
    ids[idx] = trk["id"][clipped[idx] - 1]
    summ = np.zeros((), SUMMARY_DTYPE)
    for f, val in zip(SUMMARY_FIELDS, (R, K, matched, K - matched, kp - matched, R - K, n_warped, next_id)):
        summ[f] = val
    # commit
    slot.labels, slot.depth, slot.cam = clipped, depth.ravel(order="F").copy(), cam
    slot.ids, slot.births, slot.counts = [int(x) for x in trk["id"][:K]], [int(x) for x in trk["birth_frame"][:K]], n_cur
    slot.frames, slot.next_id, slot.has_prev = slot.frames + 1, next_id, True
    return summ, trk, ids.reshape(cols, rows).T.copy(), O
