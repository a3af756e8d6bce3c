"""The definitions of include/sf_body_maps.h restated: the reference of the body map tests. np.float32 with one expression per
operation in the header's order (NumPy's + - * / and sqrt on float32 are correctly rounded, element by element the arithmetic of
the scalars); keys, ranks and the table rules are those of join_ref; winners by dictionaries. Images are (rows, cols) arrays,
cameras those of track_ref.camera, motions 4x4 (row, col). It imports neither the product nor the oracle."""
import numpy as np

import join_ref as jr
import track_ref as tr

F = np.float32
COUNT_FIELDS = ("n_pixels", "n_candidates", "n_voxels", "n_merged", "n_added", "n_conflict", "n_out")
DEFAULTS = dict(cell=0.01, z_max=8.0, normal_dz=0.05, min_dot=0.8, conf_new=0.1, gain=0.25, max_weight=32.0)
SQRT2 = F(1.41421356237)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1])


def _min(x, y):
    return np.where(y < x, y, x)


def _row(M, r, x, y, z, translate):
    """row r of the 4x4 (row, col) matrix M applied in the header's order"""
    a = M[r, 0] * x
    b = M[r, 1] * y
    c = M[r, 2] * z
    ab = a + b
    abc = ab + c
    return abc + M[r, 3] if translate else abc


def channel_byte(x):
    q = np.floor(x * F(255) + F(0.5))
    return np.where((q >= F(0)) & (q <= F(255)), q, F(0)).astype(np.int64)


def encode_colour(r, g, b):
    return ((channel_byte(r) << 16) + (channel_byte(g) << 8) + channel_byte(b)).astype(F)


def decode_colour(c):
    c = np.asarray(c, F)
    k = np.where((c >= F(0)) & (c < F(16777216)), c, F(0)).astype(np.int64)
    return ((k >> 16) & 255).astype(F) / F(255), ((k >> 8) & 255).astype(F) / F(255), (k & 255).astype(F) / F(255)


def pixel_surfels(depth, cam, colour, p, time, v0=0, u0=0):
    """PIXEL SURFEL of every pixel: (has (rows, cols) bool, S (rows, cols, 12) float32, zeros where has is false). The image's
    element (i, j) is pixel (v0 + i, u0 + j); only its interior can have surfels."""
    z = np.asarray(depth, F)
    rows, cols = z.shape
    has = np.zeros((rows, cols), bool)
    S = np.zeros((rows, cols, 12), F)
    if rows < 3 or cols < 3:
        return has, S
    zm, dz = F(p["z_max"]), F(p["normal_dz"])
    v, u = np.meshgrid(np.arange(rows) + v0, np.arange(cols) + u0, indexing="ij")
    pose = np.asarray(cam["pose"], F).reshape(4, 4)
    if colour is None:
        rgb = np.full((rows, cols, 3), 128, np.uint8)
    else:
        rgb = np.asarray(colour, np.uint8).reshape(rows, cols, 3)
    with np.errstate(all="ignore"):
        P = tr.back_project(cam, v, u, z)
        valid = (z > F(0)) & (z <= zm)
        c, l, r, up, dn = z[1:-1, 1:-1], z[1:-1, :-2], z[1:-1, 2:], z[:-2, 1:-1], z[2:, 1:-1]
        ok = valid[1:-1, 1:-1] & valid[1:-1, :-2] & valid[1:-1, 2:] & valid[:-2, 1:-1] & valid[2:, 1:-1]
        for zn in (l, r, up, dn):
            ok &= np.abs(zn - c) <= dz
        a = tuple(q[1:-1, 2:] - q[1:-1, :-2] for q in P)
        b = tuple(q[2:, 1:-1] - q[:-2, 1:-1] for q in P)
        cr = _cross(a, b)
        cc = _dot(cr, cr)
        ok &= (cc > F(0)) & (cc < F(np.inf))
        s = np.sqrt(cc)
        n = tuple(ck / s for ck in cr)
        Pc = tuple(q[1:-1, 1:-1] for q in P)
        focal = (cam["fx"] + cam["fy"]) / F(2)
        r0 = (Pc[2] / focal) * SQRT2
        radius = _min(F(2) * r0, r0 / np.abs(n[2]))
        out = np.zeros((rows - 2, cols - 2, 12), F)
        for k in range(3):
            out[..., k] = _row(pose, k, Pc[0], Pc[1], Pc[2], True)
            out[..., 8 + k] = _row(pose, k, n[0], n[1], n[2], False)
        out[..., 3] = F(p["conf_new"])
        ch = [rgb[1:-1, 1:-1, k].astype(F) / F(255) for k in range(3)]
        out[..., 4] = encode_colour(*ch)
        out[..., 5] = F(1)
        out[..., 6] = out[..., 7] = F(time)
        out[..., 11] = radius
        assert all(q.dtype == F for q in (cc, s, r0, radius, out))
    has[1:-1, 1:-1] = ok
    S[1:-1, 1:-1] = np.where(ok[..., None], out, F(0))
    return has, S


def pixel_surfel(depths, v, u, cam, colour, p, time):
    """the pixel surfel of the interior pixel (v, u) from depths = Z(v, u), Z(v, u - 1), Z(v, u + 1), Z(v - 1, u), Z(v + 1, u);
    None for a pixel without a normal"""
    d = np.asarray(depths, F)
    img = np.ones((3, 3), F)
    img[1, 1], img[1, 0], img[1, 2], img[0, 1], img[2, 1] = d
    rgb = None if colour is None else np.tile(np.asarray(colour, np.uint8).reshape(1, 1, 3), (3, 3, 1))
    has, S = pixel_surfels(img, cam, rgb, p, time, v0=v - 1, u0=u - 1)
    return S[1, 1].copy() if has[1, 1] else None


def move(surfels, W):
    """MOVE: every surfel's position and normal through W (4x4 (row, col); None: the identity, through the same arithmetic)"""
    s = np.ascontiguousarray(surfels, F).reshape(-1, 12)
    M = np.eye(4, dtype=F) if W is None else np.asarray(W, F).reshape(4, 4)
    out = s.copy()
    out[:, 0:3] = jr.transform_rows(M, s[:, 0:3], True)
    out[:, 8:11] = jr.transform_rows(M, s[:, 8:11], False)
    return out


def merge_surfel(s, q, p, time):
    """MERGE of the pixel surfel q into the (moved) map surfel s"""
    s, q = np.asarray(s, F).reshape(12), np.asarray(q, F).reshape(12)
    o = s.copy()
    with np.errstate(all="ignore"):
        w = np.fmin(s[5], F(p["max_weight"]))
        den = w + F(1)

        def blend(old, new):
            return ((w * old) + new) / den

        for k in (0, 1, 2, 11):
            o[k] = blend(s[k], q[k])
        n = [blend(s[8 + k], q[8 + k]) for k in range(3)]
        nn = _dot(n, n)
        if nn > F(0) and nn < F(np.inf):
            length = np.sqrt(nn)
            for k in range(3):
                o[8 + k] = n[k] / length
        cs, cq = decode_colour(s[4]), decode_colour(q[4])
        o[4] = encode_colour(*[blend(cs[k], cq[k]) for k in range(3)])
        c = s[3]
        o[3] = c + F(p["gain"]) * (F(1) - c)
        o[5] = s[5] + F(1)
        o[7] = F(time)
        assert all(isinstance(x, F) for x in (w, den, nn, o[3], o[5]))
    return o


def counts(**kw):
    c = dict.fromkeys(COUNT_FIELDS, 0)
    c.update(kw)
    return c


def table_slots(count, rows, cols):
    """the slots of an entry's table"""
    return jr.table_slots(count + max(rows - 2, 0) * max(cols - 2, 0))


def fuse(surfels, tick, depth, labels, cam, t, W=None, colour=None, p=None, detail=None):
    """one entry: (the map's surfels afterwards, counts). detail, a dict, gets `merged` (surfel index -> pixel (v, u)), `added` (the
    pixels in the order of the append) and `conflict` (pixels)."""
    p = params() if p is None else p
    time = F(tick)
    moved = move(surfels, W)
    labels = np.asarray(labels)
    rows, cols = labels.shape
    skeys, sinside = jr.voxel_keys(moved[:, 0:3], p["cell"])
    rk = jr.ranks(moved[:, 3])
    rep = {}  # key -> (rank, index): the highest rank, among equal ranks the lowest index
    for e in np.flatnonzero(sinside).tolist():
        k, r = int(skeys[e]), int(rk[e])
        if k not in rep or r > rep[k][0]:
            rep[k] = (r, e)
    has, S = pixel_surfels(depth, cam, colour, p, time)
    pkeys, pinside = jr.voxel_keys(S[..., 0:3].reshape(-1, 3), p["cell"])
    pkeys, pinside = pkeys.reshape(rows, cols), pinside.reshape(rows, cols)
    mine = labels == t
    cand = mine & has & pinside
    winners = {}  # key -> the candidate of lowest pixel index v + u * rows
    for u, v in zip(*np.nonzero(cand.T)):  # (ascending u, then v: ascending pixel index)
        winners.setdefault(int(pkeys[v, u]), (int(v), int(u)))
    out = moved.copy()
    merged, added, conflict = {}, [], []
    with np.errstate(all="ignore"):
        for k, (v, u) in sorted(winners.items(), key=lambda kv: kv[1][0] + kv[1][1] * rows):
            if k in rep:
                e = rep[k][1]
                d = _dot(moved[e, 8:11], S[v, u, 8:11])
                assert isinstance(d, F)
                if d >= F(p["min_dot"]):
                    merged[e] = (v, u)
                    out[e] = merge_surfel(moved[e], S[v, u], p, time)
                else:
                    conflict.append((v, u))
            else:
                added.append((v, u))
    if added:
        out = np.concatenate([out, np.stack([S[v, u] for v, u in added])])
    if detail is not None:
        detail.update(merged=merged, added=added, conflict=conflict)
    c = counts(n_pixels=int(mine.sum()), n_candidates=int(cand.sum()), n_voxels=len(rep), n_merged=len(merged), n_added=len(added), n_conflict=len(conflict),
               n_out=moved.shape[0] + len(added))
    return np.ascontiguousarray(out, F), c
