"""The definitions of include/sf_bodies.h in NumPy / Python: the reference of the body tests. The pixel passes -- the target
model of frame 1 and the linearisation of every region -- run in np.float32, one expression per operation in the header's order
(NumPy's + - * / and sqrt on float32 are correctly rounded, element by element the arithmetic of the scalars); the sums are
int64; the step (align_ref.step) and the world motion run in Python floats (fp64, only + - * /). Images are (rows, cols)
arrays, cameras those of track_ref.camera. It imports neither the product nor the oracle."""
import numpy as np

import align_ref as ar
import track_ref as tr

F = np.float32
OK, FEW_PAIRS, DEGENERATE = ar.OK, ar.FEW_PAIRS, ar.DEGENERATE
SYSTEM_DTYPE = ar.SYSTEM_DTYPE
MOTION_DTYPE = np.dtype([("d", np.float32, (16,)), ("w", np.float32, (16,)), ("status", np.int32), ("iterations_done", np.int32), ("n_first", np.int64),
                         ("ss_first", np.int64), ("n_last", np.int64), ("ss_last", np.int64), ("reserved", np.int64, (3,))])
DEFAULTS = dict(dist_max=0.10, z_max=8.0, normal_dz=0.05, damping=0.0, iterations=10, min_pairs=64)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1])


def model(depth1, labels1, cam1, p):
    """TARGET MODEL: dict(has (rows, cols) bool, P and n: three (rows, cols) float32 planes each, label (rows, cols) int64)"""
    z = np.asarray(depth1, F)
    rows, cols = z.shape
    zm, dz = F(p["z_max"]), F(p["normal_dz"])
    has = np.zeros((rows, cols), bool)
    n = [np.zeros((rows, cols), F) for _ in range(3)]
    v, u = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    with np.errstate(all="ignore"):
        P = tr.back_project(cam1, v, u, z)
        if rows >= 3 and cols >= 3:
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
            for k in range(3):
                n[k][1:-1, 1:-1] = np.where(ok, cr[k] / s, F(0))
            has[1:-1, 1:-1] = ok
    lab = np.zeros((rows, cols), np.int64) if labels1 is None else np.asarray(labels1).astype(np.int64)
    return dict(has=has, P=P, n=tuple(n), label=lab)


def linearise(mdl, depth0, labels0, cam0, cam1, p, t, want, D):
    """the 32 int64 words of the system of region t at the estimate D (12 Python floats, row-major); want: pairs[t - 1]"""
    z0 = np.asarray(depth0, F)
    rows, cols = z0.shape
    Df = [F(x) for x in D]
    v, u = np.nonzero(np.asarray(labels0) == t)
    z = z0[v, u]
    with np.errstate(all="ignore"):
        ok = (z > F(0)) & (z <= F(p["z_max"]))
        P = tr.back_project(cam0, v, u, z)
        Q = tuple(((Df[4 * k] * P[0] + Df[4 * k + 1] * P[1]) + Df[4 * k + 2] * P[2]) + Df[4 * k + 3] for k in range(3))
        ok &= Q[2] > F(0)
        nu = cam1["fx"] * Q[0]
        nv = cam1["fy"] * Q[1]
        uf = nu / Q[2] + cam1["cx"]
        vf = nv / Q[2] + cam1["cy"]
        ui = np.floor(uf + F(0.5))
        vi = np.floor(vf + F(0.5))
        ok &= (ui >= F(0)) & (ui < F(cols)) & (vi >= F(0)) & (vi < F(rows))
        i = np.where(ok, ui, F(0)).astype(np.int64)
        j = np.where(ok, vi, F(0)).astype(np.int64)
        ok &= mdl["has"][j, i]
        if want != 0:
            ok &= mdl["label"][j, i] == want
        M = tuple(q[j, i] for q in mdl["P"])
        n = tuple(q[j, i] for q in mdl["n"])
        d = (Q[0] - M[0], Q[1] - M[1], Q[2] - M[2])
        ok &= _dot(d, d) <= F(p["dist_max"]) * F(p["dist_max"])
        r = _dot(n, d)
        ok &= np.abs(r) <= F(p["dist_max"])
        J = _cross(Q, n) + n
    return ar.system_words(ok, J, r)


def world_motion(pose0, pose1, D):
    """WORLD MOTION: 16 float32, column-major, from two 4x4 (row, col) poses and D (12 Python floats); None for a NaN or inf"""
    p0, p1 = np.asarray(pose0, F).reshape(4, 4), np.asarray(pose1, F).reshape(4, 4)
    D = [float(x) for x in D]
    if not (np.isfinite(p0).all() and np.isfinite(p1).all() and np.isfinite(D).all()):
        return None
    T0 = [[float(p0[r, c]) for c in range(4)] for r in range(4)]
    T1 = [[float(p1[r, c]) for c in range(4)] for r in range(4)]
    w = np.zeros(16, F)
    with np.errstate(all="ignore"):
        for r in range(3):
            A = []
            for c in range(4):
                val = (T1[r][0] * D[c] + T1[r][1] * D[4 + c]) + T1[r][2] * D[8 + c]
                if c == 3:
                    val = val + T1[r][3]
                A.append(val)
            W = [(A[0] * T0[c][0] + A[1] * T0[c][1]) + A[2] * T0[c][2] for c in range(3)]
            for c in range(3):
                w[r + 4 * c] = np.float64(W[c]).astype(F)
            back = (W[0] * T0[0][3] + W[1] * T0[1][3]) + W[2] * T0[2][3]
            w[r + 12] = np.float64(A[3] - back).astype(F)
    w[15] = F(1)
    return w


def as_4x4(D):
    """D as the 16 float32 of a column-major 4 x 4 with last row 0 0 0 1"""
    d = np.zeros(16, F)
    with np.errstate(all="ignore"):
        for k in range(3):
            for c in range(4):
                d[k + 4 * c] = np.float64(D[4 * k + c]).astype(F)
    d[15] = F(1)
    return d


def start(cam0, cam1):
    """D0: the relative transform of the two poses as 12 Python floats, row-major"""
    rel = tr.relative(cam0["pose"], cam1["pose"])
    return [float(rel[k, c]) for k in range(3) for c in range(4)]


def estimate(depth0, labels0, depth1, labels1, cam0, cam1, K, pairs=None, p=None, max_regions=8, slots=None, trace=None):
    """one entry: (max_regions records of MOTION_DTYPE, (max_regions, slots, 32) int64 systems); slots: I + 1 of the call, at
    least iterations + 1. trace, a list, gets (t, it, D) of every linearisation."""
    p = params() if p is None else p
    its = int(p["iterations"])
    slots = its + 1 if slots is None else slots
    out = np.zeros(max_regions, MOTION_DTYPE)
    systems = np.zeros((max_regions, slots, 32), np.int64)
    if K == 0:
        return out, systems
    mdl = model(depth1, labels1, cam1, p)
    for t in range(1, K + 1):
        want = 0 if pairs is None else int(pairs[t - 1])
        D = start(cam0, cam1)
        status, done, it = OK, 0, 0
        while True:
            w = linearise(mdl, depth0, labels0, cam0, cam1, p, t, want, D)
            if trace is not None:
                trace.append((t, it, list(D)))
            systems[t - 1, it] = w
            if it == 0:
                first = (w[0], w[1])
            if it == its:
                break
            if w[0] < int(p["min_pairs"]):
                status = FEW_PAIRS
                break
            code, Dn = ar.step(w, p["damping"], D)
            if code != OK:
                status = DEGENERATE
                break
            D = Dn
            done = it = it + 1
        r = out[t - 1]
        r["d"], r["w"] = as_4x4(D), world_motion(cam0["pose"], cam1["pose"], D)
        r["status"], r["iterations_done"] = status, done
        r["n_first"], r["ss_first"], r["n_last"], r["ss_last"] = first[0], first[1], w[0], w[1]
    return out, systems
