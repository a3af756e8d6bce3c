"""The definition of include/sf_align.h restated: the reference of the align tests. The pixel pass runs in np.float32, one
expression per operation in the header's order (NumPy's + - * / on float32 are correctly rounded, element by element the
arithmetic of the scalars), on top of the NumPy renderer of tests/view_ref.py; the sums are int64; the step runs in Python
floats (fp64, only + - * /). Images are (rows, cols) arrays. It imports neither the product nor the oracle."""
import copy

import numpy as np

import view_ref

F = np.float32
OK, FEW_PAIRS, DEGENERATE = 0, 1, 2
SYSTEM_DTYPE = np.dtype([("n", np.int64), ("ss", np.int64), ("g", np.int64, (6,)), ("H", np.int64, (21,)), ("reserved", np.int64, (3,))])
PAIRS = [(k, l) for k in range(6) for l in range(k, 6)]  # the order of H


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def system_words(ok, J, r):
    """the 32 int64 words of the system whose pairs are the elements with ok set: J the six float32 arrays of the row, r the
    float32 residual; a = rint(clamp(J, -64, 64) * 4096), rho = rint(r * 65536), the sums in int64 (align, bodies and register)"""
    with np.errstate(all="ignore"):
        a = [np.where(ok, np.rint(np.fmin(np.fmax(Jk, F(-64)), F(64)) * F(4096)), F(0)).astype(np.int64) for Jk in J]
        rho = np.where(ok, np.rint(r * F(65536)), F(0)).astype(np.int64)
    return [int(ok.sum()), int((rho * rho).sum())] + [int((ak * rho).sum()) for ak in a] + [int((a[k] * a[l]).sum()) for k, l in PAIRS] + [0, 0, 0]


def model_image(surfels, view, tick=1):
    """dict(drawn (rows, cols) bool, M and n: three (rows, cols) float32 planes each) of the map drawn from view"""
    surfels = np.ascontiguousarray(surfels, np.float32).reshape(-1, 12)
    v = copy.copy(view)
    v.shade = 0
    index = view_ref.render(surfels, v, tick=tick)["index"]  # (rows, cols), -1: not drawn
    with np.errstate(all="ignore"):
        c = view_ref._Ctx(v, tick)
        drawn = index >= 0
        q = surfels[np.maximum(index, 0)] if surfels.shape[0] else np.zeros(index.shape + (12,), np.float32)
        T = c.T
        x, y, z = q[..., 0], q[..., 1], q[..., 2]
        h = (((T[0] * x + T[4] * y) + T[8] * z) + T[12], ((T[1] * x + T[5] * y) + T[9] * z) + T[13], ((T[2] * x + T[6] * y) + T[10] * z) + T[14])
        nx, ny, nz = q[..., 8], q[..., 9], q[..., 10]
        n = view_ref._normalize(((T[0] * nx + T[4] * ny) + T[8] * nz, (T[1] * nx + T[5] * ny) + T[9] * nz, (T[2] * nx + T[6] * ny) + T[10] * nz))
        l = tuple(np.ascontiguousarray(r.T) for r in c.rays)  # the ray table is [i, j]
        t = _dot(h, n) / _dot(l, n)
        M = (l[0] * t, l[1] * t, l[2] * t)
    return dict(drawn=drawn, M=M, n=n)


def linearise(model, view, depth, b, params, D):
    """the 32 int64 words of the sfa_system at the estimate D (12 Python floats, row-major)"""
    rows, cols, stride = int(view.rows), int(view.cols), int(params.stride)
    cx, cy, fx, fy = F(view.cx), F(view.cy), F(view.fx), F(view.fy)
    Df = [F(v) for v in D]
    with np.errstate(all="ignore"):
        ys, xs = np.meshgrid(np.arange(0, rows, stride), np.arange(0, cols, stride), indexing="ij")
        zf = np.asarray(depth, np.float32)[ys, xs]
        ok = (zf > F(0)) & (zf <= F(params.z_max))
        if params.use_b:
            ok &= np.asarray(b, np.float32)[ys, xs] > F(params.b_min)
        P = (((xs.astype(np.float32) - cx) * zf) / fx, ((ys.astype(np.float32) - cy) * zf) / fy, zf)
        Q = tuple(((Df[4 * k] * P[0] + Df[4 * k + 1] * P[1]) + Df[4 * k + 2] * P[2]) + Df[4 * k + 3] for k in range(3))
        ok &= Q[2] >= F(0.4)
        px = (fx * Q[0]) / Q[2] + cx
        py = (fy * Q[1]) / Q[2] + cy
        ok &= (px >= F(0)) & (px < F(cols)) & (py >= F(0)) & (py < F(rows))
        i = np.where(ok, np.floor(px), F(0)).astype(np.int64)
        j = np.where(ok, np.floor(py), F(0)).astype(np.int64)
        ok &= model["drawn"][j, i]
        M = tuple(p[j, i] for p in model["M"])
        n = tuple(p[j, i] for p in model["n"])
        d = (Q[0] - M[0], Q[1] - M[1], Q[2] - M[2])
        ok &= _dot(d, d) <= F(params.dist_max) * F(params.dist_max)
        ok &= _dot(n, n) > F(0.5)
        r = _dot(n, d)
        ok &= np.abs(r) <= F(params.dist_max)
        c = (Q[1] * n[2] - n[1] * Q[2], Q[2] * n[0] - n[2] * Q[0], Q[0] * n[1] - n[0] * Q[1])
    return system_words(ok, c + n, r)


def step(w, damping, D):
    """STEP of the header: (status, D_out as 12 Python floats or None). w: 32 ints, D: 12 floats; fp64, only + - * /"""
    n = float(int(w[0]))
    A = [[0.0] * 6 for _ in range(6)]
    for idx, (k, l) in enumerate(PAIRS):
        v = float(int(w[8 + idx])) * (1.0 / 16777216.0)
        A[k][l] = v
        A[l][k] = v
    lam = float(F(damping)) * n
    bvec = [0.0] * 6
    for k in range(6):
        A[k][k] = A[k][k] + lam
        bvec[k] = -(float(int(w[2 + k])) * (1.0 / 268435456.0))
    floor_d = 1e-9 * n
    L = [[0.0] * 6 for _ in range(6)]
    d = [0.0] * 6
    for j in range(6):
        s = A[j][j]
        for k in range(j):
            s = s - (L[j][k] * L[j][k]) * d[k]
        if not s > floor_d:
            return DEGENERATE, None
        d[j] = s
        for i in range(j + 1, 6):
            t = A[i][j]
            for k in range(j):
                t = t - (L[i][k] * L[j][k]) * d[k]
            L[i][j] = _div(t, s)
    z = [0.0] * 6
    for i in range(6):
        t = bvec[i]
        for k in range(i):
            t = t - L[i][k] * z[k]
        z[i] = t
    x = [0.0] * 6
    for i in range(5, -1, -1):
        t = _div(z[i], d[i])
        for k in range(i + 1, 6):
            t = t - L[k][i] * x[k]
        x[i] = t
    R = cayley(x[0], x[1], x[2])
    out = [0.0] * 12
    for k in range(3):
        for c in range(4):
            v = (R[k][0] * D[c] + R[k][1] * D[4 + c]) + R[k][2] * D[8 + c]
            if c == 3:
                v = v + x[3 + k]
            out[4 * k + c] = v
    return OK, out


def _div(a, b):
    """a / b as the hardware divides: inf and NaN instead of Python's exceptions"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def cayley(w0, w1, w2):
    a0, a1, a2 = 0.5 * w0, 0.5 * w1, 0.5 * w2
    aa = (a0 * a0 + a1 * a1) + a2 * a2
    s = _div(2.0, 1.0 + aa)
    return [[1.0 - s * (a1 * a1 + a2 * a2), s * (a0 * a1 - a2), s * (a0 * a2 + a1)],
            [s * (a0 * a1 + a2), 1.0 - s * (a0 * a0 + a2 * a2), s * (a1 * a2 - a0)],
            [s * (a0 * a2 - a1), s * (a1 * a2 + a0), 1.0 - s * (a0 * a0 + a1 * a1)]]


def compose_pose(pose16, D):
    """pose = T0 * D rounded to float, column-major"""
    t0 = [float(F(v)) for v in pose16]
    out = np.zeros(16, np.float32)
    with np.errstate(all="ignore"):
        for r in range(4):
            for c in range(4):
                v = (t0[r] * D[c] + t0[r + 4] * D[4 + c]) + t0[r + 8] * D[8 + c]
                if c == 3:
                    v = v + t0[r + 12]
                out[r + 4 * c] = np.float64(v).astype(np.float32)
    return out


def refine(surfels, view, depth, b=None, params=None, tick=1, slots=None, model=None):
    """(result dict, (slots, 32) int64 array of systems) of one (map, view, frame) entry; slots: I + 1 of the call, at least
    params.iterations + 1; params: anything with the members of sfa_params"""
    K = int(params.iterations)
    slots = K + 1 if slots is None else slots
    if model is None:
        model = model_image(surfels, view, tick)
    systems = np.zeros((slots, 32), np.int64)
    D = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    status, done, it = OK, 0, 0
    while True:
        w = linearise(model, view, depth, b, params, D)
        systems[it] = w
        if it == 0:
            first = (w[0], w[1])
        if it == K:
            break
        if w[0] < int(params.min_pairs):
            status = FEW_PAIRS
            break
        code, Dn = step(w, params.damping, D)
        if code != OK:
            status = DEGENERATE
            break
        D = Dn
        done = it = it + 1
    res = dict(pose=compose_pose(view.pose[:], D), status=status, iterations_done=done, n_first=first[0], ss_first=first[1], n_last=w[0], ss_last=w[1])
    return res, systems


def as_words(record):
    """a record of SYSTEM_DTYPE (the product's has the same layout) as 32 ints"""
    return [int(v) for v in np.asarray(record).reshape(1).view(np.int64)]
