"""A plain NumPy restatement of include/sf_deform.h: BIND, DEFORM, EDGES, the deformation of poses and the solver. It imports
nothing of the product. fp32 parts use float32 arrays elementwise (one rounding per operation, in the header's order); the
solver uses float64 and only + - * /. Ties of (d2, j) are settled by a stable sort over ascending j."""
import numpy as np

F = np.float32
D = np.float64
INF = F(np.inf)
COUNT_FIELDS = ("n_surfels", "n_bound", "n_unbound", "n_short")
DEFAULTS = dict(time_window=float("inf"))
SOLVE_DEFAULTS = dict(time_window=float("inf"), w_reg=1.0, damping=1e-6, iterations=8)
OK, DEGENERATE = 0, 2


def _f(a, shape):
    return np.ascontiguousarray(np.asarray(a, F).reshape(shape))


def bind(pos, times, window, P, tau, skip_self=False):
    """BIND of the n points P (n, 3) with times tau (n,): m (n,), idx (n, 4) (-1: missing), w (n, 4) (0: missing).
    skip_self: point q is node q and is left out of its own search (EDGES)."""
    pos, times, P, tau = _f(pos, (-1, 3)), _f(times, (-1,)), _f(P, (-1, 3)), _f(tau, (-1,))
    n, G = P.shape[0], pos.shape[0]
    window = F(window)
    with np.errstate(all="ignore"):
        dx = P[:, None, 0] - pos[None, :, 0]
        dy = P[:, None, 1] - pos[None, :, 1]
        dz = P[:, None, 2] - pos[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        ok = (d2 < INF) & (np.abs(times[None, :] - tau[:, None]) <= window)
        if skip_self:
            ok[np.arange(n), np.arange(n)] = False
        key = np.where(ok, d2, INF)
        order = np.argsort(key, axis=1, kind="stable")[:, :5]  # ineligible nodes sort behind every eligible one
        if order.shape[1] < 5:
            order = np.concatenate([order, np.zeros((n, 5 - order.shape[1]), order.dtype)], axis=1)
        E = np.minimum(ok.sum(axis=1), 5)
        held = np.arange(5)[None, :] < E[:, None]
        b_d2 = np.where(held, np.take_along_axis(key, np.minimum(order, G - 1), axis=1), INF).astype(F)
        b_j = np.where(held, order, -1).astype(np.int32)
        m = np.minimum(E, 4).astype(np.int32)
        idx = b_j[:, :4].copy()
        taken = np.arange(4)[None, :] < m[:, None]
        last = np.take_along_axis(b_d2, np.maximum(m - 1, 0)[:, None].astype(np.int64), axis=1)[:, 0]
        dmax2 = np.where(E > 4, b_d2[:, 4], F(4.0) * last).astype(F)
        smax = np.sqrt(dmax2)
        ratio = np.sqrt(b_d2[:, :4]) / smax[:, None]
        one_less = F(1.0) - ratio
        w = one_less * one_less
        w = np.where((dmax2 == 0)[:, None], F(1.0), w)
        w = np.where(taken, w, F(0.0)).astype(F)
        S = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
        flat = ~(S > 0)
        w = np.where(flat[:, None] & taken, F(1.0), w).astype(F)
        S = np.where(flat, m.astype(F), S).astype(F)
        w = np.where(taken, w / S[:, None], F(0.0)).astype(F)
    return m, idx, w


def blend(pos, M, m, idx, w, P, N):
    """the ascending sums of w_i * phi_i(P) and w_i * (A_i N) for the rows with m >= 1 (the others: zeros)"""
    pos, M = _f(pos, (-1, 3)), _f(M, (-1, 3, 4))
    P, N = _f(P, (-1, 3)), _f(N, (-1, 3))
    Po, No = np.zeros_like(P), np.zeros_like(N)
    with np.errstate(all="ignore"):
        for i in range(4):
            rows = np.nonzero(m > i)[0]
            if rows.size == 0:
                break
            j = idx[rows, i]
            g, A, t = pos[j], M[j, :, :3], M[j, :, 3]
            d = P[rows] - g
            wi = w[rows, i]
            for r in range(3):
                rot = (A[:, r, 0] * d[:, 0] + A[:, r, 1] * d[:, 1]) + A[:, r, 2] * d[:, 2]
                a = wi * ((rot + g[:, r]) + t[:, r])
                b = wi * ((A[:, r, 0] * N[rows, 0] + A[:, r, 1] * N[rows, 1]) + A[:, r, 2] * N[rows, 2])
                Po[rows, r] = a if i == 0 else Po[rows, r] + a
                No[rows, r] = b if i == 0 else No[rows, r] + b
    return Po, No


def unit(V):
    """(V / sqrtf(V . V) per row, the rows where that holds: 0 < V . V < inf)"""
    with np.errstate(all="ignore"):
        vv = (V[:, 0] * V[:, 0] + V[:, 1] * V[:, 1]) + V[:, 2] * V[:, 2]
        ok = (vv > 0) & (vv < INF)
        return (V / np.sqrt(vv)[:, None]).astype(F), ok


def deform(pos, times, M, window, surfels):
    """DEFORM of every surfel (n, 12): (the deformed surfels, m (n,))"""
    s = _f(surfels, (-1, 12)).copy()
    if s.shape[0] == 0:
        return s, np.zeros(0, np.int32)
    m, idx, w = bind(pos, times, window, s[:, 0:3], s[:, 6])
    Po, No = blend(pos, M, m, idx, w, s[:, 0:3], s[:, 8:11])
    U, ok = unit(No)
    bound = m > 0
    s[bound, 0:3] = Po[bound]
    turn = bound & ok
    s[turn, 8:11] = U[turn]
    return s, m


def counts(m):
    return dict(n_surfels=int(m.shape[0]), n_bound=int((m > 0).sum()), n_unbound=int((m == 0).sum()), n_short=int(((m > 0) & (m < 4)).sum()))


def edges(pos, times, window):
    pos, times = _f(pos, (-1, 3)), _f(times, (-1,))
    return bind(pos, times, window, pos, times, skip_self=True)[1]


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def deform_poses(pos, times, M, window, poses, taus):
    """POSE for n poses given as 4x4 (row, col): (n, 4, 4)"""
    T = np.asarray(poses, F).reshape(-1, 4, 4).copy()
    n = T.shape[0]
    if n == 0:
        return T
    origin = np.ascontiguousarray(T[:, :3, 3])
    m, idx, w = bind(pos, times, window, origin, taus)
    a = []
    Po = None
    for c in range(3):
        Po, Ac = blend(pos, M, m, idx, w, origin, np.ascontiguousarray(T[:, :3, c]))
        a.append(Ac)
    with np.errstate(all="ignore"):
        x, ok = unit(a[0])
        y, ok_y = unit((a[1] - _dot(x, a[1])[:, None] * x).astype(F))
        z, ok_z = unit(((a[2] - _dot(x, a[2])[:, None] * x) - _dot(y, a[2])[:, None] * y).astype(F))
    bound = m > 0
    turn = bound & ok & ok_y & ok_z
    for c, v in enumerate((x, y, z)):
        T[turn, :3, c] = v[turn]
    T[bound, :3, 3] = Po[bound]
    return T


# ---- the solver -----------------------------------------------------------------------------------------------------------
def _neg_cross(q):
    z = D(0.0)
    return np.array([[z, q[2], -q[1]], [-q[2], z, q[0]], [q[1], -q[0], z]], D)


def _rotate(R, d):
    return np.array([(R[r, 0] * d[0] + R[r, 1] * d[1]) + R[r, 2] * d[2] for r in range(3)], D)


class _State:
    pass


def _energy(s, accumulate):
    n = 6 * s.G
    if accumulate:
        s.H = np.zeros((n, n), D)
        s.b = np.zeros(n, D)
    energy = D(0.0)

    def add(wgt, res, nodes, J):
        nonlocal energy
        energy = energy + wgt * ((res[0] * res[0] + res[1] * res[1]) + res[2] * res[2])
        if not accumulate:
            return
        gi = np.concatenate([6 * j + np.arange(6) for j in nodes])
        ix = np.ix_(gi, gi)
        for r in range(3):
            Jr = J[r, :gi.shape[0]]
            s.H[ix] = s.H[ix] + wgt * np.outer(Jr, Jr)
            s.b[gi] = s.b[gi] + wgt * (Jr * res[r])

    eye = np.eye(3, dtype=D)
    for c in range(s.C):
        m = int(s.bm[c])
        if m == 0:
            continue
        J = np.zeros((3, 24), D)
        v = np.zeros(3, D)
        for i in range(m):
            j = int(s.bidx[c, i])
            wn = s.bw[c, i]
            d = s.src[c] - s.g[j]
            q = _rotate(s.R[j], d)
            K = _neg_cross(q)
            phi = (q + s.g[j]) + s.t[j]
            term = wn * phi
            v = term if i == 0 else v + term
            J[:, 6 * i:6 * i + 3] = wn * K
            J[:, 6 * i + 3:6 * i + 6] = wn * eye
        add(s.weight[c], v - s.dst[c], [int(k) for k in s.bidx[c, :m]], J)
    for j in range(s.G):
        for slot in range(4):
            k = int(s.edges[j, slot])
            if k < 0:
                continue
            q = _rotate(s.R[j], s.g[k] - s.g[j])
            res = (((q + s.g[j]) + s.t[j]) - s.g[k]) - s.t[k]
            J = np.zeros((3, 24), D)
            J[:, 0:3] = _neg_cross(q)
            J[:, 3:6] = eye
            J[:, 9:12] = np.where(eye == 1, D(-1.0), D(0.0))
            add(s.w_reg, res, [j, k], J)
    return energy


def _ldlt_solve(s, damping, floor_d):
    """x of (H + damping I) x = -b, or None for a refused pivot. Right-looking: pivot k is subtracted from what lies behind
    it, so every element loses the same terms in the same order as in the row-wise form."""
    A = s.H.copy()
    n = A.shape[0]
    A[np.arange(n), np.arange(n)] = A[np.arange(n), np.arange(n)] + damping
    L = np.zeros((n, n), D)
    d = np.zeros(n, D)
    for k in range(n):
        dk = A[k, k]
        if not (dk > floor_d):
            return None
        d[k] = dk
        col = A[k + 1:, k] / dk
        L[k + 1:, k] = col
        A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - np.outer(col, col) * dk
    z = np.zeros(n, D)
    for i in range(n):
        v = -s.b[i]
        for k in range(i):
            v = v - L[i, k] * z[k]
        z[i] = v
    x = np.zeros(n, D)
    for i in range(n - 1, -1, -1):
        v = z[i] / d[i]
        for k in range(i + 1, n):
            v = v - L[k, i] * x[k]
        x[i] = v
    return x


def _update(s, x):
    for j in range(s.G):
        xj = x[6 * j:6 * j + 6]
        a0, a1, a2 = D(0.5) * xj[0], D(0.5) * xj[1], D(0.5) * xj[2]
        aa = (a0 * a0 + a1 * a1) + a2 * a2
        sc = D(2.0) / (D(1.0) + aa)
        one = D(1.0)
        Q = np.array([[one - sc * (a1 * a1 + a2 * a2), sc * (a0 * a1 - a2), sc * (a0 * a2 + a1)],
                      [sc * (a0 * a1 + a2), one - sc * (a0 * a0 + a2 * a2), sc * (a1 * a2 - a0)],
                      [sc * (a0 * a2 - a1), sc * (a1 * a2 + a0), one - sc * (a0 * a0 + a1 * a1)]], D)
        R = s.R[j]
        out = np.zeros((3, 3), D)
        for r in range(3):
            for c in range(3):
                out[r, c] = (Q[r, 0] * R[0, c] + Q[r, 1] * R[1, c]) + Q[r, 2] * R[2, c]
        s.R[j] = out
        s.t[j] = s.t[j] + xj[3:6]


def solve(pos, times, src, dst, con_times, weights, M=None, time_window=float("inf"), w_reg=1.0, damping=1e-6, iterations=8):
    """SOLVE: (M (G, 3, 4) float32, dict(status, iterations_done, n_bound, n_unbound, energy))"""
    pos, times = _f(pos, (-1, 3)), _f(times, (-1,))
    G = pos.shape[0]
    M = np.tile(np.eye(3, 4, dtype=F), (G, 1, 1)) if M is None else _f(M, (-1, 3, 4)).copy()
    src, dst = _f(src, (-1, 3)), _f(dst, (-1, 3))
    s = _State()
    s.G, s.C = G, src.shape[0]
    con_times = np.broadcast_to(np.asarray(con_times, F), (s.C,))
    s.weight = np.broadcast_to(np.asarray(weights, F), (s.C,)).astype(D)
    s.src, s.dst = src.astype(D), dst.astype(D)
    s.g = pos.astype(D)
    s.R = M[:, :, :3].astype(D)
    s.t = M[:, :, 3].astype(D)
    s.edges = edges(pos, times, time_window)
    s.w_reg = D(F(w_reg))
    if s.C:
        s.bm, s.bidx, bw = bind(pos, times, time_window, src, con_times)
        s.bw = bw.astype(D)
    else:
        s.bm = np.zeros(0, np.int32)
    n_bound = int((s.bm > 0).sum())
    floor_d = D(1e-9) * D(n_bound + int((s.edges >= 0).sum()))
    damping = D(F(damping))
    energies, status, it = [], OK, 0
    with np.errstate(all="ignore"):
        while it < iterations:
            energies.append(_energy(s, True))
            x = _ldlt_solve(s, damping, floor_d)
            if x is None:
                status = DEGENERATE
                break
            _update(s, x)
            it += 1
        if status == OK:
            energies.append(_energy(s, False))
    out = np.zeros((G, 3, 4), F)
    out[:, :, :3] = s.R.astype(F)
    out[:, :, 3] = s.t.astype(F)
    return out, dict(status=status, iterations_done=it, n_bound=n_bound, n_unbound=s.C - n_bound, energy=np.array(energies, D))
