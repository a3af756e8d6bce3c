"""The definition of include/sf_register.h restated: the reference of the register tests. The surfel pass runs in np.float32, one
expression per operation in the header's order (NumPy's + - * / and sqrt on float32 are correctly rounded, element by element
the arithmetic of the scalars); the table is a dictionary from voxel key to representative (tests/join_ref.py: keys and ranks);
the sums are int64; the step is that of tests/align_ref.py (fp64, only + - * /). It imports neither the product nor the oracle."""
import numpy as np

import align_ref
import join_ref

F = np.float32
OK, FEW_PAIRS, DEGENERATE = 0, 1, 2
NOT_PAIRED, NOT_SAMPLED = -1, -2
SYSTEM_DTYPE = align_ref.SYSTEM_DTYPE
DEFAULTS = dict(cell=0.1, dist_max=0.05, min_cos=0.5, min_confidence=0.0, damping=0.0, iterations=10, stride=1, min_pairs=64)
IDENTITY = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]


class Params:
    """the members of sfg_params"""

    def __init__(self, **kw):
        vars(self).update(DEFAULTS)
        assert set(kw) <= set(DEFAULTS), kw
        vars(self).update(kw)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def table(dst, cell):
    """TABLE: voxel key -> index of its representative: the highest rank, among equal ranks the lowest index"""
    d = np.ascontiguousarray(dst, np.float32).reshape(-1, 12)
    keys, inside = join_ref.voxel_keys(d[:, 0:3], cell)
    rk = join_ref.ranks(d[:, 3])
    best = {}
    for e in np.flatnonzero(inside).tolist():
        k, r = int(keys[e]), int(rk[e])
        if k not in best or r > best[k][0]:
            best[k] = (r, e)
    return {k: e for k, (_, e) in best.items()}


def _unit(v):
    """(exists, the three components of v / sqrt(v . v))"""
    vv = _dot(v, v)
    ok = (vv > F(0)) & (vv < F(np.inf))
    ln = np.sqrt(np.where(ok, vv, F(1)))
    assert ln.dtype == np.float32
    return ok, (v[0] / ln, v[1] / ln, v[2] / ln)


def linearise(dst, src, params, E, tab=None):
    """(the 32 int64 words of the system at the estimate E (12 Python floats, row-major), n_sampled, n_outside, the pairs)"""
    d = np.ascontiguousarray(dst, np.float32).reshape(-1, 12)
    s = np.ascontiguousarray(src, np.float32).reshape(-1, 12)
    if tab is None:
        tab = table(d, params.cell)
    inv = join_ref.inverse_cell(params.cell)
    Ef = [F(v) for v in E]
    count = s.shape[0]
    pairs = np.full(count, NOT_SAMPLED, np.int32)
    with np.errstate(all="ignore"):
        sampled = np.arange(count) % int(params.stride) == 0
        if F(params.min_confidence) > 0:
            sampled &= s[:, 3] >= F(params.min_confidence)
        idx = np.flatnonzero(sampled)
        p = (s[idx, 0], s[idx, 1], s[idx, 2])
        m = (s[idx, 8], s[idx, 9], s[idx, 10])
        Q = tuple(((Ef[4 * k] * p[0] + Ef[4 * k + 1] * p[1]) + Ef[4 * k + 2] * p[2]) + Ef[4 * k + 3] for k in range(3))
        mm = tuple((Ef[4 * k] * m[0] + Ef[4 * k + 1] * m[1]) + Ef[4 * k + 2] * m[2] for k in range(3))
        sc = tuple(q * inv for q in Q)
        f = tuple(np.floor(x) for x in sc)
        inside = np.ones(idx.size, bool)
        for k in range(3):
            inside &= np.isfinite(Q[k]) & np.isfinite(f[k]) & (np.abs(f[k]) < join_ref.Q_LIMIT)
        side = tuple(np.where(sc[k] - f[k] < F(0.5), -1, 1).astype(np.int64) for k in range(3))
        cell_i = tuple(np.where(inside, f[k], F(0)).astype(np.int64) for k in range(3))
        partner = np.full(idx.size, -1, np.int64)
        dd = np.zeros(idx.size, np.float32)
        for a in (0, 1):
            for b in (0, 1):
                for c in (0, 1):
                    q = (cell_i[0] + a * side[0], cell_i[1] + b * side[1], cell_i[2] + c * side[2])
                    in_grid = inside & (np.abs(q[0]) < (1 << 20)) & (np.abs(q[1]) < (1 << 20)) & (np.abs(q[2]) < (1 << 20))
                    keys = ((q[0] + (1 << 20)) << 42) | ((q[1] + (1 << 20)) << 21) | (q[2] + (1 << 20))
                    rep = np.array([tab.get(int(k), -1) if g else -1 for k, g in zip(keys.tolist(), in_grid.tolist())], np.int64).reshape(-1)
                    has = rep >= 0
                    M = d[np.maximum(rep, 0)] if d.shape[0] else np.zeros((idx.size, 12), np.float32)
                    e = (Q[0] - M[:, 0], Q[1] - M[:, 1], Q[2] - M[:, 2])
                    ee = _dot(e, e)
                    take = has & ((partner < 0) | (ee < dd))
                    partner = np.where(take, rep, partner)
                    dd = np.where(take, ee, dd)
        ok = partner >= 0                                                    # 1
        P = d[np.maximum(partner, 0)] if d.shape[0] else np.zeros((idx.size, 12), np.float32)
        if F(params.min_confidence) > 0:
            ok &= P[:, 3] >= F(params.min_confidence)                        # 2
        ok &= dd <= F(params.dist_max) * F(params.dist_max)                  # 3
        dv = (Q[0] - P[:, 0], Q[1] - P[:, 1], Q[2] - P[:, 2])
        n_ok, n = _unit((P[:, 8], P[:, 9], P[:, 10]))
        ok &= n_ok                                                           # 4
        m_ok, mn = _unit(mm)
        ok &= m_ok                                                           # 5
        ok &= _dot(mn, n) >= F(params.min_cos)                               # 6
        r = _dot(n, dv)
        ok &= np.abs(r) <= F(params.dist_max)                                # 7
        cr = (Q[1] * n[2] - n[1] * Q[2], Q[2] * n[0] - n[2] * Q[0], Q[0] * n[1] - n[0] * Q[1])
        for x in (dd, r) + Q + mm + n + mn:
            assert x.dtype == np.float32
    pairs[idx] = np.where(ok, partner, NOT_PAIRED).astype(np.int32)
    return align_ref.system_words(ok, cr + n, r), int(idx.size), int((~inside).sum()), pairs


def start(T0):
    """E0 from a 4 x 4 matrix (None: the identity): 12 Python floats, row-major"""
    if T0 is None:
        return list(IDENTITY)
    M = np.asarray(T0, np.float32).reshape(4, 4)
    return [float(M[k, c]) for k in range(3) for c in range(4)]


def result_T(E):
    """T of the result: E rounded to float, column-major, last row 0 0 0 1"""
    T = np.zeros(16, np.float32)
    with np.errstate(all="ignore"):
        for k in range(3):
            for c in range(4):
                T[k + 4 * c] = np.float64(E[4 * k + c]).astype(np.float32)
    T[15] = 1
    return T


def register(dst, src, T0=None, params=None, slots=None, tab=None):
    """(result dict, (slots, 32) int64 array of systems, the pairs of the last linearisation, E) of one entry; slots: I + 1 of
    the call, at least params.iterations + 1"""
    params = Params() if params is None else params
    K = int(params.iterations)
    slots = K + 1 if slots is None else slots
    d = np.ascontiguousarray(dst, np.float32).reshape(-1, 12)
    if tab is None:
        tab = table(d, params.cell)
    systems = np.zeros((slots, 32), np.int64)
    E = start(T0)
    status, done, it = OK, 0, 0
    while True:
        w, n_sampled, n_outside, pairs = linearise(d, src, params, E, tab)
        systems[it] = w
        if it == 0:
            first = (w[0], w[1])
        if it == K:
            break
        if w[0] < int(params.min_pairs):
            status = FEW_PAIRS
            break
        code, En = align_ref.step(w, params.damping, E)
        if code != align_ref.OK:
            status = DEGENERATE
            break
        E = En
        done = it = it + 1
    res = dict(T=result_T(E), status=status, iterations_done=done, n_first=first[0], ss_first=first[1], n_last=w[0], ss_last=w[1], n_sampled=n_sampled,
               n_outside=n_outside)
    return res, systems, pairs, E
