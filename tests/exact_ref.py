"""Exact (fp64) references of the warp splat, the IRLS normal equations, the 6 x 6 solve, the velocity filter and the SE(3)
update -- each recomputed from the inputs the implementation under test gave that stage, and each returned together with the
rounding bound a correct float implementation must meet (tests/test_exact_references.py) -- and, section D, of the stages
between the warp and the rows: calculateCoord, the gradients, the pre-weights, the Jacobian rows and the segmentation prior
(tests/test_exact_linearisation.py).

Plain NumPy. Nothing here imports oracle/ or the product: the point is an answer that neither of them wrote.

Conventions: images are (rows, cols) arrays as the bindings return them; "column-major" pixel order is the reference's
validPixels order (u outer, v inner); 4 x 4 transforms are (row, col) float64 matrices.
"""
import numpy as np

U32 = 2.0 ** -24  # unit roundoff of float32 (round to nearest)
FIX_DEPTH_Q = 2.0 ** -26   # resolution of the fixed-point depth sums (sf_device_common.h: FIX_DEPTH)
FIX_INTENS_Q = 2.0 ** -28  # ... and of the intensity sums (FIX_INTENS)


def gamma(n, u=U32):
    """Higham's gamma_n = n u / (1 - n u): the relative bound of n successive float roundings."""
    n = np.asarray(n, dtype=np.float64)
    return n * u / (1.0 - n * u)


def ulp32(x):
    """ulp of the float32 values nearest to x (>= the smallest subnormal)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def cm_to_mat(T16):
    """16 floats in column-major storage (sf_outer_trace::T) -> (row, col) float64 matrix"""
    return np.asarray(T16, dtype=np.float64).reshape(4, 4).T.copy()


# --------------------------------------------------------------------------------------------------------------------------
#  A. warpImagesAccurateInverse (reference FrontEnd.cpp:775-892) from the source planes the implementation used
# --------------------------------------------------------------------------------------------------------------------------
def warp_geometry(rows, cols, tan_half_fovh):
    """f, disp_u, disp_v in float32 as every implementation evaluates them (FrontEnd.cpp:795-798)"""
    f = np.float32(cols) / (np.float32(2.0) * np.float32(tan_half_fovh))
    return float(f), float(np.float32(0.5) * np.float32(cols - 1)), float(np.float32(0.5) * np.float32(rows - 1))


def _taps(uw, vw):
    """The reference's taps (FrontEnd.cpp:821-867) of integer centi-pixel positions (arrays, all accepted):
    (rows, cols, weights) each of shape (4, n); a snapped source has its weight-200 tap in slot 0 and zero weight elsewhere."""
    qu, ru = uw // 100, uw % 100
    qv, rv = vw // 100, vw % 100
    d_l, d_r, d_d, d_u = ru, 100 - ru, rv, 100 - rv
    snap = (np.minimum(d_r, d_l) + np.minimum(d_u, d_d)) < 5
    tv = np.stack([qv + 1, qv + 1, qv, qv])
    tu = np.stack([qu + 1, qu, qu + 1, qu])
    w = np.stack([d_l + d_d, d_r + d_d, d_l + d_u, d_r + d_u])
    tv[0] = np.where(snap, np.where(d_u > d_d, qv, qv + 1), tv[0])
    tu[0] = np.where(snap, np.where(d_r > d_l, qu, qu + 1), tu[0])
    w[0] = np.where(snap, 200, w[0])
    w[1:] = np.where(snap[None, :], 0, w[1:])
    return tv, tu, w


def warp_reference(depth, intensity, xx, yy, T_odometry, tan_half_fovh):
    """Exact warp of the source planes (depth, intensity, xx, yy: the PRED planes of one level) by T_odometry^-1.

    The implementation evaluates, per source pixel, in float32 (FMA contraction allowed):
        x_w = t00 xx + t01 yy + t02 z + t03   (y_w, depth_w alike)         t = float32(inv(T)): double Gauss-Jordan, rounded
        U = 100 (f x_w / depth_w + disp_u),  uwarp = trunc(U)              (V, vwarp alike)
    and splats with integer weights. This function evaluates the same expressions in fp64 on the same float32 inputs and bounds
    how far the float32 evaluation can be from them (u = 2^-24):
      * t: the implementation's entries may differ from float32(inv_fp64(T)) by 1 ulp <= 2u |t|  (its Gauss-Jordan in double
        rounds to the same float unless the double result sits within 1e-16 of a rounding boundary);
      * a 4-term affine sum with 4 roundings in any order / contraction: |err| <= gamma_4 S, S = sum |t_k x_k| (+ 2u S for t):
            e_x = (gamma_4 + 2u) S_x,  e_d = (gamma_4 + 2u) S_d;
      * f x_w / depth_w: |f x^/d^ - f x/d| <= f e_x / (|d| - e_d) + f |x| e_d / (|d| (|d| - e_d)), plus the rounding of the
        product and of the quotient (2u |Q|) and a 1-ulp difference of f itself (tan in another libm: 2u |Q|)  -> e_Q;
      * + disp: u |P| more (P = Q + disp), x 100: u 100 |P| more:  e_U = 100 (e_Q + u |P|) + 100 u |P|.
    The second-order terms (products of two u-sized errors) are covered by a factor 1 + 1e-3. A source whose trunc(U +- e_U)
    or trunc(V +- e_V) differ is AMBIGUOUS: every cell any of its candidate positions reaches is left unchecked.

    Returns a dict of (rows, cols) arrays: `w` (exact integer weight sums of the unambiguous sources), `depth`, `intensity` (exact
    quotients), `checked`, the per-cell bound terms `e_depth` (sum w e_d / sum w), `abs_depth` / `abs_intensity` (sum |w v| / sum
    w), `count` (contributions), and scalars: `n_sources`, `n_ambiguous`, `max_depth_w`, `min_depth_w_margin` (min depth_w - e_d),
    `max_count`; `sums` (the raw sums of the unambiguous sources) and `ambiguous` (per ambiguous source: candidate ranges, exact
    position, warped depth, intensity, e_d) for section E. Use `warp_bounds` for the tolerance of a given summation path.
    """
    rows, cols = depth.shape
    f, disp_u, disp_v = warp_geometry(rows, cols, tan_half_fovh)
    Ti = np.linalg.inv(np.asarray(T_odometry, dtype=np.float64)).astype(np.float32).astype(np.float64)
    # sources in column-major order (the reference's loop order; it matters for nothing but is kept for reading)
    z = np.asarray(depth, np.float32).T.ravel().astype(np.float64)
    sel = z != 0.0
    ii = np.asarray(intensity, np.float32).T.ravel().astype(np.float64)[sel]
    xr = np.asarray(xx, np.float32).T.ravel().astype(np.float64)[sel]
    yr = np.asarray(yy, np.float32).T.ravel().astype(np.float64)[sel]
    z = z[sel]
    src = np.stack([xr, yr, z, np.ones_like(z)])
    X, Y, D = (Ti[r] @ src for r in range(3))
    S = [np.abs(Ti[r])[:, None] * np.abs(src) for r in range(3)]
    S = [s.sum(0) for s in S]
    c_aff = gamma(4) + 2 * U32
    e_x, e_y, e_d = (c_aff * s + 4e-16 * s for s in S)
    assert np.all(D - e_d > 0), "a source lands on or behind the camera plane: outside this reference's preconditions"
    Dm = D - e_d

    def centi(N, e_n, disp):
        Q = f * N / D
        e_q = f * e_n / Dm + f * np.abs(N) * e_d / (np.abs(D) * Dm) + 4 * U32 * np.abs(Q)
        P = Q + disp
        e_u = 100.0 * (e_q + U32 * np.abs(P)) + 100.0 * U32 * np.abs(P)
        return 100.0 * P, e_u * (1.0 + 1e-3) + 1e-9

    Uc, e_U = centi(X, e_x, disp_u)
    Vc, e_V = centi(Y, e_y, disp_v)
    u_lo, u_hi = np.trunc(Uc - e_U), np.trunc(Uc + e_U)
    v_lo, v_hi = np.trunc(Vc - e_V), np.trunc(Vc + e_V)
    ambiguous = (u_lo != u_hi) | (v_lo != v_hi)
    cols_lim, rows_lim = 100 * (cols - 1), 100 * (rows - 1)

    def accepted(uw, vw):
        return (uw >= 0) & (uw < cols_lim) & (vw >= 0) & (vw < rows_lim)

    shape = (rows, cols)
    W = np.zeros(shape, np.int64)
    SD = np.zeros(shape)
    SI = np.zeros(shape)
    SE = np.zeros(shape)
    CNT = np.zeros(shape, np.int64)
    unchecked = np.zeros(shape, bool)

    ok = ~ambiguous
    uw, vw = u_lo[ok].astype(np.int64), v_lo[ok].astype(np.int64)
    acc = accepted(uw, vw)
    tv, tu, w = _taps(uw[acc], vw[acc])
    d_k, i_k, e_k = D[ok][acc], ii[ok][acc], e_d[ok][acc]
    for t in range(4):
        m = w[t] > 0
        np.add.at(W, (tv[t][m], tu[t][m]), w[t][m])
        np.add.at(SD, (tv[t][m], tu[t][m]), w[t][m] * d_k[m])
        np.add.at(SI, (tv[t][m], tu[t][m]), w[t][m] * i_k[m])
        np.add.at(SE, (tv[t][m], tu[t][m]), w[t][m] * e_k[m])
        np.add.at(CNT, (tv[t][m], tu[t][m]), 1)
    # every cell an ambiguous source could reach, over all its candidate centi-pixel positions
    amb = np.nonzero(ambiguous)[0]
    for k in amb:
        for a in range(int(u_lo[k]), int(u_hi[k]) + 1):
            for b in range(int(v_lo[k]), int(v_hi[k]) + 1):
                if accepted(a, b):
                    tv1, tu1, w1 = _taps(np.array([a]), np.array([b]))
                    for t in range(4):
                        if w1[t, 0] > 0:
                            unchecked[tv1[t, 0], tu1[t, 0]] = True
    touched = W > 0
    Wd = np.where(touched, W, 1).astype(np.float64)
    return dict(
        w=W, depth=np.where(touched, SD / Wd, 0.0), intensity=np.where(touched, SI / Wd, 0.0), checked=~unchecked,
        e_depth=SE / Wd, abs_depth=np.abs(SD) / Wd, abs_intensity=np.abs(SI) / Wd, count=CNT,
        n_sources=int(sel.sum()), n_ambiguous=int(ambiguous.sum()),
        max_depth_w=float(D.max()) if D.size else 0.0, min_depth_w_margin=float(Dm.min()) if D.size else np.inf,
        min_intensity=float(ii.min()) if ii.size else 0.0, max_intensity=float(ii.max()) if ii.size else 0.0,
        max_count=int(CNT.max()),
        # for section E, which has to carry the ambiguous sources through a sum instead of leaving their cells out: the raw sums of
        # the unambiguous sources, and per ambiguous source its candidate centi-pixel ranges, its exact position and its values
        sums=dict(w=W, depth=SD, intensity=SI, e_depth=SE, count=CNT),
        ambiguous=dict(u_lo=u_lo[amb].astype(np.int64), u_hi=u_hi[amb].astype(np.int64), v_lo=v_lo[amb].astype(np.int64),
                       v_hi=v_hi[amb].astype(np.int64), u_exact=np.trunc(Uc[amb]).astype(np.int64), v_exact=np.trunc(Vc[amb]).astype(np.int64),
                       depth_w=D[amb], intensity=ii[amb], e_depth=e_d[amb]),
    )


def warp_bounds(ref, ordered):
    """Per-cell tolerances (depth, intensity) of a checked, touched cell.

    integer path (exact fixed-point sums, sf_splat.h): each contribution enters as trunc(w depth_w^ 2^26) -- the weighted
    mean of those truncations is within 2^-26 of the mean of w depth_w^ (2^-28 for intensity); depth_w^ is within e_d of the
    exact depth_w; the int64 -> float conversion and the division round twice: 2 ulp of the result.
        |gpu - ref| <= 2 ulp(ref) + q + sum w e_d / sum w
    float-order path (the reference's own float sums, the oracle and the ordered coarse splat): instead of q the n-term float sum
    of the rounded products w depth_w^: gamma_{n+1} sum |w v| / sum w.
    """
    n = ref["count"]
    if ordered:
        tail_d = gamma(n + 1) * (ref["abs_depth"] + ref["e_depth"])
        tail_i = gamma(n + 1) * ref["abs_intensity"]
    else:
        tail_d, tail_i = FIX_DEPTH_Q, FIX_INTENS_Q
    bd = 2 * ulp32(ref["depth"]) + ref["e_depth"] + tail_d + 1e-14 * ref["abs_depth"]
    bi = 2 * ulp32(ref["intensity"]) + tail_i + 1e-14 * ref["abs_intensity"]
    return bd, bi


def check_warp(ref, depth, intensity, ordered):
    """Compare a warped depth / intensity plane with the exact reference on the checked cells. Returns (failures, stats):
    failures is a list of strings (empty: pass); stats holds coverage and the largest |got - ref| / bound."""
    got_d = np.asarray(depth, np.float64)
    got_i = np.asarray(intensity, np.float64)
    chk = ref["checked"]
    touched = ref["w"] > 0
    fails = []
    set_diff = chk & (touched != (got_d != 0.0))
    if set_diff.any():
        v, u = np.nonzero(set_diff)
        fails.append("touched-cell sets differ at %d checked cells, first (v, u) = (%d, %d): ref weight %d, got depth %r"
                     % (set_diff.sum(), v[0], u[0], ref["w"][v[0], u[0]], got_d[v[0], u[0]]))
    bd, bi = warp_bounds(ref, ordered)
    m = chk & touched
    rd = np.where(m, np.abs(got_d - ref["depth"]) / bd, 0.0)
    ri = np.where(m, np.abs(got_i - ref["intensity"]) / bi, 0.0)
    for name, r, got, want in (("depth", rd, got_d, ref["depth"]), ("intensity", ri, got_i, ref["intensity"])):
        if not np.all(np.isfinite(got[m])) or r.max() > 1.0:
            v, u = np.unravel_index(int(np.argmax(np.where(np.isfinite(r), r, np.inf))), r.shape)
            fails.append("%s: %d checked cells beyond the bound, worst (v, u) = (%d, %d): got %r, exact %r, |d| / bound = %.3g"
                         % (name, int((r > 1.0).sum()), v, u, got[v, u], want[v, u], r[v, u]))
    scope = touched | ~chk
    stats = dict(coverage=float(m.sum()) / max(1, int(scope.sum())), checked_cells=int(m.sum()),
                 ratio_depth=float(rd.max()), ratio_intensity=float(ri.max()), max_count=ref["max_count"],
                 n_ambiguous=ref["n_ambiguous"], n_sources=ref["n_sources"])
    return fails, stats


# --------------------------------------------------------------------------------------------------------------------------
#  B. IRLS normal equations (one IRLS iteration from var = 0), 6 x 6 solve, velocity filter, SE(3) update
# --------------------------------------------------------------------------------------------------------------------------
def irls_weights(B, b_row, kc_cauchy):
    """The weights of the first IRLS iteration (reference FrontEnd.cpp:588-637): residuals res = -B (var = 0),
    aver_res = sum |B| / 2N, w_r = clamp(b, 0, 1) / sqrt(1 + (res_r / (kc aver_res))^2); b_row: the b of each row's pixel."""
    B = np.asarray(B, np.float64)
    aver = np.abs(B).sum() / B.size
    inv_c = 1.0 / (kc_cauchy * aver)
    return np.clip(b_row, 0.0, 1.0) / np.sqrt(1.0 + (B * inv_c) ** 2), aver


def row_term_magnitudes(A, x, y, d):
    """Per row and entry, the sum of the magnitudes of the terms the product's factored rows combine into that entry
    (sf_irls.h, PixFact: a_c = P g1 + Q g2, a_d = W g3 + P g1 + Q g2 with P = -a_0, Q = -a_1, g1 = [-1, 0, x/d, xy/d,
    -(x^2/d + d), y], g2 = [0, -1, y/d, y^2/d + d, -xy/d, -x], g3 = [0, 0, 1, y, -x, 0]): a computed entry is off by a few u of
    THIS, not of |a|, where its terms cancel. x, y, d: the Inter planes at each row's pixel (2 rows per pixel)."""
    A = np.asarray(A, np.float64)
    x, y, d = (np.repeat(np.asarray(v, np.float64), 2) for v in (x, y, d))
    g1 = np.abs(np.stack([np.ones_like(x), 0 * x, x / d, x * y / d, x * x / d + d, y], 1))
    g2 = np.abs(np.stack([0 * x, np.ones_like(x), y / d, y * y / d + d, x * y / d, x], 1))
    g3 = np.abs(np.stack([0 * x, 0 * x, np.ones_like(x), y, x, 0 * x], 1))
    P, Q = np.abs(A[:, 0:1]), np.abs(A[:, 1:2])
    s = P * g1 + Q * g2
    depth_row = (np.arange(A.shape[0]) % 2 == 1)[:, None]
    Wd = np.abs(A[:, 2] + A[:, 0] * x / d + A[:, 1] * y / d)[:, None]  # the depth row's twd (its a_2 minus the P, Q terms)
    return s + np.where(depth_row, Wd * g3, 0.0)


def normal_equations(A, B, w, s=None, c_row=12.0, c_sum=72.0):
    """AtA, AtB of the weighted rows (w a_r, w B_r) in fp64, and their entrywise bounds.

    The implementation forms each weighted row entry in float (weights from reciprocal square roots, factored rows) -- off by
    at most c_row u s_ri, s the term magnitudes of row_term_magnitudes (|a| when s is None) -- and sums w^2 a_ri a_rj as
    fused products into float partial sums of at most 2 x 32 rows, then a 4- or 16-lane float group sum, then fp64:
        |AtA_ij^ - AtA_ij| <= u [c_row sum w^2 (|a_i| s_j + s_i |a_j|) + c_sum sum w^2 |a_i a_j|] + ulp(AtA_ij)
    (c_sum = 64 + 8 covers the longest float chain; the final rounding to float is the ulp). The oracle (float products, fp64
    sums of its own rows) sits far inside this."""
    A = np.asarray(A, np.float64)
    B = np.asarray(B, np.float64)
    Aw = A * w[:, None]
    Bw = B * w
    s = np.abs(A) if s is None else np.asarray(s, np.float64)
    Sw = s * np.abs(w)[:, None]
    Ab = np.abs(Aw)
    AtA = Aw.T @ Aw
    AtB = Aw.T @ Bw
    bA = U32 * (c_row * (Ab.T @ Sw + Sw.T @ Ab) + c_sum * (Ab.T @ Ab))
    # w B_r is one product (no cancellation): off by at most c_row u |w B_r|
    bB = U32 * (c_row * (Sw.T @ np.abs(Bw) + Ab.T @ np.abs(Bw)) + c_sum * (Ab.T @ np.abs(Bw)))
    bA = bA + ulp32(AtA) + 1e-13 * (Ab.T @ Ab)
    bB = bB + ulp32(AtB) + 1e-13 * (Ab.T @ np.abs(Bw))
    return AtA, AtB, bA, bB


def solve_residual(AtA, AtB, var, c=64.0):
    """Scaled residual of a 6 x 6 symmetric solve on the implementation's own float AtA, AtB, var: a backward-stable solver
    (LDL^T of an SPD matrix: |dA| <= c u |L||D||L^T|) leaves ||AtA var - AtB|| <= c u (||AtA|| ||var|| + ||AtB||).
    Returns (residual, bound)."""
    M = np.asarray(AtA, np.float64).reshape(6, 6)
    b = np.asarray(AtB, np.float64)
    x = np.asarray(var, np.float64)
    r = np.linalg.norm(M @ x - b)
    return r, c * U32 * (np.linalg.norm(M, 2) * np.linalg.norm(x) + np.linalg.norm(b))


def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def se3_exp(xi):
    """exp of the twist xi = (v, w) (translation first, the reference's convention): 4 x 4 fp64"""
    xi = np.asarray(xi, np.float64)
    v, w = xi[:3], xi[3:]
    th2 = float(w @ w)
    th = np.sqrt(th2)
    if th < 1e-3:  # Taylor series: the closed forms cancel catastrophically here
        a = 1 - th2 / 6 + th2 * th2 / 120
        b = 0.5 - th2 / 24 + th2 * th2 / 720
        c = 1 / 6 - th2 / 120 + th2 * th2 / 5040
    else:
        a, b, c = np.sin(th) / th, (1 - np.cos(th)) / th2, (th - np.sin(th)) / (th2 * th)
    W = _hat(w)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + a * W + b * W @ W
    T[:3, 3] = (np.eye(3) + b * W + c * W @ W) @ v
    return T


def se3_log(T):
    """inverse of se3_exp (rotation angle < pi) from the antisymmetric part of R and atan2 (accurate at small angles)"""
    T = np.asarray(T, np.float64)
    R, t = T[:3, :3], T[:3, 3]
    r = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.linalg.norm(r)
    th = np.arctan2(s, 0.5 * (np.trace(R) - 1.0))
    w = r * (1 + th * th / 6 if s < 1e-9 else th / s)
    th2 = float(w @ w)
    tha = np.sqrt(th2)
    d = 1 / 12 + th2 / 720 if tha < 1e-3 else (1 - tha * np.sin(tha) / (2 * (1 - np.cos(tha)))) / th2
    Wh = _hat(w)
    return np.concatenate([(np.eye(3) - 0.5 * Wh + d * Wh @ Wh) @ t, w])


def velocity_filter(AtA, res_sqnorm, var, twist_old, T_prev, level, eig_weight, const_weight):
    """filterEstimateAndComputeT's filter (reference FrontEnd.cpp:713-755) as the matrix function it is -- no eigenvectors:
        C = inv(AtA) ||A var - B||^2,  W = cf C + df I  (cf, df carry exp(-level)),
        twist_level = (I + W)^-1 (var + W (twist_old - log T_prev)).
    Returns twist_level and the parts a tolerance needs."""
    M = np.asarray(AtA, np.float64).reshape(6, 6)
    e_l = float(np.float32(np.exp(-float(level))))
    cf = float(np.float32(np.float32(eig_weight) * np.float32(e_l)))
    df = float(np.float32(np.float32(const_weight) * np.float32(e_l)))
    C = np.linalg.inv(M) * res_sqnorm
    C = 0.5 * (C + C.T)
    Wm = cf * C + df * np.eye(6)
    old = np.asarray(twist_old, np.float64) - se3_log(T_prev)
    tl = np.linalg.solve(np.eye(6) + Wm, np.asarray(var, np.float64) + Wm @ old)
    return tl, dict(C=C, W=Wm, old=old, cf=cf, df=df, cond=np.linalg.cond(M))


# --------------------------------------------------------------------------------------------------------------------------
#  C. the b-solve (SegmentationBackground.cpp:133-174) from per-label mean residuals
# --------------------------------------------------------------------------------------------------------------------------
def b_solve(aver_res_label, aver_res_old, b_prior, lambda_t_w, connectivity, kb, kc, lambda_prior, lambda_reg):
    """24 x 24 fp64 solve of the segmentation system and the clamp to [-1, 2] (reference SegmentationBackground.cpp:133-174);
    also returns the unclamped solution."""
    L = len(b_prior)
    ar = np.asarray(aver_res_label, np.float64)
    lam = np.asarray(lambda_t_w, np.float64)
    bp = np.asarray(b_prior, np.float64)
    repr_res = max(0.001, aver_res_old)
    fixed = np.log(1.0 + (kb * repr_res / (kc * aver_res_old)) ** 2)
    data = fixed - np.log(1.0 + (ar / (kc * aver_res_old)) ** 2)
    big = lam > 0.1
    Ad = np.where(big, 2 * lam * lambda_prior, 2 * lam)
    Bs = np.where(big, data + 2 * lambda_prior * lam * bp, 2 * lam * bp)
    M = np.diag(Ad * Ad)
    w2 = (2.0 * lambda_reg) ** 2
    for l in range(L):
        for m in range(l + 1, L):
            if connectivity[l][m]:
                M[l, l] += w2
                M[m, m] += w2
                M[l, m] -= w2
                M[m, l] -= w2
    x = np.linalg.solve(M, Ad * Bs)
    return np.clip(x, -1.0, 2.0), x


def label_means(res_abs_pair, labels, n_labels=24):
    """per-label mean |r| with the reference's num_pix + 1 (FrontEnd.cpp:650-667): sum / (2 (count + 1)); res_abs_pair: |r_c| +
    |r_d| per valid pixel"""
    s = np.bincount(labels, weights=res_abs_pair, minlength=n_labels)[:n_labels]
    n = np.bincount(labels, minlength=n_labels)[:n_labels]
    return s / (2.0 * (n + 1)), n


# --------------------------------------------------------------------------------------------------------------------------
#  D. linearisation and segmentation prior: calculateCoord, calculateDerivatives, computeWeights, the Jacobian rows
#     (reference FrontEnd.cpp:393-586) and computeSegPrior (SegmentationBackground.cpp:53-103)
# --------------------------------------------------------------------------------------------------------------------------
# Every constant below is a count of float roundings (u = 2^-24 each; a 1-ulp hardware rcp / rsq counts 2 u, because
# ulp(x) <= 2 u |x|), applied to the magnitude of the terms that can cancel. Products of two u-sized errors are covered by
# the factor SECOND_ORDER. The float constants are the float32 values the code uses.
EPS_INTENSITY = float(np.float32(1e-6))   # epsilon_intensity (:445)
EPS_DEPTH = float(np.float32(0.005))      # epsilon_depth (:446)
ERR_M_C, ERR_M_D = 1.0, float(np.float32(0.01))  # error_m_c, error_m_d (:491-492)
K_DUVT_C, K_DUVT_D = 10.0, 200.0          # kduvt_c, kduvt_d (:487-488)
SECOND_ORDER = 1.0 + 1e-5

# gradient (rl D_r + rc D_l) / (rc + rl), r = |D| + eps:  D = a - b: u;  r: u |D| + u r <= 2 u r;  product r D: 2 + 1 + 1 = 4 u;
# numerator: 4 u of each product + u of the sum <= 5 u (|t1| + |t2|);  denominator: 2 u of each r + u = 3 u;  so the quotient is
# off by (5 + 3) u m, m = (|t1| + |t2|) / (rc + rl), plus its own rounding, 1/2 ulp of the value.
C_GRADIENT = 8.0
# raw pre-weight sqrtf(1.f / (e_m + k (|t| + |u| + |v|))), IEEE: two sums and the product 3 u, e_m + ...: u -> argument 4 u (all
# terms positive); 1 / x: + u = 5 u; sqrt halves it and rounds: 2.5 + 1 = 3.5 u.
C_WEIGHT_RAW = 3.5
# normalised: the maximum is one of the raw values (3.5 u), 1.f / max: + u = 4.5 u, times the raw value (3.5 u), rounded (u): 9 u
C_WEIGHT = 9.0
# The product's kernels (fact_from_record of sf_irls.h + debug_rows of sf_solver_support.h), from the stored derivative planes:
#   pre-weight  twc = (inv_max_c rsq(1 + e)) kph:  argument 4 u -> 2 u, rsq 1 ulp = 2 u, inv_max_c 4.5 u (above: its minimum-e
#               argument 4 u, 1 / x u, sqrt -> 3.5 u, 1 / max u), two products 2 u                                       = 10.5 u
#               (twd = inv_max_d rsq(0.01 + e): one product less, 9.5 u)
#   fd = f rcp(d):  f = float(cols) / (2 tan): tan of another libm 1 ulp = 2 u, the division u = 3 u; d = 0.5 (dn + dw) u,
#               rcp 1 ulp = 2 u; the product u                                                                         = 7 u
#   pc = twc (dcu fd): two products                                                                          10.5 + 7 + 2 = 19.5 u
#   geometry    x = 0.5 (xn + xw): xn = (inv_f_pyr (u - disp)) dn: inv_f_pyr 3 u, two products = 5 u; xw = (u - disp) dw inv_f_w:
#               inv_f_w = 1 / f 4 u, two products = 6 u; the sum u -> 7 u.  xd = x rcp(d): 7 + 3 + 1 = 11 u;  xyd = xd y: 11 + 7
#               + 1 = 19 u;  xxd = fma(xd, x, d): 11 + 7 = 18 u on x^2 / d, u on d, the fma's rounding u <= 19 u
#   entry       fma(pc, g1, qc g2) (colour), fma(twd, g3, fma(pd, g1, qd g2)) (depth): per term 19.5 + 19 u and the rounding of its
#               product or fma (u), the depth row's outer fma u more                                                  <= 40.5 u
# -> |a - exact| <= 41 u s, s = row_term_magnitudes (the magnitudes of the terms the entry combines, not |a|). The reference's
# expression order (the oracle: IEEE, no rcp / rsq, the weight planes at 9 u) needs fewer.
C_ROW_A = 41.0
# B: bct = twc dct: 10.5 + 1 = 11.5 u;  bdt = twd ddt: 9.5 u, ddt = dn - dw u, the product u = 11.5 u. Relative: no cancellation.
C_ROW_B = 12.0
# prior term 1 - kz |dn - dw|: the difference u, the product u -> 2 u kz |ddt|; the outer difference u |t|
#   integer sums (Q32.32): every term truncated to 2^-32, the int64 sum exact; (float)(sum 2^-32): u; / count: u
#   float order: n float additions of the terms gamma_n sum |t|; / count: u
#   fp64 sums rounded to float (the oracle's exact_sums hook): u; / count: u
FIX_PRIOR_Q = 2.0 ** -32


def _inner(shape):
    m = np.zeros(shape, bool)
    m[1:-1, 1:-1] = True
    return m


def coord_reference(d_new, i_new, d_warp, i_warp, behind_camera="product"):
    """calculateCoord (:393-430) and the temporal derivatives (:477-478) from the NEW and WARPED planes of the level.

    behind_camera: what becomes of a pixel whose warped depth is negative (a point warped behind the camera that still projects
    into the image). "reference": nothing special (the reference, the oracle with its switch off, the reference-order build).
    "product": it is not in validPixels, stays non-Null, and its stored warped depth is |dw| -- so `ddt` is dn - |dw| there
    (the prior reads it; sf_linearise.h, solve_linearise).
    Every value is one float operation on float inputs: the bound is 1/2 ulp (`check_planes(..., c=0, half_ulp=True)`); Null and
    validPixels are exact. Returns a dict of (rows, cols) arrays."""
    assert behind_camera in ("product", "reference")
    dn, i_n, dw, iw = (np.asarray(a, np.float32).astype(np.float64) for a in (d_new, i_new, d_warp, i_warp))
    null = ~((dn != 0.0) & (dw != 0.0))
    valid = ~null & _inner(dn.shape)
    dwp = dw
    if behind_camera == "product":
        valid &= dw > 0.0
        dwp = np.abs(dw)
    return dict(null=null, valid=valid, depth=np.where(null, 0.0, 0.5 * (dn + dw)), intensity=0.5 * (i_n + iw), dct=i_n - iw,
                ddt=dn - dwp, n_behind=int((~null & _inner(dn.shape) & (dw < 0.0)).sum()))


def _edge_aware(X, null, eps):
    """the four-neighbour stencil of :448-474 on one Inter plane -> (du, dv, m_u, m_v) on the inner pixels that are not Null, 0
    elsewhere. r = 1 where the left / upper neighbour is Null (its rx / ry keep the fill value of :436-439)."""
    du, dv, mu, mv = (np.zeros(X.shape) for _ in range(4))
    c = X[1:-1, 1:-1]
    ok = ~null[1:-1, 1:-1]
    for out, mag, lo, hi, nlo in ((du, mu, X[1:-1, :-2], X[1:-1, 2:], null[1:-1, :-2]), (dv, mv, X[:-2, 1:-1], X[2:, 1:-1], null[:-2, 1:-1])):
        d_hi, d_lo = hi - c, c - lo
        r_c = np.abs(d_hi) + eps
        r_lo = np.where(nlo, 1.0, np.abs(d_lo) + eps)
        den = r_c + r_lo
        out[1:-1, 1:-1] = np.where(ok, (r_lo * d_hi + r_c * d_lo) / den, 0.0)
        mag[1:-1, 1:-1] = np.where(ok, (np.abs(r_lo * d_hi) + np.abs(r_c * d_lo)) / den, 0.0)
    return du, dv, mu, mv


def gradient_reference(depth_inter, intensity_inter, null):
    """calculateDerivatives' spatial part (:432-474) from the implementation's own INTER depth and intensity planes and Null.
    Returns dcu, dcv, ddu, ddv and their term magnitudes m_dcu ... (|r_l D_r| + |r_c D_l|) / (r_c + r_l): a float evaluation is
    within C_GRADIENT u m + 1/2 ulp(value). Defined on the inner non-Null pixels; the caller masks with its validPixels (the
    planes are exactly 0 outside them)."""
    D = np.asarray(depth_inter, np.float32).astype(np.float64)
    I = np.asarray(intensity_inter, np.float32).astype(np.float64)
    null = np.asarray(null) != 0
    dcu, dcv, mcu, mcv = _edge_aware(I, null, EPS_INTENSITY)
    ddu, ddv, mdu, mdv = _edge_aware(D, null, EPS_DEPTH)
    return dict(dcu=dcu, dcv=dcv, ddu=ddu, ddv=ddv, m_dcu=mcu, m_dcv=mcv, m_ddu=mdu, m_ddv=mdv)


def check_planes(got, exact, valid, c=0.0, mag=None, relative=False, half_ulp=True):
    """max over `valid` of |got - exact| / bound, bound = c u (mag, or |exact| when relative) + 1/2 ulp(exact) -- and whether the
    plane is exactly 0 outside `valid`. -> (ratio, (v, u) of the worst pixel, zero_outside)"""
    got = np.asarray(got, np.float64)
    scale = np.abs(exact) if relative or mag is None else mag
    bound = SECOND_ORDER * c * U32 * scale + (0.5 * ulp32(exact) if half_ulp else 0.0) + 1e-300
    r = np.where(valid, np.abs(got - exact) / bound, 0.0)
    r = np.where(np.isfinite(r), r, np.inf)
    at = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r.max()), tuple(int(k) for k in at), bool(np.all(got[~valid] == 0.0))


def weights_reference(dcu, dcv, dct, ddu, ddv, ddt, valid):
    """computeWeights (:481-510) from the implementation's six derivative planes on its validPixels: the raw pre-weights
    1 / sqrt(e_m + k (|t| + |u| + |v|)), their maxima, and the normalised planes (0 outside validPixels).
    IEEE evaluation (the oracle; the planes sf_get_lin_plane recomputes on the host with the device's 1 / max): raw within
    C_WEIGHT_RAW u, normalised within C_WEIGHT u, relative. The weights the product's KERNELS use (rsq, rcp at 1 ulp) are seen
    through the rows only (rows_reference)."""
    p = [np.abs(np.asarray(a, np.float32).astype(np.float64)) for a in (dcu, dcv, dct, ddu, ddv, ddt)]
    e_c = K_DUVT_C * (p[2] + p[0] + p[1])
    e_d = K_DUVT_D * (p[5] + p[3] + p[4])
    raw_c = np.where(valid, 1.0 / np.sqrt(ERR_M_C + e_c), 0.0)
    raw_d = np.where(valid, 1.0 / np.sqrt(ERR_M_D + e_d), 0.0)
    max_c, max_d = (float(r.max()) if valid.any() else 0.0 for r in (raw_c, raw_d))
    return dict(raw_c=raw_c, raw_d=raw_d, max_c=max_c, max_d=max_d, wc=raw_c / max_c if max_c else raw_c, wd=raw_d / max_d if max_d else raw_d,
                min_e_c=float(e_c[valid].min()) if valid.any() else np.inf, min_e_d=float(e_d[valid].min()) if valid.any() else np.inf)


def focal_length(cols, tan_half_fovh):
    """f = float(cols) / (2.f * tan) in float32 (:537)"""
    return float(np.float32(cols) / (np.float32(2.0) * np.float32(tan_half_fovh)))


def rows_reference(dcu, dcv, dct, ddu, ddv, d_new, d_warp, wc, wd, valid, tan_half_fovh, k_photometric_res):
    """The Jacobian rows (:535-586) in fp64: A (2N x 6) and B (2N) in validPixels order (u outer, v inner; the colour row of a
    pixel, then its depth row), from the implementation's derivative planes, the NEW and WARPED depth of the level and the EXACT
    normalised weights of weights_reference -- so this is the check that sees the weights the kernels themselves evaluate
    (fact_from_record: rsq of the stored planes times the device's 1 / max), which sf_get_lin_plane does not return.

    ddt = dn - dw, d = (dn + dw) / 2, x = (u - disp_u) d / f, y = (v - disp_v) d / f. The Inter coordinates are 0.5 (xx + xxWarped)
    with xxWarped = (u - disp_u) dw (1 / f) after a warp and the pyramid's (inv_f_i (u - disp_u)) dw on a first iteration
    (Warped := Pred): the same number in exact arithmetic, two float associations -- both inside the count of C_ROW_A.
    Returns A, B and x, y, d per valid pixel (for row_term_magnitudes)."""
    rows, cols = np.shape(d_new)
    f = focal_length(cols, tan_half_fovh)
    sel = np.asarray(valid).T.ravel()
    col = lambda a: np.asarray(a, np.float64).T.ravel()[sel]
    uu, vv = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    dn, dw = col(np.asarray(d_new, np.float32)), col(np.asarray(d_warp, np.float32))
    d = 0.5 * (dn + dw)
    x = (col(uu) - 0.5 * (cols - 1)) * d / f
    y = (col(vv) - 0.5 * (rows - 1)) * d / f
    inv_d = 1.0 / d
    kph = float(np.float32(k_photometric_res))
    N = int(sel.sum())
    A = np.zeros((2 * N, 6))
    B = np.zeros(2 * N)
    for half, (gu, gv, gt, w, one) in enumerate(((col(dcu), col(dcv), col(dct), col(wc) * kph, 0.0), (col(ddu), col(ddv), dn - dw, col(wd), 1.0))):
        dy, dz = gu * f * inv_d, gv * f * inv_d
        A[half::2, 0] = w * -dy
        A[half::2, 1] = w * -dz
        A[half::2, 2] = w * (one + dy * x * inv_d + dz * y * inv_d)
        A[half::2, 3] = w * (one * y + dy * inv_d * y * x + dz * (y * y * inv_d + d))
        A[half::2, 4] = w * (-one * x - dy * (x * x * inv_d + d) - dz * inv_d * y * x)
        A[half::2, 5] = w * (dy * y - dz * x)
        B[half::2] = w * -gt
    return A, B, (x, y, d)


def check_rows(A_got, B_got, A, B, xyd):
    """-> (max |A_got - A| / (C_ROW_A u s), max |B_got - B| / (C_ROW_B u |B|), (row, column) of the worst A entry)"""
    s = row_term_magnitudes(A, *xyd)
    rA = np.abs(np.asarray(A_got, np.float64) - A) / (SECOND_ORDER * C_ROW_A * U32 * s + 1e-300)
    rB = np.abs(np.asarray(B_got, np.float64) - B) / (SECOND_ORDER * C_ROW_B * U32 * np.abs(B) + 0.5 * ulp32(B) + 1e-300)
    at = np.unravel_index(int(np.argmax(rA)), rA.shape) if rA.size else (0, 0)
    return float(rA.max()) if rA.size else 0.0, float(rB.max()) if rB.size else 0.0, (int(at[0]), int(at[1]))


def seg_prior_reference(d_new, d_warp, labels, kz, behind_camera="product", n_labels=24):
    """computeSegPrior (SegmentationBackground.cpp:53-103) from the NEW and WARPED depth and the labels of the level.

    The counts are exact. lambda_t_w is evaluated in float32 (the `ratio < 0.1f` branch is a decision: it must be bit-equal).
    b_prior: the exact mean of t = 1 - kz |dn - dw| (|dw| in place of dw under the product's rule) over the non-Null pixels of
    the cluster, clamped to [-1, 2] (1-Lipschitz), -1 on the starved branch, 0 for an empty cluster -- with one bound per
    summation path (see the counts above C_ROW_B):
        "integer":  mean e_t + 2^-32 + 2 u |mean|      (Q32.32 sums: the product builds)
        "float":    mean e_t + gamma_n sum |t| / n + u |mean|   (the reference's order: the oracle, the reference-order build)
        "fp64":     mean e_t + 2 u |mean|              (the oracle's exact_sums hook)
    e_t = u |t| + 2 u kz |ddt| is the float evaluation of one term. Returns a dict; `bound[path]` are arrays of n_labels."""
    dn = np.asarray(d_new, np.float32).astype(np.float64)
    dw = np.asarray(d_warp, np.float32).astype(np.float64)
    if behind_camera == "product":
        dw = np.abs(dw)
    lab = np.asarray(labels).astype(np.int64)
    kz = float(np.float32(kz))
    member = lab != n_labels
    nonnull = member & (dn != 0.0) & (dw != 0.0)
    size = np.bincount(lab[member], minlength=n_labels)[:n_labels]
    nn = np.bincount(lab[nonnull], minlength=n_labels)[:n_labels]
    ddt = np.abs(dn - dw)[nonnull]
    t = 1.0 - kz * ddt
    e_t = U32 * np.abs(t) + 2 * U32 * kz * ddt
    S = np.bincount(lab[nonnull], weights=t, minlength=n_labels)[:n_labels]
    Sa = np.bincount(lab[nonnull], weights=np.abs(t), minlength=n_labels)[:n_labels]
    Se = np.bincount(lab[nonnull], weights=e_t, minlength=n_labels)[:n_labels]
    ratio = (nn.astype(np.float32) / np.maximum(size, 1).astype(np.float32)).astype(np.float32)  # float(nonnull) / float(size), :89
    starved = (size > 0) & (ratio < np.float32(0.1))
    lam = np.where(size > 0, np.where(starved, np.float32(0.1), ratio), np.float32(0)).astype(np.float32)
    n = np.maximum(nn, 1).astype(np.float64)
    mean = S / n
    full = (size > 0) & ~starved
    b = np.where(full, np.clip(mean, -1.0, 2.0), np.where(starved, -1.0, 0.0))
    me, am = Se / n * SECOND_ORDER, np.abs(mean)
    z = np.zeros(n_labels)
    bound = {"integer": np.where(full, me + FIX_PRIOR_Q + 2 * U32 * am, z),
             "float": np.where(full, me + gamma(nn) * Sa / n + U32 * am, z),
             "fp64": np.where(full, me + 2 * U32 * am, z)}
    return dict(size=size, nonnull=nn, lambda_t_w=lam, b_prior=b, bound=bound, starved=starved, full=full, terms=t, term_labels=lab[nonnull],
                sum=S)


# --------------------------------------------------------------------------------------------------------------------------
#  E. computeResidualsAgainstPreviousImage (reference FrontEnd.cpp:896-1069) and buildSegmImage (SegmentationBackground.cpp:
#     176-197): the five-frame residuals per cluster from the images fed, the poses reported and the labels
# --------------------------------------------------------------------------------------------------------------------------
# Counts (u = 2^-24 per float rounding), for a counted target pixel with current depth dc, warped depth dw, intensity
# difference idiff and warped intensity iw:
#   dw, iw        the splat of section A: bd, bi = warp_bounds(., ordered) of the path the build takes at level 0
#   dc - dw       one rounding: u |dc - dw|;   idiff - iw: u |idiff - iw|, times k: one more -> 2 u k |idiff - iw|
#   t = |.| + k |.|   one rounding (or none, fused): u t
#   -> e_t = bd + k bi + u (|dc - dw| + 2 k |idiff - iw|) + u t
#   integer sums (the product builds): t 2^32 is exact in float (a power of two), to_fix truncates it by less than one unit:
#       2^-32 per term; the int64 sums over lanes, labels and workgroups are exact; (float)(sum 2^-32): u; / float(2 (c + 1)): u
#       -> (sum e_t + c 2^-32) / (2 (c + 1)) + 2 u |result|
#   float order (the oracle, the reference-order build): c sequential float additions, gamma_c sum |t|, in place of c 2^-32;
#       the division u (the 2 u above covers it)
HISTORY = 5               # bufferLength (StaticFusion-datasets.cpp)
N_LABELS = 24             # NUM_CLUSTERS; the label of a pixel without a cluster
FIX_RES_Q = 2.0 ** -32    # resolution of the per-label residual sums (sf_device_common.h: FIX_RES)
STATIC_RESIDUAL = 0.017   # buildSegmImage's threshold on the mean residual (SegmentationBackground.cpp:187)
MAX_COMBINATIONS = 4096   # candidate placements of the ambiguous sources of ONE cell that are enumerated


def mul4_cm_f32(A, B):
    """mul4_cm (sf_smallmath.h; reference FrontEnd.cpp:766): C = A B in float32, the inner sum left to right, every product and
    every sum rounded on its own (the library is built without contraction). (row, col) float32 matrices."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    C = np.zeros((4, 4), np.float32)
    for c in range(4):
        for r in range(4):
            s = A[r, 0] * B[0, c]
            s = s + A[r, 1] * B[1, c]
            s = s + A[r, 2] * B[2, c]
            s = s + A[r, 3] * B[3, c]
            C[r, c] = s
    return C


def history_transform(hist_T, T_odometry, index):
    """The transform computeResidualsAgainstPreviousImage(index) inverts (:901-909): I odomBuffer[(index - 4) % 5] ...
    odomBuffer[(index - 1) % 5] T_odometry, each product as mul4_cm evaluates it -- bit for bit the float32 matrix the stage
    hands to its inverse. hist_T: the five ring slots ((row, col) float32 matrices; slots the chain does not read may be None)."""
    T = np.eye(4, dtype=np.float32)
    for i in range(index - HISTORY + 1, index):
        T = mul4_cm_f32(T, hist_T[i % HISTORY])
    return mul4_cm_f32(T, T_odometry)


def residual_sources(d_old, d_cur, tan_half_fovh):
    """The sources of the stage's splat: the old depth where it and the CURRENT depth are not 0 (Src::load of sf_residuals.h;
    reference :1232), and xxBuffer / yyBuffer (:922-926) in float32 as every implementation evaluates them:
    (inv_f_i (u - disp_u)) z, inv_f_i = 2 tan / cols."""
    rows, cols = np.shape(d_old)
    inv_f_i = np.float32(2.0) * np.float32(tan_half_fovh) / np.float32(cols)
    _, disp_u, disp_v = warp_geometry(rows, cols, tan_half_fovh)
    z = np.where(np.asarray(d_cur, np.float32) != 0, np.asarray(d_old, np.float32), np.float32(0)).astype(np.float32)
    xs = inv_f_i * (np.arange(cols, dtype=np.float32) - np.float32(disp_u))
    ys = inv_f_i * (np.arange(rows, dtype=np.float32) - np.float32(disp_v))
    return z, (xs[None, :] * z).astype(np.float32), (ys[:, None] * z).astype(np.float32)


def _residual_terms(W, SD, SI, SE, CNT, dc, idf, k):
    """From the sums of a cell: the term t, whether the cell counts as far as the warp decides (touched, warped depth not 0),
    and e_t per summation path of the splat (see the counts above)."""
    Wd = np.maximum(W, 1).astype(np.float64)
    cell = dict(depth=SD / Wd, intensity=SI / Wd, e_depth=SE / Wd, abs_depth=np.abs(SD) / Wd, abs_intensity=np.abs(SI) / Wd, count=CNT)
    rd, ri = np.abs(dc - cell["depth"]), np.abs(idf - cell["intensity"])
    t = rd + k * ri
    e = {}
    for ordered in (False, True):
        bd, bi = warp_bounds(cell, ordered)
        e[ordered] = SECOND_ORDER * (bd + k * bi + U32 * (rd + 2 * k * ri) + U32 * t)
    return t, (W > 0) & (cell["depth"] != 0.0), e, cell


def residuals_reference(d_old, i_old, d_cur, i_cur, labels0, T, tan_half_fovh, k_photometric_res, segmentation_enabled):
    """perClusterAverageResidual of computeResidualsAgainstPreviousImage: the images pushed five frames ago (d_old, i_old) warped
    by T^-1 (T: history_transform) onto the current ones, t = |d_cur - d_w| + k |idiff - i_w| summed per level-0 label over the
    target pixels that are touched, have a current depth, a warped depth and a label below 24; idiff = i_cur where the old depth
    of that pixel is not 0, else 0 (:937, :1022); result sum t / (2 (c + 1)), NaN for c = 0. Without segmentation every pixel has
    label 0 (clusterAllocation[0] keeps its constructor value).

    The splat is warp_reference's (section A). A source whose centi-pixel truncation the float evaluation could put on either
    side cannot be left out of a SUM: for every cell such sources reach, the term is evaluated under every combination of their
    candidate positions (each source: the distinct weights it can give that cell; beyond MAX_COMBINATIONS the ranges of d_w
    and i_w over the extreme weights -- a weighted mean is linear-fractional in each weight -- and interval arithmetic), giving
    [t_lo, t_hi] and whether the cell counts under all or only some of them.

    Returns a dict of arrays over the 24 labels: `value` (the sources at their exact positions), `c`, `sum_abs`; `c_min`, `c_max`,
    `s_lo`, `s_hi`; `sum_e[path]`, `bound[path]`, `lo[path]`, `hi[path]` for path "integer" (the splat's and the stage's
    fixed-point sums), "ordered+integer" (the ordered float splat of an image of at most 2048 pixels on one workgroup, the
    stage's fixed-point sums) and "float" (the reference's order in both); the admissible interval of a correct build is
        [s_lo / (2 (c_max + 1)) - bound, s_hi / (2 (c_min + 1)) + bound];
    and `terms` / `counted` / `depth_w` / `intensity_w` / `idiff` (planes, exact positions), `labels`, `k`, and what the scene exercised: n_sources, n_ambiguous,
    n_ambiguous_cells, n_capped_cells, n_idiff_zero, n_invalid_label, n_untouched."""
    import itertools

    d_old, i_old, d_cur, i_cur = (np.asarray(a, np.float32).astype(np.float64) for a in (d_old, i_old, d_cur, i_cur))
    rows, cols = d_cur.shape
    lab = np.asarray(labels0).astype(np.int64) if segmentation_enabled else np.zeros((rows, cols), np.int64)
    k = float(np.float32(k_photometric_res))
    z, xx, yy = residual_sources(d_old, d_cur, tan_half_fovh)
    ref = warp_reference(z, i_old, xx, yy, T, tan_half_fovh)
    idiff = np.where(d_old != 0.0, i_cur, 0.0)
    eligible = (d_cur != 0.0) & (lab < N_LABELS)
    sm = ref["sums"]
    paths = (False, True)  # the splat's: integer, ordered float

    # -- the cells no ambiguous source reaches
    t, counts, e, _ = _residual_terms(sm["w"], sm["depth"], sm["intensity"], sm["e_depth"], sm["count"], d_cur, idiff, k)
    sure = eligible & ref["checked"] & counts
    binsum = lambda mask, w=None: np.bincount(lab[mask], weights=None if w is None else w[mask], minlength=N_LABELS)[:N_LABELS].astype(np.float64)
    c_min = binsum(sure)
    c_max = c_min.copy()
    c_nom = c_min.copy()
    s_lo = binsum(sure, t)
    s_hi, s_nom = s_lo.copy(), s_lo.copy()
    sum_e = {p: binsum(sure, e[p]) for p in paths}
    terms = np.where(sure, t, np.nan)
    counted = sure.copy()
    Wd = np.maximum(sm["w"], 1).astype(np.float64)
    depth_w, intensity_w = np.where(sure, sm["depth"] / Wd, np.nan), np.where(sure, sm["intensity"] / Wd, np.nan)

    # -- the cells they reach
    amb = ref["ambiguous"]
    cols_lim, rows_lim = 100 * (cols - 1), 100 * (rows - 1)
    cand, nominal, reach = [], [], {}
    for s in range(amb["depth_w"].size):
        cl, cells = [], set()
        for a in range(int(amb["u_lo"][s]), int(amb["u_hi"][s]) + 1):
            for b in range(int(amb["v_lo"][s]), int(amb["v_hi"][s]) + 1):
                taps = {}
                if 0 <= a < cols_lim and 0 <= b < rows_lim:
                    tv, tu, w = _taps(np.array([a]), np.array([b]))
                    taps = {(int(tv[q, 0]), int(tu[q, 0])): int(w[q, 0]) for q in range(4) if w[q, 0] > 0}
                if (a, b) == (int(amb["u_exact"][s]), int(amb["v_exact"][s])):
                    nominal.append(len(cl))
                cl.append(taps)
                cells |= set(taps)
        cand.append(cl)
        for cell in cells:
            reach.setdefault(cell, []).append(s)
    assert len(nominal) == len(cand)
    assert all(not ref["checked"][cell] for cell in reach)
    rec = []  # (cell number, is the exact placement, W, SD, SI, SE, CNT) of every enumerated combination
    cells, capped = [], []
    for cell, srcs in sorted(reach.items()):
        if not eligible[cell]:
            continue
        base = [sm[q][cell] for q in ("w", "depth", "intensity", "e_depth", "count")]
        opts = [sorted({cl.get(cell, 0) for cl in cand[s]}) for s in srcs]
        nom = tuple(cand[s][nominal[s]].get(cell, 0) for s in srcs)
        n_comb = int(np.prod([len(o) for o in opts], dtype=np.float64))
        if n_comb > MAX_COMBINATIONS:
            assert len(srcs) <= 16, "more than 16 ambiguous sources reach one cell: outside this reference's preconditions"
            opts = [[o[0], o[-1]] for o in opts]
            capped.append(len(cells))
        combos = list(itertools.product(*opts))
        if nom not in combos:
            combos.append(nom)
        for ws in combos:
            r = list(base)
            for s, w in zip(srcs, ws):
                if w:
                    r[0] += w
                    r[1] += w * amb["depth_w"][s]
                    r[2] += w * amb["intensity"][s]
                    r[3] += w * amb["e_depth"][s]
                    r[4] += 1
            rec.append([len(cells), ws == nom] + r)
        cells.append(cell)
    n_cells = len(cells)
    if n_cells:
        R = np.array(rec, dtype=np.float64)
        cid, is_nom = R[:, 0].astype(np.int64), R[:, 1] != 0
        cv, cu = (np.array([c[q] for c in cells]) for q in (0, 1))
        t, counts, e, cell_v = _residual_terms(R[:, 2], R[:, 3], R[:, 4], R[:, 5], R[:, 6], d_cur[cv, cu][cid], idiff[cv, cu][cid], k)
        t_lo, t_hi = np.full(n_cells, np.inf), np.full(n_cells, -np.inf)
        np.minimum.at(t_lo, cid[counts], t[counts])
        np.maximum.at(t_hi, cid[counts], t[counts])
        some = np.zeros(n_cells, bool)
        some[cid[counts]] = True
        always = np.ones(n_cells, bool)
        always[cid[~counts]] = False
        e_max = {p: np.zeros(n_cells) for p in paths}
        for p in paths:
            np.maximum.at(e_max[p], cid[counts], e[p][counts])
        for q in capped:  # the extremes of d_w and i_w are among the enumerated corners; t between them by interval arithmetic
            m = (cid == q) & counts
            if m.any():
                dc, idf = d_cur[cells[q]], idiff[cells[q]]
                dl, dh, il, ih = cell_v["depth"][m].min(), cell_v["depth"][m].max(), cell_v["intensity"][m].min(), cell_v["intensity"][m].max()
                t_lo[q] = max(0.0, dl - dc, dc - dh) + k * max(0.0, il - idf, idf - ih)
                t_hi[q] = max(abs(dc - dl), abs(dc - dh)) + k * max(abs(idf - il), abs(idf - ih))
        cl_lab = lab[cv, cu]
        acc = lambda mask, w: np.bincount(cl_lab[mask], weights=w[mask], minlength=N_LABELS)[:N_LABELS]
        one = np.ones(n_cells)
        c_min += acc(always, one)
        c_max += acc(some, one)
        s_lo += acc(always, np.where(always, t_lo, 0.0))
        s_hi += acc(some, np.where(some, t_hi, 0.0))
        for p in paths:
            sum_e[p] += acc(some, e_max[p])
        nm = is_nom & counts
        c_nom += np.bincount(cl_lab[cid[nm]], minlength=N_LABELS)[:N_LABELS]
        s_nom += np.bincount(cl_lab[cid[nm]], weights=t[nm], minlength=N_LABELS)[:N_LABELS]
        terms[cv[cid[nm]], cu[cid[nm]]] = t[nm]
        counted[cv[cid[nm]], cu[cid[nm]]] = True
        depth_w[cv[cid[nm]], cu[cid[nm]]] = cell_v["depth"][nm]
        intensity_w[cv[cid[nm]], cu[cid[nm]]] = cell_v["intensity"][nm]

    with np.errstate(invalid="ignore", divide="ignore"):
        value = np.where(c_nom > 0, s_nom / (2.0 * (c_nom + 1.0)), np.nan)
        top = s_hi / (2.0 * (c_min + 1.0))
        # path -> (the splat's sums, the stage's sums)
        parts = {"integer": (sum_e[False], c_max * FIX_RES_Q), "ordered+integer": (sum_e[True], c_max * FIX_RES_Q),
                 "float": (sum_e[True], gamma(c_max) * s_hi)}
        bound = {p: np.where(c_max > 0, (se + tail) / (2.0 * (c_min + 1.0)) + 2 * U32 * top, np.nan) for p, (se, tail) in parts.items()}
        lo = {p: np.where(c_max > 0, s_lo / (2.0 * (c_max + 1.0)) - bound[p], np.nan) for p in bound}
        hi = {p: np.where(c_max > 0, top + bound[p], np.nan) for p in bound}
        sum_e = {p: se for p, (se, _) in parts.items()}
    touched = (sm["w"] > 0) | ~ref["checked"]
    return dict(value=value, c=c_nom.astype(np.int64), sum_abs=s_nom, c_min=c_min.astype(np.int64), c_max=c_max.astype(np.int64), s_lo=s_lo,
                s_hi=s_hi, sum_e=sum_e, bound=bound, lo=lo, hi=hi, terms=terms, counted=counted, labels=lab,
                depth_w=depth_w, intensity_w=intensity_w, idiff=idiff, k=k,
                n_sources=ref["n_sources"], n_ambiguous=ref["n_ambiguous"], n_ambiguous_cells=n_cells, n_capped_cells=len(capped),
                n_idiff_zero=int((counted & (d_old == 0.0)).sum()), n_invalid_label=int((lab >= N_LABELS).sum()),
                n_untouched=int(((d_cur != 0.0) & ~touched).sum()))


def check_residuals(ref, got, path):
    """cluster_residuals() of a build against residuals_reference: the NaN pattern (a cluster whose count interval includes 0 may
    be either) and the admissible interval. -> (failures, ratio): ratio is the largest |got - value| / bound -- above 1 only
    where the ambiguous sources, not the roundings, decide -- over the clusters that have a value."""
    got = np.asarray(got, np.float64)
    fails, ratio = [], 0.0
    for l in range(N_LABELS):
        if ref["c_max"][l] == 0:
            if not np.isnan(got[l]):
                fails.append("label %d: %r for a cluster without a counted pixel" % (l, got[l]))
        elif np.isnan(got[l]):
            if ref["c_min"][l] > 0:
                fails.append("label %d: NaN for a cluster of %d counted pixels" % (l, ref["c"][l]))
        else:
            if not ref["lo"][path][l] <= got[l] <= ref["hi"][path][l]:
                fails.append("label %d (%d pixels): got %r outside [%r, %r], exact %r, |d| / bound = %.3g"
                             % (l, ref["c"][l], got[l], ref["lo"][path][l], ref["hi"][path][l], ref["value"][l],
                                abs(got[l] - ref["value"][l]) / ref["bound"][path][l]))
            if ref["c"][l] > 0:
                ratio = max(ratio, abs(got[l] - ref["value"][l]) / ref["bound"][path][l])
    return fails, float(ratio)


def segm_image_reference(labels0, b_segm, cluster_res, uncertain=None):
    """buildSegmImage: per pixel clamp(b_segm[label], 0, 1), replaced by max(b, 1 - b) where double(residual) < 0.017; 1 for a
    pixel without a cluster ("assume static"). All in float32, exact. cluster_res: the 24 residuals, or (lo, hi), the admissible
    interval of each (NaN: an empty cluster, never below the threshold); a cluster whose interval straddles the threshold, or
    that `uncertain` marks (it may or may not be empty), and whose value depends on the answer, is left out.
    -> (image, checked pixels, number of clusters left out)"""
    lab = np.asarray(labels0).astype(np.int64)
    lo, hi = cluster_res if isinstance(cluster_res, tuple) else (cluster_res, cluster_res)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    b = np.minimum(np.maximum(np.asarray(b_segm, np.float32), np.float32(0)), np.float32(1))
    flipped = np.maximum(b, np.float32(1) - b)
    with np.errstate(invalid="ignore"):
        below, some_below = hi < STATIC_RESIDUAL, lo < STATIC_RESIDUAL
    open_ = (below != some_below) | (np.zeros(N_LABELS, bool) if uncertain is None else np.asarray(uncertain) & some_below)
    open_ &= flipped != b
    val = np.append(np.where(below, flipped, b), np.float32(1)).astype(np.float32)
    idx = np.minimum(lab, N_LABELS)
    return val[idx], ~np.append(open_, False)[idx], int(open_.sum())
