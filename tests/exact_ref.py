"""Exact (fp64) references of the warp splat, the IRLS normal equations, the 6 x 6 solve, the velocity filter and the SE(3)
update -- each recomputed from the inputs the implementation under test gave that stage, and each returned together with the
rounding bound a correct float implementation must meet (tests/test_exact_references.py).

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
    `max_count`. Use `warp_bounds` for the tolerance of a given summation path.
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
    )


def warp_bounds(ref, ordered):
    """Per-cell tolerances (depth, intensity) of a checked, touched cell.

    integer path (exact fixed-point sums, sf_device_common.h): each contribution enters as trunc(w depth_w^ 2^26) -- the weighted
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
    (sf_solver.h, PixFact: a_c = P g1 + Q g2, a_d = W g3 + P g1 + Q g2 with P = -a_0, Q = -a_1, g1 = [-1, 0, x/d, xy/d,
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
