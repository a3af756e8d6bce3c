"""Exact (fp64) references of the surfel drawing and of the prediction's composition: sections F and G of tests/exact_ref.py,
kept in a file of their own for length (tests/test_exact_surfels.py).

F  one target of IndexMap::combinedPredict (reference IndexMap.cpp:221-300), derived from Shaders/splat.vert and
   Shaders/combo_splat.frag: for every surfel and every pixel of its gl_PointSize square the cull, the centre-in-image test,
   the square, the ray-plane intersection with the disc test, the depth-range test and z -- in fp64 from the float32 inputs,
   every decision with the margin inside which a float evaluation may fall either way.
G  Reconstruction::getPredictedImages on top of two targets (Reconstruction.cpp:628-720, denseEnough :218-233, Shaders/
   fill_vertex.frag, fill_vertex_from_texture.frag, fill_rgb.frag, extract_depth.frag, color.glsl): every operation is one
   float32 rounding or an integer, so given the winners the result is exact.

Plain NumPy. Nothing here imports oracle/, the product or tests/view_ref.py: the point is an answer that none of them wrote.
No pixel rectangle other than the square of splat.vert:85 is applied: the shaders have none.

THE MARGINS. A value is carried as (v, e): v the exact value of the shader's expression on the float32 inputs (fp64), e a bound
of |float evaluation - v| for an evaluation in the shader's association with IEEE + - * / sqrt (which the oracle, view_ref
and the kernels all claim to repeat). Every operation propagates the errors of its operands to first AND second order (products
of errors are kept, a divisor is taken at its smallest magnitude |b| - e_b) and adds its own rounding, u (|r| + propagated) with
u = 2^-24 -- unless both operands are exact and r is itself a float32 value, when the operation is exact (an identity pose
leaves h exact, dyadic intrinsics leave ndc exact: the threshold scenes rest on that). A divisor that can reach zero
(dot(l, n) -> 0: an edge-on disc; a corner z -> 0) makes e infinite. A comparison x > y is CERTAIN when |x - y| exceeds
e_x + e_y and OPEN otherwise; an infinite or NaN margin is always open, never certain. A NaN VALUE from a NaN input makes
every comparison false, as in the shader. The worst-case counts these rules give per decision are listed next to C_* below:
they are what a hand count of roundings gives (section D's style), and the table of tests/README.md repeats them.
"""
import numpy as np

from exact_ref import U32

SQRT2_F = float(np.float32(1.41421356))  # splat.vert:70, the float the shader multiplies by
NEAR_F = float(np.float32(0.4))          # splat.vert:57
TINY = 2.0 ** -149                       # smallest float32 subnormal: the absolute floor of a rounding

# Worst-case counts of roundings (u each), by hand, on the magnitude named; the tracker below never charges more
# (test_exact_surfels.py::test_the_tracker_stays_within_the_hand_counts holds it to C_H, C_NV / C_NORMAL, C_RAY, C_NDC and C_DEPTH;
# C_PLANE and C_DISC only document what the chain of operations adds up to: no test holds the tracker to them).
C_H = 7.0        # h = T p: per term T's ulp (2 u), a product (u) and up to three sums (3 u) on sum |T_ij p_j| + |T_i3|, the
                 # translation's own margin apart                                                        <= 7 u mags (0 at identity)
C_NV = 5.0       # v = T3 q[8..10]: T's ulp (2 u), the product (u), two sums (2 u) on m_i = sum_j |T_ij q_j|            5 u m_i
C_NORMAL = 13.5  # n = v / |v|: e_i <= C_NV u m_i / |v| + |n_i| (C_NV u sum_k |v_k| m_k / |v|^2 + 3.5 u): the squares carry twice v's error
                 # and u, the sums 2 u, the root halves it and adds u, the quotient u. Without cancellation (m = |v|): 2 x 5 + 3.5
C_RAY = 7.5      # l = normalize((x - cx) / fx, ., 1): difference, quotient 2 u; square 5 u; sums 7 u; sqrt 4.5 u; quotient    7.5 u |l_k|
C_NDC = 5.0      # ndc = (((f h.x) / h.z + c) - w/2) / (w/2): five operations on |f h.x / h.z| + |c| + w/2                    5 u (+ h's)
C_PLANE = 3.0    # dot(h, n), dot(l, n): product and two sums on sum |a_k b_k|, plus the operands' own errors            3 u (+ C_NORMAL, C_RAY)
C_DISC = 6.0     # dot(diff, diff) - rad^2: diff = l t - h (2 u on |l t| + |h|), squares and sums 3 u, rad^2 u; t carries C_PLANE / |dot(l, n)|
C_DEPTH = 2.0    # z / (2 maxDepth) + 0.5: the quotient and the sum (2 maxDepth is exact)                                    2 u (+ z's / 2 maxDepth)


def _nan_to_inf(e):
    return np.where(np.isnan(e), np.inf, e)


class R:
    """an array of exact values with the bound of their float evaluation error"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape)

    def take(self, idx):
        return R(self.v[idx], self.e[idx])

    @staticmethod
    def _lift(x):
        return x if isinstance(x, R) else R(np.float64(x))

    def _round(self, r, prop, exact_in, unrounded=False):
        """the operation's own rounding: none when the operands are exact and the result is a float32 value, or when the
        operation returns an operand as it is (x + 0, x * 0)"""
        with np.errstate(all="ignore"):
            is_f32 = r.astype(np.float32).astype(np.float64) == r
            exact = exact_in & is_f32 & (prop == 0)
            return R(r, _nan_to_inf(np.where(exact, 0.0, np.where(unrounded, prop, prop + U32 * (np.abs(r) + prop) + TINY))))

    def _zero(self):
        return (self.v == 0) & (self.e == 0)

    def __add__(self, o):
        o = R._lift(o)
        return self._round(self.v + o.v, self.e + o.e, (self.e == 0) & (o.e == 0), self._zero() | o._zero())

    def __sub__(self, o):
        o = R._lift(o)
        return self._round(self.v - o.v, self.e + o.e, (self.e == 0) & (o.e == 0), self._zero() | o._zero())

    def __mul__(self, o):
        o = R._lift(o)
        with np.errstate(all="ignore"):
            # an exact zero times anything finite is an exact zero
            zero = (self._zero() & np.isfinite(o.v)) | (o._zero() & np.isfinite(self.v))
            prop = np.where(zero, 0.0, _nan_to_inf(np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e))
            return self._round(self.v * o.v, prop, ((self.e == 0) & (o.e == 0)) | zero, zero)

    def __truediv__(self, o):
        o = R._lift(o)
        with np.errstate(all="ignore"):
            r = self.v / o.v
            low = np.abs(o.v) - o.e  # the divisor's smallest magnitude
            prop = np.where(low > 0, (self.e + np.abs(r) * o.e) / np.where(low > 0, low, 1.0), np.inf)
            prop = np.where((self.e == 0) & (o.e == 0), 0.0, _nan_to_inf(prop))
            return self._round(r, prop, (self.e == 0) & (o.e == 0))

    def __neg__(self):
        return R(-self.v, self.e)

    def abs(self):
        return R(np.abs(self.v), self.e)

    def sqrt(self):
        with np.errstate(all="ignore"):
            r = np.sqrt(self.v)
            den = r + np.sqrt(np.maximum(self.v - self.e, 0.0))
            prop = np.where(self.e == 0, 0.0, np.where(den > 0, self.e / np.where(den > 0, den, 1.0), np.inf))
            return self._round(r, _nan_to_inf(prop), self.e == 0)


def rmin(*xs):
    """min / max move by at most the largest error of their operands (fmin: a NaN operand is ignored)"""
    return R(np.fmin.reduce([x.v for x in xs]), np.maximum.reduce([x.e for x in xs]))


def rmax(*xs):
    return R(np.fmax.reduce([x.v for x in xs]), np.maximum.reduce([x.e for x in xs]))


def gt(x, y):
    """x > y in float: (certainly true, certainly false). Neither: open. A NaN value compares false; a NaN or infinite margin
    is open."""
    x, y = R._lift(x), R._lift(y)
    with np.errstate(all="ignore"):
        d = x.v - y.v
        m = _nan_to_inf(x.e + y.e)
        nan = np.isnan(x.v) | np.isnan(y.v)
        finite = np.isfinite(m)
        # (equal infinities give d = NaN with non-NaN values: open)
        t = finite & ~nan & (d > m)
        f = nan | (finite & (d <= -m))
    return t, f


def _all(*dec):
    """a conjunction of (true, false) decisions"""
    t = np.logical_and.reduce([d[0] for d in dec])
    f = np.logical_or.reduce([d[1] for d in dec])
    return t, f


def _not(d):
    return d[1], d[0]


def rdot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def rnormalize(a):
    n = rdot(a, a).sqrt()
    return (a[0] / n, a[1] / n, a[2] / n)


def rcross(a, b):
    return (a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1])


def inverse_f32(pose):
    """t_inv as the uniform the shader gets: the inverse of the float pose, rounded to float32 (column-major, 16)"""
    inv = np.linalg.inv(np.asarray(pose, np.float32).astype(np.float64).reshape(4, 4))
    inv[np.abs(inv) < 1e-300] = 0.0
    return np.ascontiguousarray(inv.T.reshape(16).astype(np.float32))


# --------------------------------------------------------------------------------------------------------------------------
#  F. one target of the drawing
# --------------------------------------------------------------------------------------------------------------------------
class Drawing:
    """What section F knows of one target. Per fragment that is not certainly discarded (arrays of equal length, sorted by
    pixel): s (surfel), pix (j * cols + i), certain (True: certainly drawn unless hidden; False: open), z, z_err, depth,
    depth_err (gl_FragDepth), admissible (may win its pixel). Per pixel: has_certain, has_any."""

    def __init__(self, rows, cols, n):
        self.rows, self.cols, self.n = rows, cols, n

    def fragments_of(self, certain_only=True):
        """(rows, cols) count of certain(-or-open) fragments per pixel"""
        m = self.certain if certain_only else np.ones_like(self.certain)
        return np.bincount(self.pix[m], minlength=self.rows * self.cols).reshape(self.rows, self.cols)


def draw_reference(surfels, pose, cx, cy, fx, fy, rows, cols, max_depth, conf_threshold, time=None, time_delta=None, max_time=None,
                   nan_age_culls=False, t_inv=None, max_fragments=40_000_000):
    """Section F. surfels (n, 12) float32; pose 4 x 4 (row, col) float32. The age tests of splat.vert:57 run when time_delta /
    max_time are given (`time - s[7] > time_delta`, `s[7] > max_time`); nan_age_culls: a NaN s[7] fails the age test, as
    include/sf_view.h words it (`not tick - s[7] <= max_age`), where the shader's form lets it pass."""
    q = np.ascontiguousarray(surfels, np.float32).reshape(-1, 12)
    n = q.shape[0]
    T = inverse_f32(pose) if t_inv is None else np.asarray(t_inv, np.float32)
    # another correct inversion may round an entry the other way: one ulp (2 u) on every entry that is not 0 or +-1
    # Assumption: the implementation inverts the pose in double and rounds to float (the library's routine, Eigen's for a
    # rigid pose alike), so an entry of the rotation block is the float next to the exact one, at worst the other neighbour:
    # one ulp (2 u). The translation column is -R^T t, three products and two sums that can cancel: its margin is taken from
    # their magnitudes (4 u sum_k |R_ki t_k|, what a float32 evaluation of it could be off by), not from the entry.
    def _entry(k):
        t = float(T[k])
        if k in (3, 7, 11, 15) or (k < 12 and (t == 0 or abs(t) == 1)):
            return 0.0
        if k < 12:
            return 2 * U32 * abs(t)
        i = k - 12
        mags = sum(abs(float(T[i + 4 * j])) * abs(float(np.asarray(pose, np.float32).reshape(4, 4)[j, 3])) for j in range(3))
        return max(4 * U32 * mags, 2 * U32 * abs(t)) if mags > 0 else 0.0

    Tc = [R(np.float64(t), _entry(k)) for k, t in enumerate(T)]
    col = [R(q[:, k].astype(np.float64)) for k in range(12)]
    f32 = lambda x: R(np.float64(np.float32(x)))
    cxr, cyr, fxr, fyr, mdr = f32(cx), f32(cy), f32(fx), f32(fy), f32(max_depth)
    out = Drawing(int(rows), int(cols), n)
    with np.errstate(all="ignore"):
        # ---- per surfel: splat.vert ------------------------------------------------------------------------------------
        x, y, z = col[0], col[1], col[2]
        h = tuple(((Tc[i] * x + Tc[4 + i] * y) + Tc[8 + i] * z) + Tc[12 + i] for i in range(3))  # :55
        culls = [gt(h[2], mdr), gt(R(NEAR_F), h[2]), gt(f32(conf_threshold), col[3])]              # :57
        if time_delta is not None:
            age = gt(f32(time) - col[7], f32(time_delta))
            if nan_age_culls:
                nan_t = np.isnan(q[:, 7])
                age = (age[0] | nan_t, age[1] & ~nan_t)
            culls.append(age)
        if max_time is not None:
            culls.append(gt(col[7], f32(max_time)))
        passes = _all(*[_not(c) for c in culls])
        fcols, frows = R(np.float64(cols)), R(np.float64(rows))
        half_c, half_r = fcols * 0.5, frows * 0.5
        ndc_x = ((((fxr * h[0]) / h[2]) + cxr) - half_c) / half_c                                   # :41-42, :64
        ndc_y = ((((fyr * h[1]) / h[2]) + cyr) - half_r) / half_r
        centre = _all(_not(gt(-1.0, ndc_x)), _not(gt(ndc_x, 1.0)), _not(gt(-1.0, ndc_y)), _not(gt(ndc_y, 1.0)))  # the point is clipped by its centre
        xw, yw = (ndc_x + 1.0) * half_c, (ndc_y + 1.0) * half_r                                     # the viewport transform
        nv = tuple((Tc[i] * col[8] + Tc[4 + i] * col[9]) + Tc[8 + i] * col[10] for i in range(3))
        nrm = rnormalize(nv)                                                                        # :68
        rad = col[11]
        u1 = rnormalize((nrm[1] - nrm[2], -nrm[0], nrm[0]))
        x1 = tuple((a * rad) * SQRT2_F for a in u1)                                                 # :70
        y1 = rcross(nrm, x1)                                                                        # :72
        corners = [tuple(a + b for a, b in zip(h, x1)), tuple(a + b for a, b in zip(h, y1)), tuple(a - b for a, b in zip(h, y1)),
                   tuple(a - b for a, b in zip(h, x1))]                                             # :74-77
        px = [((fxr * c[0]) / c[2]) + cxr for c in corners]                                         # :46-51
        py = [((fyr * c[1]) / c[2]) + cyr for c in corners]
        x_diff = (rmax(*px) - rmin(*px)).abs()                                                      # :79-83
        y_diff = (rmax(*py) - rmin(*py)).abs()
        size = rmax(R(np.zeros(n)), rmax(x_diff, y_diff))                                           # :85
        sized = gt(size, 0.0)
        half = size * 0.5
        lo_x, hi_x = (xw - half) - 0.5, (xw + half) - 0.5  # pixel i is in the square when lo <= i <= hi (centres at + 0.5)
        lo_y, hi_y = (yw - half) - 0.5, (yw + half) - 0.5
        pn = rdot(h, nrm)
        r2 = rad * rad                                                                              # combo_splat.frag:42
        nan_in = np.isnan(q[:, [0, 1, 2, 8, 9, 10, 11]]).any(axis=1)  # fmin / fmax drop NaN corners: size 0, nothing drawn
        surfel_dec = _all(passes, centre, sized)
        alive = ~surfel_dec[1] & ~nan_in
        out.corner_z = np.stack([c[2].v for c in corners], 1)
        out.corner_z_err = np.stack([c[2].e for c in corners], 1)
        out.corner_box = (rmin(*px), rmax(*px), rmin(*py), rmax(*py))
        out.surfel_certain, out.surfel_alive = surfel_dec[0] & ~nan_in, alive
        out.h, out.h_err = np.stack([a.v for a in h], 1), np.stack([a.e for a in h], 1)
        out.t_err = np.array([float(t.e) for t in Tc])
        out.nv, out.nv_err = np.stack([a.v for a in nv], 1), np.stack([a.e for a in nv], 1)
        out.nrm, out.nrm_err = np.stack([a.v for a in nrm], 1), np.stack([a.e for a in nrm], 1)
        out.ndc, out.ndc_err = np.stack([ndc_x.v, ndc_y.v], 1), np.stack([ndc_x.e, ndc_y.e], 1)
        Tf = T.astype(np.float64)
        out.h_mags = np.stack([np.abs(Tf[i] * x.v) + np.abs(Tf[4 + i] * y.v) + np.abs(Tf[8 + i] * z.v) + abs(Tf[12 + i]) for i in range(3)], 1)

        # ---- the candidate pixels of every live surfel: the square widened by its margins, the whole image when they blow up
        def span(lo, hi, size_):
            a = np.where(np.isfinite(lo.v - lo.e), np.ceil(np.clip(lo.v - lo.e, -1.0, size_)), 0.0)
            b = np.where(np.isfinite(hi.v + hi.e), np.floor(np.clip(hi.v + hi.e, -1.0, size_)), size_ - 1.0)
            return np.maximum(a, 0).astype(np.int64), np.minimum(b, size_ - 1).astype(np.int64)

        i0, i1 = span(lo_x, hi_x, cols)
        j0, j1 = span(lo_y, hi_y, rows)
        wi, wj = np.maximum(i1 - i0 + 1, 0), np.maximum(j1 - j0 + 1, 0)
        cnt = np.where(alive, wi * wj, 0)
        total = int(cnt.sum())
        assert total <= max_fragments, "section F: %d candidate fragments" % total
        out.square_fragments_per_surfel = cnt
        s_of = np.repeat(np.arange(n), cnt)
        k = np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        pi = i0[s_of] + k % np.maximum(wi[s_of], 1)
        pj = j0[s_of] + k // np.maximum(wi[s_of], 1)

        # ---- per fragment: the square, then combo_splat.frag -----------------------------------------------------------
        g = lambda r: r.take(s_of)
        fi, fj = R(pi.astype(np.float64)), R(pj.astype(np.float64))
        square = _all(_not(gt(g(lo_x), fi)), _not(gt(fi, g(hi_x))), _not(gt(g(lo_y), fj)), _not(gt(fj, g(hi_y))))
        lx = ((fi + 0.5) - cxr) / fxr                                                               # :37
        ly = ((fj + 0.5) - cyr) / fyr
        l = rnormalize((lx, ly, R(np.ones(total))))
        out.ray, out.ray_err = np.stack([a.v for a in l], 1), np.stack([a.e for a in l], 1)
        hn = tuple(g(a) for a in h)
        nn = tuple(g(a) for a in nrm)
        t = g(pn) / rdot(l, nn)                                                                     # :39
        c = tuple(a * t for a in l)
        diff = tuple(a - b for a, b in zip(c, hn))                                                  # :43
        disc = _not(gt(rdot(diff, diff), g(r2)))                                                    # :45
        depth = (c[2] / (mdr * 2.0)) + 0.5                                                          # :60
        in_range = _all(_not(gt(0.0, depth)), gt(1.0, depth))  # clipped to [0, 1], and GL_LESS against the cleared 1.0
        keep = _all((out.surfel_certain[s_of], np.zeros(total, bool)), square, disc, in_range)
        not_out = ~keep[1]
    out.square_fragments = int((~square[1]).sum())  # fragments inside (or possibly inside) a sprite square
    out.open_fragments = int((not_out & ~keep[0]).sum())
    order = np.argsort((pj * cols + pi)[not_out], kind="stable")
    sel = np.flatnonzero(not_out)[order]
    out.s, out.pix, out.certain = s_of[sel], (pj * cols + pi)[sel], keep[0][sel]
    out.z, out.z_err, out.depth, out.depth_err = c[2].v[sel], c[2].e[sel], depth.v[sel], depth.e[sel]
    out.max_depth = float(np.float32(max_depth))
    npix = rows * cols
    # the admissible winners: not above the smallest certain depth plus both bounds
    upper = np.where(out.certain, out.depth + out.depth_err, np.inf)
    limit = np.full(npix, np.inf)
    np.minimum.at(limit, out.pix, upper)
    out.admissible = out.depth - out.depth_err <= limit[out.pix]
    out.has_certain = np.isfinite(limit).reshape(rows, cols)
    out.has_any = np.bincount(out.pix, minlength=npix).reshape(rows, cols) > 0
    # bit-identical duplicate records: the lowest index of each class
    raw = np.ascontiguousarray(q).view(np.uint32).reshape(n, 12)
    if n:
        _, first, inv = np.unique(raw, axis=0, return_index=True, return_inverse=True)
        lowest = np.full(first.shape[0], n, np.int64)
        np.minimum.at(lowest, inv.reshape(-1), np.arange(n))
        out.first_of = lowest[inv.reshape(-1)]
    else:
        out.first_of = np.zeros(0, np.int64)
    # pixels with more than one admissible winner (copies of one record count once)
    cls = out.first_of[out.s] if n else out.s
    key = np.unique(np.stack([out.pix[out.admissible], cls[out.admissible]], 1), axis=0) if out.admissible.any() else np.zeros((0, 2), np.int64)
    out.winners_per_pixel = np.bincount(key[:, 0], minlength=npix).reshape(rows, cols)
    out.surfels = q
    return out


class DrawingMismatch(AssertionError):
    pass


def _fail(msg, where):
    jj, ii = np.nonzero(where)
    raise DrawingMismatch("%s at %d pixels, first (row %d, col %d)" % (msg, jj.size, jj[0], ii[0]))


def check_drawing(ref, index, depth):
    """An (index, depth) image of one target (include/sf_view.h: -1 / 0 where nothing is drawn, z of the winner elsewhere)
    against section F. Raises DrawingMismatch; returns the figures of tests/README.md."""
    rows, cols = ref.rows, ref.cols
    index = np.asarray(index).reshape(rows, cols)
    depth = np.asarray(depth, np.float32).reshape(rows, cols)
    drawn = index >= 0
    if (ref.has_certain & ~drawn).any():
        _fail("a certainly drawn pixel is empty", ref.has_certain & ~drawn)
    if (drawn & ~ref.has_any).any():
        _fail("a pixel no fragment can reach is drawn", drawn & ~ref.has_any)
    if (~drawn & (depth != 0)).any():
        _fail("an empty pixel has a depth", ~drawn & (depth != 0))
    if (index[drawn] >= ref.n).any():
        _fail("an index beyond the buffer", drawn & (index >= ref.n))
    # the named fragment of every drawn pixel
    got_key = (np.arange(rows * cols).reshape(rows, cols) * (ref.n + 1) + np.where(drawn, index, ref.n)).reshape(-1)
    frag_key = ref.pix * (ref.n + 1) + ref.s
    order = np.argsort(frag_key, kind="stable")
    pos = np.searchsorted(frag_key[order], got_key)
    pos = np.minimum(pos, max(frag_key.size - 1, 0))
    found = (frag_key[order][pos] == got_key) if frag_key.size else np.zeros(rows * cols, bool)
    f = order[pos] if frag_key.size else np.zeros(rows * cols, np.int64)
    found2 = found.reshape(rows, cols)
    if (drawn & ~found2).any():
        _fail("a drawn pixel names a surfel with no fragment there", drawn & ~found2)
    adm = np.zeros(rows * cols, bool)
    adm[found] = ref.admissible[f[found]]
    if (drawn & ~adm.reshape(rows, cols)).any():
        _fail("a drawn pixel names a fragment that a certainly nearer one hides", drawn & ~adm.reshape(rows, cols))
    err = np.abs(depth.reshape(-1).astype(np.float64) - ref.z[f] if frag_key.size else np.zeros(rows * cols))
    bound = ref.z_err[f] if frag_key.size else np.ones(rows * cols)
    d = drawn.reshape(-1)
    bad = d & ~(err <= bound)
    if bad.any():
        _fail("the depth of a drawn pixel is off by up to %.3g of its bound" % np.nanmax(err[bad] / bound[bad]), bad.reshape(rows, cols))
    named = index[drawn]
    if (ref.first_of[named] != named).any():
        w = np.zeros((rows, cols), bool)
        w[drawn] = ref.first_of[named] != named
        _fail("a copy of a record wins over the lower-indexed copy", w)
    ratio = float(np.max(err[d] / np.maximum(bound[d], TINY))) if d.any() else 0.0
    return dict(drawn=int(d.sum()), ratio=ratio, ambiguous=int((drawn & (ref.winners_per_pixel > 1)).sum()), open_fragments=ref.open_fragments,
                square_fragments=ref.square_fragments, certain_pixels=int(ref.has_certain.sum()),
                single_certain=int((ref.has_certain & (ref.winners_per_pixel == 1)).sum()))


def grey_f32(rgb):
    """Reconstruction.cpp:686-690: three products with 1.f / 255.f and the weighted sum, in float32"""
    F = np.float32
    norm = F(1) / F(255)
    c = np.asarray(rgb).astype(np.float32) * norm
    return (F(0.299) * c[..., 0] + F(0.587) * c[..., 1]) + F(0.114) * c[..., 2]


def decode_colour(code):
    """color.glsl decodeColor, stored to the RGBA8 target: the three bytes of int(c)"""
    c = np.trunc(np.nan_to_num(np.asarray(code, np.float64))).astype(np.int64)
    return np.stack([(c >> 16) & 0xFF, (c >> 8) & 0xFF, c & 0xFF], -1).astype(np.uint8)


def check_prediction(ref, depth, intensity, extract_max_depth, empty_intensity=0.0):
    """A prediction drawn from ONE target with nothing to fill in (conf_low == conf_high, a black previous frame, b < 0.6): no
    index image, so a pixel passes when SOME admissible winner explains its depth (within that surfel's bound, through the clip
    of extract_depth.frag) and its grey value (exactly)."""
    rows, cols = ref.rows, ref.cols
    depth = np.asarray(depth, np.float32).reshape(-1).astype(np.float64)
    inten = np.asarray(intensity, np.float32).reshape(-1)
    emax = float(np.float32(extract_max_depth))
    d, i = depth[ref.pix], inten[ref.pix]
    g = grey_f32(decode_colour(ref.surfels[ref.s, 4])) if ref.s.size else np.zeros(0, np.float32)
    kept = (np.abs(d - ref.z) <= ref.z_err) & (d > 0) & (d <= emax)
    clipped = (d == 0) & ((ref.z - ref.z_err <= 0) | (ref.z + ref.z_err > emax))
    ok_frag = ref.admissible & (kept | clipped) & (i == g)
    explained = np.zeros(rows * cols, bool)
    explained[ref.pix[ok_frag]] = True
    empty = (depth == 0) & (inten == np.float32(empty_intensity))
    ok = explained | (empty & ~ref.has_certain.reshape(-1))
    if not ok.all():
        _fail("a predicted pixel that no admissible winner explains", ~ok.reshape(rows, cols))
    err = np.where(ok_frag & kept, np.abs(d - ref.z) / np.maximum(ref.z_err, TINY), 0.0)
    return dict(drawn=int((depth > 0).sum()), ratio=float(err.max()) if err.size else 0.0)


# --------------------------------------------------------------------------------------------------------------------------
#  G. the composition: Reconstruction::getPredictedImages on top of the two targets
# --------------------------------------------------------------------------------------------------------------------------
WRONG = ("0.25 compared with >=", "sample position without + 0.5", "fill-in colour decided by z == 0")  # compose(..., wrong=)


def sample_positions(rows, cols, wrong=()):
    """Resize::image to (cols / 40) x (rows / 40): the nearest texel under the centre of every target pixel -- texel
    floor((i + 0.5) / rw * cols), an exact rational here; (rh * rw, 2) array of (row, col)"""
    rw, rh = cols // 40, rows // 40
    half = 0 if WRONG[1] in wrong else 1
    return np.array([[((2 * j + half) * rows) // (2 * rh), ((2 * i + half) * cols) // (2 * rw)] for j in range(rh) for i in range(rw)], np.int64).reshape(-1, 2)


def dense_enough(rgb_low, wrong=()):
    """denseEnough (:218-233) of the low-confidence image (rows, cols, 3) uint8"""
    rows, cols = rgb_low.shape[:2]
    pos = sample_positions(rows, cols, wrong)
    if pos.shape[0] == 0:
        return False, 0  # float(0) / float(0) > 0.25f is false
    px = rgb_low[pos[:, 0], pos[:, 1]]
    total = int(((px[:, 0] > 0) & (px[:, 1] > 0) & (px[:, 2] > 0)).sum())
    q = np.float32(total) / np.float32(pos.shape[0])
    return bool(q >= np.float32(0.25) if WRONG[0] in wrong else q > np.float32(0.25)), total


def compose(index_low, z_low, index_high, z_high, surfels, filtered_mm, rgb_prev, b_img, extract_max_depth, wrong=()):
    """Section G. The targets are (rows, cols) winner indices (-1: cleared) with the z their fragments wrote (0 where cleared);
    filtered_mm (rows, cols) uint16, rgb_prev (rows, cols, 3) uint8 and b_img (rows, cols) float32 are the previous frame's.
    Returns (dense, depth, intensity). `wrong`: entries of WRONG, each a composition that misreads the reference in one place --
    what the rejection tests run; the reference is wrong=()."""
    F = np.float32
    surfels = np.asarray(surfels, np.float32).reshape(-1, 12)

    def colours(index):
        c = decode_colour(surfels[np.maximum(index, 0), 4]) if surfels.shape[0] else np.zeros(index.shape + (3,), np.uint8)
        return np.where((index >= 0)[..., None], c, 0).astype(np.uint8)  # the targets are cleared to black

    c_low, c_high = colours(np.asarray(index_low)), colours(np.asarray(index_high))
    z_low, z_high = np.asarray(z_low, np.float32), np.asarray(z_high, np.float32)
    dense = dense_enough(c_low, wrong)[0]
    low_black = c_low.astype(np.int64).sum(-1) == 0    # fill_rgb.frag:33: sample.x + sample.y + sample.z == 0
    high_black = c_high.astype(np.int64).sum(-1) == 0
    if WRONG[2] in wrong:
        low_black, high_black = z_low == 0, z_high == 0
    if not dense:                                      # Reconstruction.cpp:663-669
        zr = np.asarray(filtered_mm).astype(np.float32) / F(1000)                  # fill_vertex.frag:50
        z1 = np.where(z_low == 0, np.where(np.asarray(b_img, np.float32) > F(0.6), zr, F(0)), z_low)  # :48-56
        z = np.where(z_high == 0, z1, z_high)                                      # fill_vertex_from_texture.frag:42-49
        c1 = np.where(low_black[..., None], np.asarray(rgb_prev, np.uint8), c_low)
        c = np.where(high_black[..., None], c1, c_high)
    else:                                              # :694-700
        z = np.where(z_high == 0, z_low, z_high)
        c = np.where(high_black[..., None], c_low, c_high)
    depth = np.where((z > F(extract_max_depth)) | (z <= 0), F(0), z).astype(np.float32)  # extract_depth.frag:32-38
    return dense, depth, grey_f32(c)
