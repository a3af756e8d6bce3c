"""A brute-force NumPy renderer of include/sf_view.h: the reference of the free-view tests at sizes and settings the oracle's
prediction cannot take (tests/test_view_reference_cpu.py checks it against the oracle where it can).

Everything runs in np.float32, one expression per operation, in the order of staticfusion_amd/csrc/sf_view.h (which repeats
sf_predict.h): NumPy's + - * / sqrt on float32 are correctly rounded, so this is the same arithmetic as the kernels'. A loop
over the surfels, vectorised over the pixels of the clipped sprite, keeps the running minimum of the 64-bit key. Meant for
small images and a few thousand surfels.
"""
import numpy as np

F = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
LARGE_PIXELS = 1024  # SFV_LARGE_PIXELS: a clipped sprite with more pixels is drawn by the large-sprite kernel
SQRT2 = F(1.41421356)  # splat.vert:70
PIXEL_CENTRE = F(0.5)  # gl_FragCoord of pixel i is i + 0.5


def invert_pose(pose16):
    """pose.inverse() as the library computes it: double Gauss-Jordan with partial pivoting, rounded to float (column-major in
    and out)"""
    A = [[float(pose16[r + 4 * c]) for c in range(4)] for r in range(4)]
    Ai = [[1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    for c in range(4):
        piv, pv = c, abs(A[c][c])
        for r in range(c + 1, 4):
            if abs(A[r][c]) > pv:
                pv, piv = abs(A[r][c]), r
        if piv != c:
            A[c], A[piv] = A[piv], A[c]
            Ai[c], Ai[piv] = Ai[piv], Ai[c]
        inv = 1.0 / A[c][c]
        for j in range(4):
            A[c][j] *= inv
            Ai[c][j] *= inv
        for r in range(4):
            if r == c:
                continue
            f = A[r][c]
            if f == 0.0:
                continue
            for j in range(4):
                A[r][j] -= f * A[c][j]
                Ai[r][j] -= f * Ai[c][j]
    return np.array([Ai[k % 4][k // 4] for k in range(16)], np.float32)


def _to_int(x):
    """(int) of a float as v_cvt_i32_f32 does it: NaN -> 0, saturating"""
    x = float(x)
    if x != x:
        return 0
    return int(min(max(x, -2147483648.0), 2147483647.0))


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _normalize(a):
    n = np.sqrt(_dot(a, a))
    return (a[0] / n, a[1] / n, a[2] / n)


def _cross(a, b):
    return (a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1])


class _Ctx:
    def __init__(self, view, tick):
        self.T = invert_pose(view.pose[:])
        self.cx, self.cy, self.fx, self.fy = F(view.cx), F(view.cy), F(view.fx), F(view.fy)
        self.rows, self.cols = int(view.rows), int(view.cols)
        self.min_confidence, self.max_depth = F(view.min_confidence), F(view.max_depth)
        self.use_age = view.max_age >= 0
        self.tick, self.max_age = F(tick), F(view.max_age)
        self.shade = int(view.shade)
        # the ray table, [i (column), j (row)]: normalize((i + 0.5 - cx) / fx, (j + 0.5 - cy) / fy, 1)
        i = np.arange(self.cols, dtype=np.float32)[:, None] + PIXEL_CENTRE
        j = np.arange(self.rows, dtype=np.float32)[None, :] + PIXEL_CENTRE
        X = np.broadcast_to((i - self.cx) / self.fx, (self.cols, self.rows))
        Y = np.broadcast_to((j - self.cy) / self.fy, (self.cols, self.rows))
        Z = np.ones((self.cols, self.rows), np.float32)
        n = np.sqrt((X * X + Y * Y) + Z * Z)
        self.rays = (X / n, Y / n, Z / n)
        self.rays_of_the_dot = _rays_of_the_dot(self.rays, (X, Y, Z))


def _rays_of_the_dot(normalised, unnormalised):
    """the ray dot(l, n) is taken with: the normalised one (combo_splat.frag:37-39)"""
    return normalised


def _corner_rectangle_applies(corners):
    """the corner rectangle prunes only while every corner is in front of the camera (sf_surfel_geom.h, surfel_sprite)"""
    return all(p[2] > F(0) for p in corners)


def _discarded(dd, r2):
    return dd > r2  # combo_splat.frag:45


def _key(depth, s):
    """GL_LESS in buffer order: the smallest (depth bits, index) wins"""
    return (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(s)


def _index_of(keys):
    return keys & np.uint64(0xFFFFFFFF)


def _to_camera(c, q):
    T = c.T
    x, y, z = q[0], q[1], q[2]
    h = (((T[0] * x + T[4] * y) + T[8] * z) + T[12], ((T[1] * x + T[5] * y) + T[9] * z) + T[13], ((T[2] * x + T[6] * y) + T[10] * z) + T[14])
    nx, ny, nz = q[8], q[9], q[10]
    n = _normalize(((T[0] * nx + T[4] * ny) + T[8] * nz, (T[1] * nx + T[5] * ny) + T[9] * nz, (T[2] * nx + T[6] * ny) + T[10] * nz))
    culled = bool(h[2] > c.max_depth or h[2] < F(0.4) or q[3] < c.min_confidence)
    if c.use_age and not (c.tick - q[7] <= c.max_age):
        culled = True
    return h, n, q[11], culled


def _sprite(c, q):
    """camera-frame geometry and the clipped pixel rectangle of surfel q, or None when it draws nothing"""
    h, n, rad, culled = _to_camera(c, q)
    if culled:
        return None
    fcols, frows = F(c.cols), F(c.rows)
    ndc_x = ((((c.fx * h[0]) / h[2]) + c.cx) - (fcols * F(0.5))) / (fcols * F(0.5))
    ndc_y = ((((c.fy * h[1]) / h[2]) + c.cy) - (frows * F(0.5))) / (frows * F(0.5))
    if not (ndc_x >= F(-1) and ndc_x <= F(1) and ndc_y >= F(-1) and ndc_y <= F(1)):
        return None
    xw, yw = (ndc_x + F(1)) * (fcols * F(0.5)), (ndc_y + F(1)) * (frows * F(0.5))
    u = _normalize((n[1] - n[2], -n[0], n[0]))
    x1 = tuple((a * rad) * SQRT2 for a in u)
    y1 = _cross(n, x1)
    corners = [tuple(a + b for a, b in zip(h, x1)), tuple(a + b for a, b in zip(h, y1)), tuple(a - b for a, b in zip(h, y1)),
               tuple(a - b for a, b in zip(h, x1))]
    px = [((c.fx * p[0]) / p[2]) + c.cx for p in corners]
    py = [((c.fy * p[1]) / p[2]) + c.cy for p in corners]
    xlo = np.fmin(px[0], np.fmin(px[1], np.fmin(px[2], px[3])))
    xhi = np.fmax(px[0], np.fmax(px[1], np.fmax(px[2], px[3])))
    ylo = np.fmin(py[0], np.fmin(py[1], np.fmin(py[2], py[3])))
    yhi = np.fmax(py[0], np.fmax(py[1], np.fmax(py[2], py[3])))
    size = np.fmax(F(0), np.fmax(np.abs(xhi - xlo), np.abs(yhi - ylo)))
    if not (size > F(0)):
        return None
    half = size * F(0.5)
    i0 = max(0, _to_int(np.ceil(xw - half - F(0.5))))
    i1 = min(c.cols - 1, _to_int(np.floor(xw + half - F(0.5))))
    j0 = max(0, _to_int(np.ceil(yw - half - F(0.5))))
    j1 = min(c.rows - 1, _to_int(np.floor(yw + half - F(0.5))))
    if _corner_rectangle_applies(corners):
        i0 = max(i0, _to_int(np.floor(xlo - F(1.5))))
        i1 = min(i1, _to_int(np.ceil(xhi + F(0.5))))
        j0 = max(j0, _to_int(np.floor(ylo - F(1.5))))
        j1 = min(j1, _to_int(np.ceil(yhi + F(0.5))))
    if not (i0 <= i1 and j0 <= j1):
        return None
    return h, n, rad, i0, i1, j0, j1


def sprite_pixels(surfels, view, tick=1):
    """pixels of the clipped sprite of every surfel (0: draws nothing): which of them the library lists as large"""
    surfels = np.ascontiguousarray(surfels, np.float32).reshape(-1, 12)
    out = np.zeros(surfels.shape[0], np.int64)
    with np.errstate(all="ignore"):
        c = _Ctx(view, tick)
        for s in range(surfels.shape[0]):
            sp = _sprite(c, surfels[s])
            if sp is not None:
                out[s] = (sp[4] - sp[3] + 1) * (sp[6] - sp[5] + 1)
    return out


def decode_colour(code):
    """color.glsl decodeColor: the three bytes of int(s[4])"""
    c = np.asarray(code, np.float32).astype(np.int64)
    return np.stack([(c >> 16) & 0xFF, (c >> 8) & 0xFF, c & 0xFF], -1).astype(np.uint8)


def grey(rgb):
    """the prediction's intensity of a colour image"""
    norm = F(1) / F(255)
    f = rgb.astype(np.float32) * norm
    return (F(0.299) * f[..., 0] + F(0.587) * f[..., 1]) + F(0.114) * f[..., 2]


def render(surfels, view, tick=1):
    """dict(depth (rows, cols) float32, rgb (rows, cols, 3) uint8, index (rows, cols) int32) of include/sf_view.h"""
    surfels = np.ascontiguousarray(surfels, np.float32).reshape(-1, 12)
    with np.errstate(all="ignore"):
        c = _Ctx(view, tick)
        keys = np.full((c.cols, c.rows), EMPTY, np.uint64)  # [i, j], like the column-major key image
        zimg = np.zeros((c.cols, c.rows), np.float32)
        nimg = np.zeros((c.cols, c.rows, 3), np.float32)
        two_max = F(2) * c.max_depth
        for s in range(surfels.shape[0]):
            sp = _sprite(c, surfels[s])
            if sp is None:
                continue
            h, n, rad, i0, i1, j0, j1 = sp
            win = (slice(i0, i1 + 1), slice(j0, j1 + 1))
            lx, ly, lz = c.rays[0][win], c.rays[1][win], c.rays[2][win]
            dx_, dy_, dz_ = (r[win] for r in c.rays_of_the_dot)
            t = _dot(h, n) / ((dx_ * n[0] + dy_ * n[1]) + dz_ * n[2])
            cx_, cy_, cz_ = lx * t, ly * t, lz * t
            dx, dy, dz = cx_ - h[0], cy_ - h[1], cz_ - h[2]
            keep = ~_discarded((dx * dx + dy * dy) + dz * dz, rad * rad)
            depth = (cz_ / two_max) + F(0.5)
            keep &= (depth >= F(0)) & (depth < F(1))
            key = _key(depth, s)
            better = keep & (key < keys[win])
            keys[win] = np.where(better, key, keys[win])
            zimg[win] = np.where(better, cz_, zimg[win])
            nimg[win] = np.where(better[..., None], np.array(n, np.float32), nimg[win])
        drawn = keys != EMPTY
        index = np.where(drawn, _index_of(keys).astype(np.int64), -1).astype(np.int32)
        if c.shade == 1:
            v = np.fmin(np.fmax(F(0.5) * nimg + F(0.5), F(0)), F(1)) * F(255)
            rgb = np.rint(v).astype(np.int32).astype(np.uint8)
        else:
            rgb = decode_colour(surfels[np.maximum(index, 0), 4]) if surfels.shape[0] else np.zeros((c.cols, c.rows, 3), np.uint8)
        rgb = np.where(drawn[..., None], rgb, 0).astype(np.uint8)
        depth_out = np.where(drawn, zimg, F(0)).astype(np.float32)
    return dict(depth=np.ascontiguousarray(depth_out.T), rgb=np.ascontiguousarray(rgb.transpose(1, 0, 2)), index=np.ascontiguousarray(index.T))
