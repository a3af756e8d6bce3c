"""Shared cases of the carve tests (test_carve_*_cpu.py, test_gpu_carve.py): parameter sets and views without the product's
types, the table of single surfels that puts the rule OBSERVE of include/sf_carve.h on each of its boundaries, the table of
DECIDE, and the scene of a wall, a floor seen at a grazing angle and a box face that is taken away."""
import types

import numpy as np

import carve_ref as cr

F = np.float32
TICK = 5


def params(**kw):
    """the parameters as a plain namespace (carve_ref reads members); defaults: those of the header"""
    d = dict(cr.DEFAULTS)
    d.update(kw)
    return types.SimpleNamespace(**d)


def as_product(p):
    from staticfusion_amd import carve

    return carve.Params(**vars(p))


def plain_view(pose=None, cx=3.0, cy=2.0, fx=4.0, fy=4.0, rows=6, cols=8, min_confidence=0.25, max_depth=20.0, max_age=-1):
    """a view as a plain namespace: pose 4x4 (row, col), stored as the 16 column-major floats of sfv_view"""
    T = np.eye(4, dtype=np.float32) if pose is None else np.asarray(pose, np.float32)
    return types.SimpleNamespace(pose=[float(x) for x in T.T.ravel()], cx=cx, cy=cy, fx=fx, fy=fy, rows=rows, cols=cols, min_confidence=min_confidence,
                                 max_depth=max_depth, max_age=max_age, shade=0)


def as_product_view(v):
    from staticfusion_amd import view

    return view.View(np.array(v.pose, np.float32).reshape(4, 4).T, v.cx, v.cy, v.fx, v.fy, v.rows, v.cols, v.min_confidence, v.max_depth, v.max_age)


def surfel(pos=(0.0, 0.0, 2.0), normal=(0.0, 0.0, -1.0), conf=0.5, t_last=3.0, radius=0.01):
    s = np.zeros(12, np.float32)
    s[0:3], s[3], s[4], s[6], s[7], s[8:11], s[11] = pos, conf, float((200 << 16) + (150 << 8) + 100), 1.0, t_last, normal, radius
    return s


def up(x):
    return np.nextafter(F(x), F(np.inf))


def down(x):
    return np.nextafter(F(x), F(-np.inf))


def mixed_image(rows, cols, seed, zp=2.0):
    """pixels in front of, on, behind a surface at zp, and invalid ones"""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0.0, zp - 0.5, zp, zp + 1.0, np.nan, 9.0], np.float32), (rows, cols))


def observe_cases():
    """[(name, surfel, tick, view, depth (rows, cols), params)]. The base: an 8 x 6 view at identity with integer cx, cy, a
    surfel on the optical axis at z = 2 that faces the camera, so that zp = 2 in every pixel; window 0, one pixel decides;
    tol = 0.25 exactly."""
    one = dict(window=0, min_pixels=1, tol_abs=0.25, tol_rel=0.0)
    out = []

    def add(name, s=None, v=None, z=None, img=None, tick=TICK, **kw):
        v = plain_view() if v is None else v
        p = dict(one)
        p.update(kw)
        img = np.full((v.rows, v.cols), F(2.0 if z is None else z), np.float32) if img is None else np.asarray(img, np.float32)
        out.append((name, surfel() if s is None else s, tick, v, img, params(**p)))

    # r on tol, and one ulp beyond it, from both sides
    add("r on +tol", z=2.25)
    add("r one ulp beyond +tol", z=up(2.25))
    add("r on -tol", z=1.75)
    add("r one ulp beyond -tol", z=down(1.75))
    add("r with a relative tolerance", z=2.3, tol_abs=0.1, tol_rel=0.1)
    # the frame's depth
    for name, z in (("z zero", 0.0), ("z negative", -1.0), ("z NaN", np.nan), ("z inf", np.inf), ("z on z_max", 3.0), ("z one ulp above z_max", up(3.0))):
        add(name, z=z, z_max=3.0)
    # den zero, negative and tiny: a plane through the camera's x = 0 plane; zp = 1 / lx
    side = surfel(pos=(1.0, 0.0, 2.0), normal=(-1.0, 0.0, 0.0))
    for name, v in (("den zero and negative", plain_view(cols=16)), ("zp below 0.4", plain_view(cols=16, fx=1.0)), ("den tiny positive", plain_view(cols=16, cx=3.001)),
                    ("den tiny negative", plain_view(cols=16, cx=2.999))):
        add(name, s=side, v=v, z=5.0, window=3, min_pixels=1, min_cos=0.0)
        add(name + ", frame in front", s=side, v=v, z=0.9, window=3, min_pixels=1, min_cos=0.0)
    # the projection on the image's borders
    add("qx exactly 0", s=surfel(pos=(-1.75, 0.0, 2.0)), z=3.0)
    add("qx exactly cols", s=surfel(pos=(2.25, 0.0, 2.0)), z=3.0)
    add("qx just below cols", s=surfel(pos=(down(2.25), 0.0, 2.0)), z=3.0)
    add("qy exactly 0", s=surfel(pos=(0.0, -1.25, 2.0)), z=3.0)
    add("qy exactly rows", s=surfel(pos=(0.0, 1.75, 2.0)), z=3.0)
    add("qx negative", s=surfel(pos=(-1.76, 0.0, 2.0)), z=3.0)
    # the window clipped at each border and each corner (pixel centres: x = (i - 3) / 2, y = (j - 2) / 2 at z = 2)
    for w in (1, 3):
        for i, j in ((0, 0), (7, 0), (0, 5), (7, 5), (3, 0), (3, 5), (0, 2), (7, 2), (3, 2)):
            add("window %d at pixel (%d, %d)" % (w, i, j), s=surfel(pos=((i - 3) / 2.0, (j - 2) / 2.0, 2.0)), img=mixed_image(6, 8, 10 * i + j), window=w, min_pixels=2)
    # window 0 and 3, min_pixels 1 and 49
    big = plain_view(rows=16, cols=16, cx=8.0, cy=8.0)
    add("window 3, 49 pixels through", v=big, z=3.0, window=3, min_pixels=49)
    img = np.full((16, 16), 3.0, np.float32)
    img[8 + 3, 8 - 3] = 0.0
    add("window 3, 48 of 49 pixels through", v=big, img=img, window=3, min_pixels=49)
    img = img.copy()
    img[8 - 3, 8 + 3] = 1.0
    add("window 3, 47 through and one in front", v=big, img=img, window=3, min_pixels=49)
    add("window 3, min_pixels 1", v=big, img=img, window=3, min_pixels=1)
    add("window 0, min_pixels 1, in front", v=big, z=1.0)
    # the angle: min_cos on its boundary, a back-facing, a zero and a NaN normal
    add("min_cos 1 on the axis", z=3.0, min_cos=1.0)
    add("min_cos 1, a short normal", s=surfel(normal=(0.0, 0.0, -0.5)), z=3.0, min_cos=1.0)
    add("min_cos 1, off the axis", s=surfel(pos=(0.25, 0.0, 2.0)), z=3.0, min_cos=1.0)
    tilted = surfel(normal=(0.6, 0.0, -0.8))
    for name, c in (("min_cos 0.8 on a 0.8 tilt", 0.8), ("min_cos just above", up(0.8)), ("min_cos just below", down(0.8)), ("min_cos 0", 0.0)):
        add(name, s=tilted, z=3.0, min_cos=float(c))
    add("a back-facing normal", s=surfel(normal=(0.0, 0.0, 1.0)), z=3.0)
    add("a normal at a right angle, min_cos 0", s=surfel(normal=(1.0, 0.0, 0.0)), z=3.0, min_cos=0.0)
    add("a zero normal", s=surfel(normal=(0.0, 0.0, 0.0)), z=3.0, min_cos=0.0)
    add("a NaN normal", s=surfel(normal=(np.nan, 0.0, -1.0)), z=3.0, min_cos=0.0)
    add("an inf normal", s=surfel(normal=(0.0, 0.0, -np.inf)), z=3.0, min_cos=0.0)
    add("a NaN position", s=surfel(pos=(np.nan, 0.0, 2.0)), z=3.0)
    # each of the four culls
    add("beyond max_depth", v=plain_view(max_depth=1.5), z=3.0)
    add("on max_depth", v=plain_view(max_depth=2.0), z=3.0)
    add("nearer than 0.4", s=surfel(pos=(0.0, 0.0, 0.3)), z=3.0)
    add("on 0.4", s=surfel(pos=(0.0, 0.0, F(0.4))), z=3.0)
    add("below min_confidence", s=surfel(conf=0.1), z=3.0)
    add("on min_confidence", s=surfel(conf=0.25), z=3.0)
    add("a NaN confidence", s=surfel(conf=np.nan), z=3.0)
    add("too old", v=plain_view(max_age=1), z=3.0)
    add("just young enough", v=plain_view(max_age=2), z=3.0)
    add("a NaN time with the age test on", s=surfel(t_last=np.nan), v=plain_view(max_age=100), z=3.0)
    add("a NaN time with the age test off", s=surfel(t_last=np.nan), z=3.0)
    # a negative fy, off the axis, tilted, under a pose
    flipped = plain_view(fy=-4.0, rows=7, cols=9, cx=4.2, cy=3.1)
    for k, pos in enumerate(((0.3, 0.4, 2.0), (0.3, -0.4, 2.0), (-0.9, 0.7, 1.7), (0.0, -1.5, 2.0))):
        add("negative fy %d" % k, s=surfel(pos=pos, normal=(0.2, -0.3, -0.9)), v=flipped, img=mixed_image(7, 9, 50 + k, zp=2.0), window=1, min_pixels=1, tol_abs=0.02, tol_rel=0.01)
    pose = np.eye(4, dtype=np.float32)
    c, s_ = np.cos(0.3), np.sin(0.3)
    pose[:3, :3] = [[c, 0, s_], [0, 1, 0], [-s_, 0, c]]
    pose[:3, 3] = (0.2, -0.1, 0.3)
    moved = plain_view(pose=pose, rows=12, cols=16, cx=7.7, cy=5.4, fx=9.0, fy=9.5)
    rng = np.random.default_rng(7)
    for k in range(40):
        pos = rng.uniform((-1.0, -1.0, 1.0), (2.0, 1.0, 4.0))
        nrm = np.array([rng.uniform(-0.8, 0.8), rng.uniform(-0.8, 0.8), -1.0])
        img = rng.uniform(*((0.5, 5.0) if k % 2 else (4.5, 7.0)), (12, 16)).astype(np.float32)
        w = int(rng.integers(0, 4))
        add("under a pose %d" % k, s=surfel(pos=pos, normal=nrm / np.linalg.norm(nrm)), v=moved, img=img, window=w, min_pixels=min(int(rng.integers(1, 4)), (2 * w + 1) ** 2),
            tol_abs=0.3, tol_rel=0.05)
    return out


# (v_through, v_support, min_votes, max_support): DECIDE with both bounds on and beside their boundaries
DECIDE_CASES = [(0, 0, 1, 0), (1, 0, 1, 0), (1, 0, 2, 0), (2, 0, 2, 0), (3, 0, 2, 0), (2, 1, 2, 0), (2, 1, 2, 1), (2, 2, 2, 1), (65535, 0, 65535, 0), (65534, 0, 65535, 0),
                (65535, 65535, 1, 65535), (65535, 65535, 1, 65534), (0, 0, 1, 65535), (5, 3, 5, 3), (5, 4, 5, 3), (4, 3, 5, 3)]


# ---- the scene: a wall at z = 3, a floor at y = 1 seen at a grazing angle, a box face at z = 1.6 ---------------------------
SCENE = dict(rows=48, cols=64, fx=52.8, fy=52.8, cx=31.5, cy=23.5)
BOX = (-0.4, 0.4, 0.0, 0.24)  # the face: x0, x1, y0, y1 at z = 1.6 (26 x 8 pixels of view A; it hides a piece of the wall only)


def scene_view(name, rows=None, cols=None, **kw):
    """views A, B and E: displaced sideways and upwards, B and E turned a little (frames have their pixel centres at integers)"""
    g = dict(SCENE)
    scale = 1.0 if cols is None else cols / g["cols"]
    T = np.eye(4, dtype=np.float32)
    if name == "B":
        T[:3, 3] = (0.25, -0.05, 0.0)
        a = -0.06
    elif name == "E":
        T[:3, 3] = (-0.3, -0.1, 0.1)
        a = 0.08
    else:
        a = 0.0
    c, s_ = np.cos(a), np.sin(a)
    T[:3, :3] = np.array([[c, 0, s_], [0, 1, 0], [-s_, 0, c]], np.float32)
    return plain_view(pose=T, cx=(g["cx"] + 0.5) * scale - 0.5, cy=(g["cy"] + 0.5) * scale - 0.5, fx=g["fx"] * scale, fy=g["fy"] * scale,
                      rows=g["rows"] if rows is None else rows, cols=g["cols"] if cols is None else cols, min_confidence=0.25, max_depth=20.0, max_age=-1, **kw)


def scene_depth(v, box, noise=0.0, seed=0):
    """the depth frame of view v, float64 ray casting rounded to float32: camera z of the nearest of wall, floor and (with `box`)
    the box face along the ray of every pixel; with `noise` a relative Gaussian error of that sigma"""
    T = np.array(v.pose, np.float64).reshape(4, 4).T
    R, t = T[:3, :3], T[:3, 3]
    u, w = np.meshgrid(np.arange(v.cols, dtype=np.float64), np.arange(v.rows, dtype=np.float64))
    ray = np.stack([(u - v.cx) / v.fx, (w - v.cy) / v.fy, np.ones_like(u)], -1) @ R.T  # world direction per unit camera z
    with np.errstate(all="ignore"):
        best = np.full(u.shape, np.inf)
        lam = (3.0 - t[2]) / ray[..., 2]  # the wall
        best = np.where(lam > 0, np.minimum(best, lam), best)
        lam = (1.0 - t[1]) / ray[..., 1]  # the floor, in front of the wall
        ok = (lam > 0) & ((t[2] + lam * ray[..., 2]) <= 3.0)
        best = np.where(ok, np.minimum(best, lam), best)
        if box:
            lam = (1.6 - t[2]) / ray[..., 2]
            x, y = t[0] + lam * ray[..., 0], t[1] + lam * ray[..., 1]
            ok = (lam > 0) & (x >= BOX[0]) & (x <= BOX[1]) & (y >= BOX[2]) & (y <= BOX[3])
            best = np.where(ok, np.minimum(best, lam), best)
    z = np.where(np.isfinite(best), best, 0.0)
    if noise:
        z = z * (1.0 + noise * np.random.default_rng(seed).standard_normal(z.shape))
    return z.astype(np.float32)


def scene_map(v, depth):
    """the map made from a view: one surfel per valid pixel in the map's point order (x outer, y inner), with the normal of the
    surface it lies on; (surfels, kind) with kind 0 wall, 1 floor, 2 box"""
    T = np.array(v.pose, np.float64).reshape(4, 4).T
    surf, kind = [], []
    for i in range(v.cols):
        for j in range(v.rows):
            z = float(depth[j, i])
            if not z > 0:
                continue
            pc = np.array([(i - v.cx) / v.fx * z, (j - v.cy) / v.fy * z, z, 1.0])
            pw = T @ pc
            if abs(pw[2] - 1.6) < 1e-3:
                k, nrm = 2, (0.0, 0.0, -1.0)
            elif abs(pw[1] - 1.0) < 1e-3:
                k, nrm = 1, (0.0, -1.0, 0.0)
            else:
                k, nrm = 0, (0.0, 0.0, -1.0)
            surf.append(surfel(pos=pw[:3], normal=nrm, conf=0.5, t_last=TICK, radius=z / v.fx))
            kind.append(k)
    return np.array(surf, np.float32).reshape(-1, 12), np.array(kind, np.int32)
