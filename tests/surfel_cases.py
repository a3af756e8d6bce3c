"""The scenes of tests/test_exact_surfels.py: seeded generators of small surfel buffers with the view they are drawn from, each
the smallest at which the drawing can still go wrong. A scene is a Case; nothing here draws anything."""
import numpy as np

from staticfusion_amd.synth import se3_exp

TICK = 5


class Case:
    def __init__(self, name, surfels, rows, cols, cx, cy, fx, fy, pose=None, min_confidence=0.25, max_depth=20.0, max_age=-1, tick=TICK,
                 ambiguous_cap=1 / 20, open_cap=1 / 50, kind="plain"):
        self.name, self.surfels = name, np.ascontiguousarray(surfels, np.float32).reshape(-1, 12)
        self.rows, self.cols, self.cx, self.cy, self.fx, self.fy = rows, cols, cx, cy, fx, fy
        self.pose = np.eye(4, dtype=np.float32) if pose is None else np.asarray(pose, np.float32)
        self.min_confidence, self.max_depth, self.max_age, self.tick = min_confidence, max_depth, max_age, tick
        # the caps of the issue: the share of drawn pixels with more than one admissible winner, of square fragments that are open
        self.ambiguous_cap, self.open_cap, self.kind = ambiguous_cap, open_cap, kind

    def __repr__(self):
        return self.name


def colour(r, g, b):
    return np.float32((int(r) << 16) + (int(g) << 8) + int(b))


def surfel(x, y, z, rad, normal=(0, 0, -1), conf=0.5, rgb=(200, 100, 50), last=TICK):
    s = np.zeros(12, np.float32)
    s[:4] = (x, y, z, conf)
    s[4] = colour(*rgb)
    s[6], s[7] = 1, last
    n = np.asarray(normal, np.float64)
    s[8:11] = n / np.linalg.norm(n)
    s[11] = rad
    return s


def scattered(n, rows, cols, cx, cy, fx, fy, seed, ordered, steep_share=0.0, z_range=(0.5, 4.0)):
    """n surfels in front of an identity camera, made as test_gpu_view.random_surfels makes them (sprites of one to a few
    pixels, confidences from a few values that tie with thresholds, last-seen ticks 1..TICK, normals tilted up to ~60 degrees,
    three NaN fields); steep_share of them are tilted between 60 and 85 degrees instead: grazing discs"""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(-2, cols + 2, n), rng.uniform(-2, rows + 2, n)
    if ordered:
        o = np.lexsort((v, u))
        u, v = u[o], v[o]
    z = rng.uniform(z_range[0], z_range[1], n)
    s = np.zeros((n, 12), np.float32)
    s[:, 0], s[:, 1], s[:, 2] = (u - cx) * z / fx, (v - cy) * z / fy, z
    s[:, 3] = rng.choice(np.array([0.1, 0.25, 0.3, 0.5], np.float32), n)
    s[:, 4] = (rng.integers(1, 256, n) << 16) + (rng.integers(1, 256, n) << 8) + rng.integers(1, 256, n)
    s[:, 6] = 1
    s[:, 7] = rng.integers(1, TICK + 1, n)
    nrm = np.stack([rng.uniform(-0.8, 0.8, n), rng.uniform(-0.8, 0.8, n), -np.ones(n)], -1)
    steep = rng.random(n) < steep_share
    tilt, turn = np.deg2rad(rng.uniform(60.0, 85.0, n)), rng.uniform(0, 2 * np.pi, n)
    graz = np.stack([np.sin(tilt) * np.cos(turn), np.sin(tilt) * np.sin(turn), -np.cos(tilt)], -1)
    nrm = np.where(steep[:, None], graz, nrm / np.linalg.norm(nrm, axis=1, keepdims=True))
    s[:, 8:11] = nrm
    s[:, 11] = z / abs(fx) * rng.uniform(0.7, 2.5, n)
    if n > 8:
        s[3, 0] = np.nan  # a NaN position: never drawn
        s[5, 3] = np.nan  # a NaN confidence: !(NaN < threshold) draws it
        s[7, 7] = np.nan  # a NaN time: drawn unless the age test is on
    return s


# ---- tilts: both splat kernels' LDS tile (ordered) and their global-atomic fallback (shuffled) ---------------------------------
TILT_VIEW = dict(rows=48, cols=64, cx=30.5, cy=25.0, fx=61.0, fy=58.5)
TILT_POSE = se3_exp(np.array([0.02, -0.03, 0.05, 0.03, -0.02, 0.05])).astype(np.float32)
# Grazing discs are the point of this scene: a disc seen at 85 degrees has dot(l, n) ~ 0.09 and every margin ten times that of
# a frontal one. That is still some 1e-5 of a pixel: section F leaves about one square fragment in 7000 open and no pixel
# ambiguous (tests/README.md has the shares per scene). Caps of its own, a few times what was measured and well inside the plain
# ones (1 in 20, 1 in 50): one drawn pixel in 200 ambiguous, one square fragment in 500 open. With one open fragment in
# thousands a buffer of ~500 surfels has one or none by chance: "open fragments exist" is asserted on the 5003-surfel buffers,
# which are the grazing scene in that sense; the buffers of 511 .. 513 are there for the workgroup size of the splat kernels.
TILT_CAPS = dict(ambiguous_cap=1 / 200, open_cap=1 / 500)


def tilts(n, ordered):
    s = scattered(n, seed=n + 48, ordered=ordered, steep_share=1 / 3, **TILT_VIEW)
    return Case("tilts-%d-%s" % (n, "ordered" if ordered else "shuffled"), s, pose=TILT_POSE, min_confidence=0.25, max_age=1, kind="grazing",
                **TILT_VIEW, **TILT_CAPS)


# ---- discs that cross the camera plane ------------------------------------------------------------------------------------------
CROSS_VIEW = dict(rows=60, cols=80, cx=40.0, cy=30.0, fx=64.0, fy=64.0)


def crossing_surfel(seed):
    """one draw of the probe that found the corner-rectangle defect: z in [0.41, 1], rad in [0.05, 1.5], a random tilt"""
    rng = np.random.default_rng(seed)
    z, rad = rng.uniform(0.41, 1.0), rng.uniform(0.05, 1.5)
    tilt, turn = np.deg2rad(rng.uniform(0.0, 80.0)), rng.uniform(0, 2 * np.pi)
    n = (np.sin(tilt) * np.cos(turn), np.sin(tilt) * np.sin(turn), -np.cos(tilt))
    return surfel(rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), z, rad, n, rgb=(9 + seed % 200, 8, 7))


# draws of crossing_surfel whose corner rectangle loses pixels that the square and the disc test draw (found on the CPU with the
# corner rectangle applied unconditionally), by the pixels of their sprite: at most SFV_LARGE_PIXELS = 1024, and more
CROSS_SEEDS_SMALL = (76,)           # an 80 x 60 image: the clipped rectangle held 880 pixels
CROSS_SEEDS_LARGE = (35, 124)       # ... 2760 and 2960 pixels (draws that leave some of the image to the small surfels)
CROSS_SEEDS_32 = (76, 61)           # a 32 x 32 image holds SFV_LARGE_PIXELS: the whole square is still the small-sprite kernel's


def crossing(seeds=None, name="crossing", view=None):
    """the crossing discs among 500 small surfels. A disc through the camera plane has rays that run along it (dot(l, n) -> 0), but
    only on a curve that passes between the pixel centres of these draws: section F leaves no fragment open and no pixel
    ambiguous here. Caps of its own, as tight as the tilts': one drawn pixel in 200 ambiguous, one square fragment in 500 open."""
    seeds = CROSS_SEEDS_SMALL + CROSS_SEEDS_LARGE if seeds is None else seeds
    view = CROSS_VIEW if view is None else view
    small = scattered(500, seed=17, ordered=True, z_range=(1.0, 3.0), **view)
    big = [crossing_surfel(k) for k in seeds]
    at = np.linspace(40, 460, len(big)).astype(int)
    parts, last = [], 0
    for p, b in zip(at, big):
        parts += [small[last:p], b[None]]
        last = p
    parts.append(small[last:])
    c = Case(name, np.concatenate(parts), min_confidence=0.0, kind="crossing", ambiguous_cap=1 / 200, open_cap=1 / 500, **view)
    c.big = at + np.arange(len(big))  # where the crossing discs are in the buffer
    return c


# ---- one sprite larger than the image, tilted ---------------------------------------------------------------------------------------
LARGE_VIEW = dict(rows=48, cols=64, cx=32.0, cy=24.0, fx=64.0, fy=64.0)


def large_sprite(where):
    small = scattered(500, seed=17, ordered=True, z_range=(1.0, 3.0), **LARGE_VIEW)
    big = surfel(0.01, -0.02, 0.45, 2.0, (0.3, -0.2, -1.0), rgb=(9, 8, 7)) if where == "in front" else surfel(0.01, -0.02, 3.5, 6.0, (0.3, -0.2, -1.0), rgb=(9, 8, 7))
    c = Case("large-" + where.replace(" ", "-"), np.concatenate([small[:250], big[None], small[250:]]), min_confidence=0.0, **LARGE_VIEW)
    c.big = np.array([250])
    return c


# ---- thresholds of the cull, under the identity pose (h is exact there) --------------------------------------------------------------
CULL_VIEW = dict(rows=30, cols=40, cx=20.0, cy=15.0, fx=32.0, fy=32.0)
CULL_MAX_DEPTH = 2.5


def cull_thresholds():
    """every surfel alone on a pixel centre, five pixels from the next, with a disc of 2.2 pixels radius (no pixel centre on the rim; the two at the far
    threshold, whose fragments are open by nature, of 0.6); `expect` says which are certainly culled (False) and which
    certainly are not (True)"""
    F = np.float32
    up, down = lambda a: np.nextafter(F(a), F(np.inf)), lambda a: np.nextafter(F(a), F(-np.inf))
    rows = [  # (z, conf, last, not culled)
        (down(0.4), 0.5, TICK, False), (F(0.4), 0.5, TICK, True), (up(0.4), 0.5, TICK, True),
        (down(CULL_MAX_DEPTH), 0.5, TICK, True), (F(CULL_MAX_DEPTH), 0.5, TICK, True), (up(CULL_MAX_DEPTH), 0.5, TICK, False),
        (F(CULL_MAX_DEPTH) * F(1 - 2.0 ** -16), 0.5, TICK, True),           # far enough inside for the depth-range test to be certain
        (1.0, down(0.25), TICK, False), (1.0, F(0.25), TICK, True), (1.0, up(0.25), TICK, True),
        (1.0, 0.5, TICK - 2, True), (1.0, 0.5, TICK - 3, False),          # tick - s[7] equal to max_age = 2 and one above
        (1.0, 0.5, TICK + 1, None),                                        # s[7] > maxTime: the prediction culls it, a view has no such test
    ]
    spots = [(2.5 + 5 * (k % 7), 7.5 + 15 * (k // 7)) for k in range(len(rows))]
    s = np.stack([surfel((u - CULL_VIEW["cx"]) * float(z) / CULL_VIEW["fx"], (v - CULL_VIEW["cy"]) * float(z) / CULL_VIEW["fy"], z,
                         (0.6 if k in (3, 4) else 2.2) * float(z) / CULL_VIEW["fx"], conf=conf, last=last, rgb=(10 + k, 20, 30))
                  for k, ((z, conf, last, _), (u, v)) in enumerate(zip(rows, spots))])
    c = Case("cull-thresholds", s, min_confidence=0.25, max_depth=CULL_MAX_DEPTH, max_age=2, **CULL_VIEW)
    c.expect = [r[3] for r in rows]
    c.spots = [(int(u), int(v)) for u, v in spots]
    c.open_by_nature = (3, 4)  # they pass the cull, but gl_FragDepth is 1.0 to within its rounding
    return c


# ---- the image border: centres that project to ndc = +-1 exactly and just outside ----------------------------------------------
BORDER_VIEW = dict(rows=32, cols=64, cx=32.0, cy=16.0, fx=32.0, fy=32.0)  # with z = 1 all dyadic: ndc is exact; x = +-1 is ndc_x = +-1


def image_border():
    """On the negative side one ulp of x outside is one ulp of the window coordinate outside (0 - 2^-18). On the positive side
    fx x + cx = 64 + 2^-18 is a tie that rounds to 64: the float ndc IS 1, and F calls the surfel open (border_ties); the first
    x that is certainly outside is two ulps out."""
    F = np.float32
    step = lambda a, k: F(a) + F(np.sign(a)) * F(k) * np.spacing(F(abs(a)))
    spots = [(F(1), F(0.1), True), (F(-1), F(-0.2), True), (step(1, 2), F(0.3), False), (step(-1, 1), F(-0.4), False),
             (F(0.5), F(0.5), True), (F(-0.5), F(-0.5), True), (F(0.25), step(0.5, 2), False), (F(-0.25), step(-0.5, 1), False)]
    s = np.stack([surfel(x, y, 1.0, 0.12, rgb=(40 + k, 50, 60)) for k, (x, y, _) in enumerate(spots)])
    c = Case("image-border", s, min_confidence=0.0, **BORDER_VIEW)
    c.expect = [sp[2] for sp in spots]
    return c


def border_ties():
    """the two centres one ulp outside on the positive side: exact ndc above 1, float ndc equal to 1"""
    F = np.float32
    return np.stack([surfel(np.nextafter(F(1), F(2)), F(0.3), 1.0, 0.12), surfel(F(0.25), np.nextafter(F(0.5), F(1)), 1.0, 0.12)])


def tiny_image():
    s = np.stack([surfel(0.0, 0.0, 1.0, 0.3, rgb=(1, 2, 3)), surfel(0.05, 0.02, 0.8, 0.2, (0.2, 0.1, -1.0), rgb=(4, 5, 6)), surfel(0.0, 0.0, 3.0, 5.0, rgb=(7, 8, 9))])
    return Case("tiny-1x1", s, rows=1, cols=1, cx=0.5, cy=0.5, fx=1.3, fy=1.1, min_confidence=0.0)


def duplicates():
    """64 records, each three times, at scattered positions of a shuffled buffer of 664"""
    v = dict(rows=48, cols=64, cx=30.5, cy=25.0, fx=61.0, fy=58.5)
    base = scattered(472, seed=23, ordered=False, **v)
    rng = np.random.default_rng(29)
    dup = scattered(80, seed=31, ordered=False, z_range=(0.5, 1.2), **v)[8:72]  # near: they win pixels
    dup[:, 3] = 0.5
    allrec = np.concatenate([base, dup, dup, dup])
    return Case("duplicates", allrec[rng.permutation(allrec.shape[0])], min_confidence=0.25, **v)


def crossing_small():
    return crossing(CROSS_SEEDS_32, "crossing-32x32", dict(rows=32, cols=32, cx=16.0, cy=16.0, fx=26.0, fy=26.0))


# ---- the composition: density test, fill-in, extraction ------------------------------------------------------------------------------
def composition(rows, cols, mp, on_samples, sample_positions, zero_channel=False):
    """Single fronto-parallel surfels of 0.6 pixels radius on pixel centres, seen from the identity pose with the handle's own
    intrinsics `mp`: high-confidence ones on the first `on_samples` of the pixels the density test samples (and, with
    zero_channel, one more there whose red byte is 0), a patch of low-confidence and a patch of high-confidence ones elsewhere,
    and black surfels of either confidence. Colours have every channel >= 1 unless said otherwise."""
    rng = np.random.default_rng(rows + on_samples)
    out = []

    def at(i, j, z, conf, rgb):
        out.append(surfel((i + 0.5 - mp.cx) * z / mp.fx, (j + 0.5 - mp.cy) * z / mp.fy, z, 0.6 * z / abs(mp.fx), conf=conf, rgb=rgb))

    for k in range(on_samples):
        at(sample_positions[k][1], sample_positions[k][0], 1.5, 0.5, tuple(rng.integers(1, 256, 3)))
    if zero_channel:
        at(sample_positions[on_samples][1], sample_positions[on_samples][0], 1.5, 0.5, (0, 200, 100))
    for i in range(3, 9):  # low confidence only: drawn in the low target; high confidence: in both
        for j in range(3, 9):
            at(i, j, 1.2 + 0.01 * i, 0.2, tuple(rng.integers(1, 256, 3)))
            at(i + 12, j, 1.8 - 0.01 * j, 0.5, tuple(rng.integers(1, 256, 3)))
    at(4, 12, 1.4, 0.5, (0, 0, 0))    # black, in both targets: keeps its depth, takes the fill-in colour
    at(7, 12, 1.4, 0.2, (0, 0, 0))    # black, in the low target only
    at(10, 12, 1.4, 0.5, (0, 0, 0))   # black in the high target behind a coloured low-confidence surfel that wins the low one
    at(10, 12, 1.2, 0.2, (90, 80, 70))
    at(13, 12, 1.4, 0.5, (0, 0, 255))  # one channel: not black
    at(16, 12, 3.0, 0.5, (5, 6, 7))    # beyond extract_max_depth = 2
    return np.stack(out)
