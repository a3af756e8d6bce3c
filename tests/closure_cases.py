"""Shared scenes of the closure tests (test_closure_*_cpu.py, test_gpu_closure.py): parameter sets without the product's
types, views of the geometries the score tests use, clouds of surfels in front of a view with depths close enough for the gates
to bite and init times for the time gap to bite, the table of the PER SAMPLE rule, and the doubled wall of a drifted walk.
References are computed once per process (functools.lru_cache) and never changed."""
import functools
import types

import numpy as np

import closure_ref as cr
from staticfusion_amd import view
from staticfusion_amd.synth import se3_exp

F = np.float32
TICK = 9
# cols, rows, cx, cy, fx, fy (the order of GEOMS in tests/test_gpu_score.py; 53 x 37 has its negative fy)
GEOMS = {"1x1": (1, 1, 0.5, 0.5, 1.3, 1.1), "1x65": (1, 65, 0.5, 33.0, 40.0, 40.0), "257x1": (257, 1, 128.0, 0.5, 150.0, 150.0),
         "16x16": (16, 16, 8.0, 7.5, 20.0, 21.0), "53x37": (53, 37, 25.25, 19.5, 47.0, -44.0), "64x48": (64, 48, 30.5, 25.0, 61.0, 58.5)}
POSE_FROM = se3_exp(np.array([0.02, -0.03, 0.05, 0.03, -0.02, 0.05])).astype(F)
POSE_TO = se3_exp(np.array([0.025, -0.02, 0.04, 0.02, -0.025, 0.04])).astype(F)


def params(**kw):
    """the parameters as a plain namespace (closure_ref reads members); defaults: those of the header"""
    return types.SimpleNamespace(**dict(cr.DEFAULTS, **kw))


def as_product(p):
    from staticfusion_amd import closure

    return closure.Params(**vars(p))


def geom_view(g, pose, **kw):
    cols, rows, cx, cy, fx, fy = g
    kw.setdefault("min_confidence", 0.0)
    return view.View(pose, cx, cy, fx, fy, rows, cols, **kw)


def cloud(g, pose, n, seed, z0=2.0, sigma=0.04, times=10, radius=1.3, rows_without=None):
    """n surfels as a camera with geometry g at `pose` sees them: random pixel positions (a little beyond the rim), depths
    z0 + N(0, sigma), facing the camera, discs of about `radius` pixels, init times 0 .. times - 1, last-seen times 1 .. TICK,
    a few confidences; rows_without = (lo, hi): no surfel whose centre lies in those pixel rows"""
    cols, rows, cx, cy, fx, fy = g
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(-1, cols + 1, n), rng.uniform(-1, rows + 1, n)
    if rows_without is not None:
        lo, hi = rows_without
        inside = (v >= lo - 3) & (v < hi + 3)  # (three pixels clear on both sides: no disc reaches in)
        v = np.where(inside, rng.uniform(hi + 3, rows + 1, n), v)
    z = z0 + rng.normal(0, sigma, n)
    cam = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], axis=1)
    R, t = pose[:3, :3].astype(np.float64), pose[:3, 3].astype(np.float64)
    s = np.zeros((n, 12), F)
    s[:, 0:3] = cam @ R.T + t
    s[:, 3] = rng.choice(np.array([0.1, 0.25, 0.5, 1.0], F), n)
    s[:, 4] = (rng.integers(1, 256, n) << 16) + (rng.integers(1, 256, n) << 8) + rng.integers(1, 256, n)
    s[:, 5] = 1
    s[:, 6] = rng.integers(0, times, n)
    s[:, 7] = rng.integers(1, TICK + 1, n)
    nrm = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), -np.ones(n)], -1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    s[:, 8:11] = nrm @ R.T
    s[:, 11] = z / min(abs(fx), abs(fy)) * radius
    return np.ascontiguousarray(s, F)


def entry(gname, n_new, n_old, seed, p, same=False, age=-1, special=False, rows_without=None, poses=(POSE_FROM, POSE_TO)):
    """(surf_new, TICK, surf_old, TICK, view_from, view_to, params) as closure_ref.build takes it; same: map_old is map_new"""
    g = GEOMS[gname]
    vf, vt = geom_view(g, poses[0], max_age=age), geom_view(g, poses[1])
    new = cloud(g, poses[0], n_new, seed)
    old = new if same else cloud(g, poses[1], n_old, seed + 1000, rows_without=rows_without)
    if special and not same:  # times that are not finite: a NaN time never links and drops its pin, an inf time drops its link
        new[np.arange(n_new) % 5 == 1, 6] = np.inf
        new[np.arange(n_new) % 7 == 2, 6] = np.nan
        old[np.arange(n_old) % 6 == 3, 6] = np.nan
        old[np.arange(n_old) % 11 == 4, 6] = -np.inf
    return (new, TICK, old, TICK, vf, vt, p)


@functools.lru_cache(maxsize=None)
def reference(key):
    """closure_ref.build of the entries CASES[key] names, computed once"""
    return cr.build(CASES[key]())


# name -> a function returning the list of entries (built anew for every caller; the reference is cached by name)
CASES = {}
for _g, _strides in (("1x1", (1, 2, 4096)), ("1x65", (1, 2, 64)), ("257x1", (1,)), ("16x16", (1, 2, 3)), ("53x37", (1, 7)), ("64x48", (1, 3, 7, 64, 4096))):
    for _s in _strides:
        for _pins in ((0, 1, 2) if (_g, _s) in (("16x16", 1), ("64x48", 3)) else (2,) if _s == 7 else (1,)):
            CASES["%s/s%d/p%d" % (_g, _s, _pins)] = functools.partial(
                lambda g, s, pins: [entry(g, 700, 700, 11 * s + pins, params(stride=s, pins=pins, gate_abs=0.03, gate_rel=0.005, min_time_gap=0.0), special=True)],
                _g, _s, _pins)
for _n in (0, 1, 255, 257, 1025):  # map sizes, another old map and the same map
    CASES["count/%d" % _n] = functools.partial(lambda n: [entry("64x48", n, max(n, 1) if n != 1 else 0, 40 + n, params(stride=2, pins=2, gate_abs=0.05, gate_rel=0.0))], _n)
    CASES["same/%d" % _n] = functools.partial(lambda n: [entry("64x48", n, n, 50 + n, params(stride=2, pins=2, min_time_gap=-np.inf), same=True, poses=(POSE_FROM, POSE_FROM))], _n)
CASES["age"] = lambda: [entry("64x48", 900, 900, 61, params(stride=1, gate_abs=np.inf, gate_rel=0.0, min_time_gap=-np.inf), age=2)]  # last-seen within 2 of 9 ticks: a third
CASES["all"] = lambda: [entry("16x16", 1025, 0, 62, params(stride=1, pins=1, gate_abs=np.inf, min_time_gap=-np.inf), same=True, poses=(POSE_FROM, POSE_FROM))]
CASES["none"] = lambda: [entry("16x16", 700, 700, 63, params(stride=1, pins=1, gate_abs=0.0, gate_rel=0.0, min_time_gap=100.0))]
CASES["gap"] = lambda: [entry("64x48", 900, 900, 64, params(stride=1, pins=1, gate_abs=np.inf, min_time_gap=0.0))]
CASES["hole"] = lambda: [entry("64x48", 2000, 2000, 65, params(stride=1, pins=2, gate_abs=np.inf, min_time_gap=-np.inf), rows_without=(16, 24))]
CASES["batch"] = lambda: [CASES[k]()[0] for k in ("64x48/s1/p1", "1x1/s2/p1", "16x16/s1/p2", "count/257", "same/1025")]


# ---- the table of the PER SAMPLE rule ------------------------------------------------------------------------------------------
def _surfel(pos, time):
    s = np.zeros(12, F)
    s[0:3], s[3], s[6], s[7], s[10], s[11] = pos, 1.0, time, time, -1.0, 0.01
    return s


def rule_table():
    """[(name, sa or None, so or None, zA, zO, pose_from, pose_to, params)]: each absence; dz exactly on the gate and one ulp beyond
    it; gate_abs 0 and +inf; min_time_gap on the boundary and -inf; NaN / inf times and positions; every pins mode"""
    a, o = _surfel([0.1, -0.2, 2.0], 12.0), _surfel([0.11, -0.19, 2.01], 3.0)
    up = lambda x: np.nextafter(F(x), F(np.inf))  # noqa: E731
    out = []
    for pins in (0, 1, 2):
        base = dict(pins=pins)
        out += [("plain", a, o, 2.0, 2.01, base), ("no a", None, o, 0.0, 2.01, base), ("no o", a, None, 2.0, 0.0, base), ("neither", None, None, 0.0, 0.0, base)]
        dyadic = dict(base, gate_abs=0.125, gate_rel=0.0625)  # at zO = 2 the gate is 0.25, and every float here is exact
        out += [("on the gate", a, o, 2.25, 2.0, dyadic), ("one ulp beyond", a, o, up(2.25), 2.0, dyadic), ("on the gate from below", a, o, 1.75, 2.0, dyadic),
                ("one ulp beyond from below", a, o, np.nextafter(F(1.75), F(0)), 2.0, dyadic)]
        out += [("gate 0 equal", a, o, 2.0, 2.0, dict(base, gate_abs=0.0, gate_rel=0.0)), ("gate 0 apart", a, o, up(2.0), 2.0, dict(base, gate_abs=0.0, gate_rel=0.0)),
                ("gate inf", a, o, 2.0, 19.0, dict(base, gate_abs=np.inf)), ("gate inf, clip", a, o, 0.5, 39.0, dict(base, gate_abs=np.inf))]
        out += [("gap on the boundary", a, o, 2.0, 2.01, dict(base, min_time_gap=9.0)), ("gap just inside", a, o, 2.0, 2.01, dict(base, min_time_gap=float(np.nextafter(F(9), F(0))))),
                ("gap -inf", _surfel([0.1, -0.2, 2.0], -50.0), o, 2.0, 2.01, dict(base, min_time_gap=-np.inf)), ("gap negative", _surfel([0, 0, 2], 1.0), o, 2.0, 2.01, base)]
        for name, sa, so in (("a time NaN", _surfel([0.1, -0.2, 2.0], np.nan), o), ("a time inf", _surfel([0.1, -0.2, 2.0], np.inf), o),
                             ("o time NaN", a, _surfel([0.11, -0.19, 2.01], np.nan)), ("o time -inf", a, _surfel([0.11, -0.19, 2.01], -np.inf)),
                             ("a position NaN", _surfel([np.nan, -0.2, 2.0], 12.0), o), ("a position inf", _surfel([0.1, np.inf, 2.0], 12.0), o),
                             ("o position NaN", a, _surfel([0.11, -0.19, np.nan], 3.0)), ("o position inf", a, _surfel([-np.inf, -0.19, 2.01], 3.0)),
                             ("both times inf", _surfel([0.1, -0.2, 2.0], np.inf), _surfel([0.11, -0.19, 2.01], np.inf))):
            out.append((name, sa, so, 2.0, 2.01, base))
        out.append(("dst overflows", _surfel([3e38, 0, 2], 12.0), o, 2.0, 2.01, dict(base, w_link=0.0, w_pin=2.5)))
    far = np.eye(4, dtype=F)
    far[:3, 3] = [3e38, 0, 0]
    rows = []
    for name, sa, so, zA, zO, kw in out:
        pose_to = far if name == "dst overflows" else POSE_TO
        rows.append((name, sa, so, F(zA), F(zO), POSE_FROM, pose_to, params(**kw)))
    return rows


# ---- the doubled wall -----------------------------------------------------------------------------------------------------------
WALL_GEOM = (64, 48, 31.5, 23.5, 60.0, 60.0)
WALL_SHIFT = np.array([0.0625, -0.03125, 0.046875])  # the drift of the believed pose: a pure translation, dyadic


def doubled_wall():
    """A wall 2 m in front of a camera at the origin, seen twice: the first sighting put it where it is (init times 1, 2), the
    second -- under a believed pose WALL_SHIFT off -- put the same surface WALL_SHIFT away (init times 20, 21). One map holds
    both. The believed pose sees the recent copy exactly as the refined pose (identity) sees the old one.
    Returns (surfels of the whole map, surfels of the old part, view_from, view_to, tick)."""
    cols, rows, cx, cy, fx, fy = WALL_GEOM
    u, v = np.meshgrid(np.arange(cols, dtype=np.float64) + 0.5, np.arange(rows, dtype=np.float64) + 0.5)
    z = 2.0 + 0.1 * np.sin(u / 9.0) * np.cos(v / 7.0)
    p = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], axis=-1).reshape(-1, 3)
    n = p.shape[0]
    old = np.zeros((n, 12), F)
    old[:, 0:3] = p
    old[:, 3], old[:, 4], old[:, 5] = 1.0, 0x808080, 1.0
    old[:, 6] = 1 + np.arange(n) % 2
    old[:, 7] = old[:, 6]
    old[:, 10] = -1.0
    old[:, 11] = (z.ravel() / fx) * 1.2
    new = old.copy()
    new[:, 0:3] = (p + WALL_SHIFT).astype(F)
    new[:, 6] = 20 + np.arange(n) % 2
    new[:, 7] = new[:, 6]
    believed = np.eye(4, dtype=F)
    believed[:3, 3] = WALL_SHIFT
    tick = 22
    vf = geom_view(WALL_GEOM, believed, max_age=3)  # the active part: seen within the last 3 ticks
    vt = geom_view(WALL_GEOM, np.eye(4, dtype=F))
    return np.concatenate([old, new]), old, vf, vt, tick
