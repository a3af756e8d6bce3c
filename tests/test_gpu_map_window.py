"""Bounded surfel maps (include/sf_map_window.h, staticfusion_amd/map_window.py) on the GPU: count, cull, extract, page out and
append against `s[mask]` in NumPy, the mask computed in np.float32 in the order the header writes the tests, bit for bit;
the batch against single calls; the buffers' limits; the state a cull leaves; every refusal; and the turning walk of
tests/test_map_window_walk_cpu.py kept inside its capacity by sfw_cull_maps, equal at every frame to the same walk windowed
by download, NumPy and upload."""
import ctypes as C

import numpy as np
import pytest

from conftest import driver_params, make_solver
from staticfusion_amd import SfError, SurfelMap, map_window, streams
from staticfusion_amd.map_window import Filter
from test_map_fusion import same_bits
from test_map_window_walk_cpu import CAPACITY, MAX_AGE, numpy_age_cull, turn_walk

pytestmark = pytest.mark.gpu

ROWS, COLS = 120, 160
TICK = 10
BIG = 262144 + 257  # more than 1024 blocks of 256: the second trip of the scan
CENTRE = (1.0, -2.0, 0.5)
_fp = C.POINTER(C.c_float)
POSE = np.array([[0, -1, 0, 0.25], [1, 0, 0, -1.5], [0, 0, 1, 2.0], [0, 0, 0, 1]], np.float32)


def random_surfels(n, seed):
    """n surfels in the layout of sf.h; among them NaN / inf positions, confidences and times and exact ties of the three tests
    of the filters below (confidence 0.5, age 3 at tick 10, a point (3, 4, 0) from CENTRE at radius 5)"""
    rng = np.random.default_rng(seed)
    s = rng.uniform(-1.0, 1.0, (n, 12)).astype(np.float32)
    s[:, 0:3] = rng.uniform(-6.0, 6.0, (n, 3))
    s[:, 3] = rng.uniform(0.0, 1.0, n)
    s[:, 7] = rng.integers(1, TICK + 1, n)
    s[:, 6] = np.minimum(s[:, 7], rng.integers(1, TICK + 1, n))
    s[:, 11] = rng.uniform(0.001, 0.05, n)
    special = [
        (0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (3, np.inf), (3, -np.inf), (7, np.nan), (7, np.inf),
        (3, 0.5), (3, np.nextafter(np.float32(0.5), np.float32(0))), (3, np.nextafter(np.float32(0.5), np.float32(1))),
        (7, TICK - 3), (7, TICK - 4), (7, TICK - 2), (7, TICK), (7, TICK + 1), (7, -2.0),
    ]
    for j, (col, v) in enumerate(special):
        if n:
            s[(j * 7 + 3) % n, col] = v
    if n > 130:  # the ties of the radius test: exactly on the sphere, one float inside, one float outside
        for j, d in enumerate(((3, 4, 0), (0, -3, 4), (-4, 0, 3), (5, 0, 0))):
            s[125 + j, 0:3] = np.array(CENTRE, np.float32) + np.array(d, np.float32)
        s[129, 0:3] = np.array(CENTRE, np.float32) + np.array((3, np.nextafter(np.float32(4), np.float32(5)), 0), np.float32)
        s[130, 0:3] = np.array(CENTRE, np.float32) + np.array((3, np.nextafter(np.float32(4), np.float32(3)), 0), np.float32)
    elif n:
        s[n // 2, 0:3] = np.array(CENTRE, np.float32) + np.array((3, 4, 0), np.float32)
    return s


def np_mask(s, tick, f):
    """include/sf_map_window.h, THE FILTER, in np.float32 in the order written; a comparison with NaN is false"""
    s = np.asarray(s, np.float32)
    sel = np.ones(s.shape[0], bool)
    with np.errstate(all="ignore"):
        if f.min_confidence > 0:
            sel &= s[:, 3] >= np.float32(f.min_confidence)
        if f.max_age >= 0:
            sel &= (np.float32(tick) - s[:, 7]) <= np.float32(f.max_age)
        if f.radius > 0:
            dx, dy, dz = (s[:, k] - np.float32(f.centre[k]) for k in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == np.float32
            sel &= d2 <= np.float32(f.radius) * np.float32(f.radius)
    return ~sel if f.invert else sel


def filters():
    kw = [dict(min_confidence=0.5), dict(max_age=3), dict(centre=CENTRE, radius=5.0), dict(min_confidence=0.5, max_age=3, centre=CENTRE, radius=5.0)]
    out = [("%s%s" % ("+".join(sorted(k)), "/inv" if inv else ""), Filter(invert=inv, **k)) for k in kw for inv in (False, True)]
    out.append(("none", Filter()))
    out.append(("nothing: none/inv", Filter(invert=True)))
    out.append(("nothing: far", Filter(centre=(100.0, 100.0, 100.0), radius=0.001)))
    out.append(("age 0", Filter(max_age=0)))
    return out


@pytest.fixture(scope="module")
def box(hip_auto):
    s = make_solver(hip_auto, ROWS, COLS, driver_params(hip_auto))
    m = SurfelMap(s, 300000)
    yield s, m
    m.close()
    s.close()


def state(m):
    i = m.info()
    return i["count"], i["tick"], i["pose"].tobytes(), tuple(i["stats"]), m.download().tobytes()


# ---- 1. sizes and filters ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1025, BIG])
def test_count_cull_extract_and_page_out_agree_with_numpy(box, n):
    s, m = box
    surf = random_surfels(n, seed=100 + n % 97)
    for name, f in filters():
        mask = np_mask(surf, TICK, f)
        if n > 130 and name == "centre+radius":
            assert mask[125:129].all() and not mask[129] and mask[130]  # the ties hold, one float beyond does not
        k = int(mask.sum())
        m.upload(surf, POSE, TICK)
        assert map_window.count([m], [f]) == [k], name
        got = map_window.extract(m, f)
        assert got.shape == (k, 12) and same_bits(got, surf[mask]), name
        assert m.info()["count"] == n and same_bits(m.download(), surf), name  # extract changes nothing
        paged = map_window.page_out(m, f)
        assert paged.shape == (n - k, 12) and same_bits(paged, surf[~mask]), name
        kept = m.download()
        assert m.info()["count"] == k and same_bits(kept, surf[mask]), name
        both = np.zeros_like(surf)
        both[mask], both[~mask] = kept, paged
        assert same_bits(both, surf), name  # the two sets together are the old map
        m.upload(surf, POSE, TICK)
        assert map_window.cull([m], [f]) == [k], name
        info = m.info()
        assert info["count"] == k and info["tick"] == TICK and np.array_equal(info["pose"], POSE), name
        assert same_bits(m.download(), surf[mask]), name
    if n == BIG:  # the filters above do select, and differently
        ks = [int(np_mask(surf, TICK, f).sum()) for _, f in filters()]
        assert len(set(ks)) >= 10 and 0 in ks and n in ks


# ---- 2. batch ----------------------------------------------------------------------------------------------------
def test_a_batch_equals_single_calls_and_numpy(box):
    s, _ = box
    counts = [0, 257, 70000, 1, 300, 500]
    fl = [Filter(max_age=3), Filter(min_confidence=0.5, invert=True), Filter(centre=CENTRE, radius=5.0, max_age=5), Filter(), Filter(invert=True), Filter(max_age=0)]
    ticks = [TICK, TICK - 1, TICK, TICK + 2, TICK, TICK]
    data = [random_surfels(n, seed=7 + q) for q, n in enumerate(counts)]
    want = [d[np_mask(d, t, f)] for d, t, f in zip(data, ticks, fl)]
    results = []
    for batched in (True, False):
        maps = [SurfelMap(s, max(n, ROWS * COLS)) for n in counts]
        for m, d, t in zip(maps, data, ticks):
            m.upload(d, POSE, t)
        if batched:
            assert map_window.count(maps[:5], fl[:5]) == [w.shape[0] for w in want[:5]]
            kept = map_window.cull(maps[:5], fl[:5])  # one sfw_cull_maps; the sixth map is not named
        else:
            kept = [map_window.cull([m], [f])[0] for m, f in zip(maps[:5], fl[:5])]
        assert kept == [w.shape[0] for w in want[:5]]
        results.append([m.download() for m in maps])
        assert [m.info()["count"] for m in maps] == kept + [counts[5]]
        assert [m.info()["tick"] for m in maps] == ticks
        for m in maps:
            m.close()
    for q in range(5):
        assert same_bits(results[0][q], want[q]) and same_bits(results[1][q], want[q]), q
    assert same_bits(results[0][5], data[5]) and same_bits(results[1][5], data[5])
    assert [w.shape[0] for w in want[:5]][3:] == [1, 0] and 0 < want[2].shape[0] < 70000


# ---- 3. buffers --------------------------------------------------------------------------------------------------
def test_buffer_limits_of_extract_page_out_and_append(box):
    s, _ = box
    b = map_window._bind(s.api)
    cap = ROWS * COLS
    m = SurfelMap(s, cap)
    surf = random_surfels(1000, seed=3)
    m.upload(surf, POSE, TICK)
    f = Filter(max_age=3)
    mask = np_mask(surf, TICK, f)
    k = int(mask.sum())
    assert 1 < k < 999
    before = state(m)
    for fn, need in ((b.extract, k), (b.page_out, 1000 - k)):
        canary = np.full((need, 12), -77.25, np.float32)
        got = C.c_int32(-5)
        assert fn(m.m, C.byref(f), canary.ctypes.data_as(_fp), need - 1, C.byref(got)) == -1  # SF_ERR_ARG
        assert got.value == need and np.all(canary == np.float32(-77.25)) and state(m) == before
        got = C.c_int32(-5)
        assert fn(m.m, C.byref(f), None, 0, C.byref(got)) == -1 and got.value == need and state(m) == before  # the size query
    # nothing selected / nothing to page: the size query is SF_OK
    got = C.c_int32(-5)
    assert b.extract(m.m, C.byref(Filter(invert=True)), None, 0, C.byref(got)) == 0 and got.value == 0
    assert b.page_out(m.m, C.byref(Filter()), None, 0, C.byref(got)) == 0 and got.value == 0 and state(m) == before
    # page out, then page in: the kept surfels followed by the paged ones
    paged = map_window.page_out(m, f)
    assert m.info()["count"] == k
    map_window.append(m, paged)
    assert m.info()["count"] == 1000 and m.info()["tick"] == TICK
    assert same_bits(m.download(), np.concatenate([surf[mask], surf[~mask]]))
    # up to exactly the capacity, and not one more
    fill = random_surfels(cap - 1000, seed=4)
    map_window.append(m, fill)
    assert m.info()["count"] == cap
    full = np.concatenate([surf[mask], surf[~mask], fill])
    assert same_bits(m.download(), full)
    before = state(m)
    assert b.append(m.m, surf.ctypes.data_as(_fp), 1) == -3  # SF_ERR_STATE
    with pytest.raises(SfError, match="capacity"):
        map_window.append(m, surf[:1])
    assert state(m) == before
    map_window.append(m, surf[:0])  # nothing appended is fine
    assert state(m) == before
    # a full map is partitioned like any other
    g = Filter(min_confidence=0.5)
    assert map_window.cull([m], [g]) == [int(np_mask(full, TICK, g).sum())]
    assert same_bits(m.download(), full[np_mask(full, TICK, g)])
    m.close()


# ---- 4. state after a cull ---------------------------------------------------------------------------------------
def test_state_after_a_cull(hip_auto):
    from test_map_fusion import COLS as QC, ROWS as QR, load_view
    from test_model_prediction import synthetic_view
    from staticfusion_amd.synth import se3_exp
    from test_map_window_walk_cpu import TURN

    A = make_solver(hip_auto, QR, QC, driver_params(hip_auto))
    B = make_solver(hip_auto, QR, QC, driver_params(hip_auto))
    m = SurfelMap(A, CAPACITY)
    T = np.eye(4)
    for k in range(2):
        depth, rgb = synthetic_view(T, sphere=False)
        load_view(A, depth, rgb, np.full(24, 0.9, np.float32))
        m.fuse_frame(0, None if k == 0 else se3_exp(TURN))
        T = T @ se3_exp(TURN)
    assert m.index_map().max() > 0  # the second fuse rendered an index image
    info, surf = m.info(), m.download()
    centre = map_window.camera_centre(m)
    assert np.array_equal(centre, info["pose"][:3, 3])
    f = Filter(centre=centre, radius=float(np.median(np.linalg.norm(surf[:, :3] - centre, axis=1))), min_confidence=0.05)  # the near half
    mask = np_mask(surf, info["tick"], f)
    assert 0 < mask.sum() < surf.shape[0]
    assert map_window.cull([m], [f]) == [int(mask.sum())]
    with pytest.raises(SfError, match="index map"):
        m.index_map()
    after = m.info()
    assert after["tick"] == info["tick"] and np.array_equal(after["pose"], info["pose"]) and after["stats"] == info["stats"]
    # the prediction straight after the cull is the prediction from the NumPy-filtered array
    m.predict(0)
    d1, i1 = A.prediction()
    mp = A.default_model_params()
    mp.time = mp.max_time = info["tick"]
    A.predict_from_model(0, surf[mask], info["pose"], mp)
    d2, i2 = A.prediction()
    assert same_bits(d1, d2) and same_bits(i1, i2) and (d1 > 0).any()
    # the map follows its stream to another handle and is culled there
    streams.rebind_map(m, B)
    g = Filter(max_age=0, invert=True)
    kept = surf[mask]
    mask2 = np_mask(kept, info["tick"], g)
    b = map_window._bind(hip_auto)
    one = (C.c_void_p * 1)(m.m.value)
    n_out = (C.c_int32 * 1)(-5)
    assert b.cull_maps(A.h, 1, one, C.byref(g), n_out) == -1 and n_out[0] == -5  # the old handle no longer owns it
    assert map_window.cull([m], [g]) == [int(mask2.sum())]
    assert same_bits(m.download(), kept[mask2])
    # ... and fuses on there: a new index image
    depth, rgb = synthetic_view(T, sphere=False)
    load_view(B, depth, rgb, np.full(24, 0.9, np.float32))
    m.fuse_frame(0, se3_exp(TURN))
    assert m.index_map().max() > 0
    m.close()
    A.close()
    B.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(box, hip_auto):
    s, _ = box
    b = map_window._bind(s.api)
    m1, m2 = SurfelMap(s, ROWS * COLS), SurfelMap(s, ROWS * COLS)
    d1, d2 = random_surfels(300, seed=1), random_surfels(65, seed=2)
    m1.upload(d1, POSE, TICK)
    m2.upload(d2, POSE, TICK)
    other = make_solver(hip_auto, ROWS, COLS, driver_params(hip_auto))
    mo = SurfelMap(other, ROWS * COLS)
    mo.upload(d2, POSE, TICK)
    before = [state(m) for m in (m1, m2, mo)]
    two = (C.c_void_p * 2)(m1.m.value, m2.m.value)
    twice = (C.c_void_p * 2)(m1.m.value, m1.m.value)
    foreign = (C.c_void_p * 2)(m1.m.value, mo.m.value)
    with_null = (C.c_void_p * 2)(m1.m.value, None)
    fl = (map_window.SfwFilter * 2)(Filter(max_age=3), Filter(max_age=3))
    nan = float("nan")
    bad = [(map_window.SfwFilter * 2)(Filter(max_age=3), Filter(**kw)) for kw in (dict(min_confidence=nan), dict(radius=nan), dict(centre=(0, nan, 0)))]
    out = (C.c_int32 * 2)(-5, -5)
    buf = np.full((400, 12), -77.25, np.float32)
    got = C.c_int32(-5)
    for fn in (b.count_maps, b.cull_maps):
        cases = [(None, 2, two, fl, out), (s.h, 2, None, fl, out), (s.h, 2, two, None, out), (s.h, 2, two, fl, None), (s.h, -1, two, fl, out),
                 (s.h, 2, foreign, fl, out), (other.h, 2, two, fl, out), (s.h, 2, twice, fl, out), (s.h, 2, with_null, fl, out)]
        cases += [(s.h, 2, two, x, out) for x in bad]
        for q, args in enumerate(cases):
            assert fn(*args) == -1, q
            assert s.api.last_error(), q
        assert fn(s.h, 0, None, None, None) == 0  # an empty batch is fine
    for fn in (b.extract, b.page_out):
        f = fl[0]
        cases = [(None, C.byref(f), buf.ctypes.data_as(_fp), 400, C.byref(got)), (m1.m, None, buf.ctypes.data_as(_fp), 400, C.byref(got)),
                 (m1.m, C.byref(f), None, 400, C.byref(got)), (m1.m, C.byref(f), buf.ctypes.data_as(_fp), -1, C.byref(got)),
                 (m1.m, C.byref(f), buf.ctypes.data_as(_fp), 400, None), (m1.m, C.byref(bad[0][1]), buf.ctypes.data_as(_fp), 400, C.byref(got))]
        for q, args in enumerate(cases):
            assert fn(*args) == -1, q
    assert b.append(None, buf.ctypes.data_as(_fp), 1) == -1 and b.append(m1.m, None, 1) == -1 and b.append(m1.m, buf.ctypes.data_as(_fp), -1) == -1
    with pytest.raises(SfError):
        map_window.cull([m1, mo], [Filter(), Filter()])  # maps of two solvers
    with pytest.raises(SfError):
        map_window.cull([m1, m1], [Filter(max_age=3), Filter(max_age=3)])
    with pytest.raises(SfError):
        map_window.count([m1], [Filter(radius=nan)])
    assert out[0] == -5 and out[1] == -5 and got.value == -5 and np.all(buf == np.float32(-77.25))
    assert [state(m) for m in (m1, m2, mo)] == before
    # the handle goes first (test_map_fusion._density_and_orphans): the map is an empty shell that fails cleanly
    other.close()
    assert mo.info()["count"] == 65
    one = (C.c_void_p * 1)(mo.m.value)
    f = Filter(max_age=3)
    assert b.count_maps(s.h, 1, one, C.byref(f), out) == -3 and b.cull_maps(s.h, 1, one, C.byref(f), out) == -3  # SF_ERR_STATE
    assert b.extract(mo.m, C.byref(f), buf.ctypes.data_as(_fp), 400, C.byref(got)) == -3
    assert b.page_out(mo.m, C.byref(f), buf.ctypes.data_as(_fp), 400, C.byref(got)) == -3
    assert b.append(mo.m, buf.ctypes.data_as(_fp), 1) == -3
    assert mo.info()["count"] == 65 and np.all(buf == np.float32(-77.25))
    # and the live maps still work
    assert map_window.cull([m1, m2], [Filter(max_age=3), Filter(max_age=3)]) == [int(np_mask(d, TICK, f).sum()) for d in (d1, d2)]
    for m in (m1, m2, mo):
        m.close()


# ---- 6. end to end -----------------------------------------------------------------------------------------------
def test_the_turning_walk_stays_inside_its_capacity_with_sfw_cull_maps(hip_auto):
    window = Filter(max_age=MAX_AGE)
    kept = []

    def device_cull(m):
        before = m.info()["count"]
        kept.append((before, map_window.cull([m], [window])[0]))

    a = turn_walk(hip_auto, device_cull)       # route A: sfw_cull_maps before each fuse
    b = turn_walk(hip_auto, numpy_age_cull)    # route B: download, NumPy, upload
    assert len(a) == len(b) == 5
    for k, (x, y) in enumerate(zip(a, b)):
        assert x["err"] is None and y["err"] is None, k
        assert x["info"]["count"] == y["info"]["count"] and x["info"]["tick"] == y["info"]["tick"] == k + 2, k
        assert np.array_equal(x["info"]["pose"], y["info"]["pose"]) and x["info"]["stats"] == y["info"]["stats"], k
        assert same_bits(x["surfels"], y["surfels"]), k
        assert (x["index"] is None and y["index"] is None and k == 0) or np.array_equal(x["index"], y["index"]), k
        assert same_bits(x["pred"][0], y["pred"][0]) and same_bits(x["pred"][1], y["pred"][1]), k
    counts = [o["info"]["count"] for o in a]
    assert max(counts) < CAPACITY and all(c < CAPACITY // 2 for c in counts[2:])
    assert kept[0][0] == kept[0][1] and all(k1 < k0 for k0, k1 in kept[1:])  # the first window drops nothing, every later one does
    plain = turn_walk(hip_auto, None, n_frames=3, images=False)
    assert plain[1]["err"] is None and plain[2]["err"] is not None and "capacity" in plain[2]["err"]
