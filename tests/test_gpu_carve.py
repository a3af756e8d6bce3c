"""The carve on the GPU (include/sf_carve.h): sfe_carve_images / sfe_carve_streams against tests/carve_ref.py, np.array_equal and
integer equality on the counts, the packed votes and the maps afterwards. Maps of 0 to 3072 surfels (a partial wave, a whole
block, a block that carves nothing between two that do), views of 1 x 1, 37 x 29 with a negative fy and 64 x 48, 0 / 1 / 2 / 7
entries per map, everything and nothing carved, dry runs, a batch against its single calls, permuted entries, the two frame
forms, what a carve leaves alone, the carver's block at three sizes, every refusal with guard words behind the outputs, the
lifetime of a carver, and the scene of tests/test_carve_reference_cpu.py through the device with the score afterwards."""
import copy
import ctypes as C

import numpy as np
import pytest

import carve_cases as cc
import carve_ref as cr
import score_ref
from conftest import driver_params, make_solver
from staticfusion_amd import SfError, SurfelMap, carve, score, view
from test_carve_reference_cpu import scene
from test_gpu_view import random_surfels, small_solver, uploaded, walk

pytestmark = pytest.mark.gpu

GEOMS = {"1x1": cc.plain_view(rows=1, cols=1, cx=0.0, cy=0.0, fx=0.8, fy=0.8, min_confidence=0.0),
         "37x29": cc.plain_view(rows=29, cols=37, cx=18.2, cy=14.6, fx=30.5, fy=-31.0, min_confidence=0.25, max_age=3),
         "64x48": cc.plain_view(rows=48, cols=64, cx=31.5, cy=23.5, fx=52.8, fy=52.8, min_confidence=0.0)}


@pytest.fixture(scope="module")
def box(hip_auto):
    s = small_solver(hip_auto, 48, 64)
    yield s
    s.close()


@pytest.fixture(scope="module")
def carver(box):
    c = carve.Carver(box)
    yield c
    c.close()


def moved(v, k):
    """the view of entry k: view v pushed a little sideways"""
    T = np.array(v.pose, np.float32).reshape(4, 4).T.copy()
    T[:3, 3] += np.array([0.04 * k, -0.03 * k, 0.01 * k], np.float32)
    w = copy.copy(v)
    w.pose = [float(x) for x in T.T.ravel()]
    return w


def frame(v, k, band=False):
    """a depth frame for entry k: far almost everywhere (the surfels of random_surfels lie at 0.5 .. 4 m), with a block that is
    nearer than they are, scattered pixels at their depths, zeros and a NaN; with `band` a stripe of columns without depth"""
    rng = np.random.default_rng(1000 + k)
    img = np.full((v.rows, v.cols), 5.0 + 0.25 * k, np.float32)
    pick = rng.random(img.shape)
    img[pick < 0.25] = rng.uniform(0.5, 4.0, img.shape).astype(np.float32)[pick < 0.25]
    img[pick < 0.04] = 0.0
    if v.rows > 8:
        r0, c0 = int(rng.integers(0, v.rows - 8)), int(rng.integers(0, v.cols - 8))
        img[r0:r0 + 8, c0:c0 + 8] = 0.45
        img[int(rng.integers(0, v.rows)), int(rng.integers(0, v.cols))] = np.nan
    if band:
        img[:, 17:34] = 0.0
    return img


def call(s, crv, specs, params, entries, votes=True):
    """maps uploaded from specs [(surfels, tick)], one call, the maps downloaded: (counts, votes, surfels after, the maps)"""
    maps = [uploaded(s, surf, tick=tick) for surf, tick in specs]
    got = crv.carve(maps, [cc.as_product(p) for p in params], [(m, cc.as_product_view(v), img) for m, v, img in entries], votes=votes)
    counts, words = got if votes else (got, None)
    return counts, words, [m.download() for m in maps], maps


def check(s, crv, specs, params, entries, where):
    want = cr.carve(specs, params, entries)
    counts, words, after, maps = call(s, crv, specs, params, entries)
    for m, w in enumerate(want):
        assert counts[m] == w["counts"], (where, m, counts[m], w["counts"])
        assert words[m].dtype == np.uint32 and np.array_equal(words[m], w["votes"]), (where, m)
        assert after[m].tobytes() == np.ascontiguousarray(w["out"]).tobytes(), (where, m)  # the partition, byte for byte (NaNs included)
        assert maps[m].info()["count"] == w["out"].shape[0], (where, m)
    for m in maps:
        m.close()
    return want


# ---- 1. against the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 3072])
@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_hip_equals_numpy(box, carver, n, geom):
    v = GEOMS[geom]
    surf = random_surfels(n, v, seed=n + 1, ordered=True)
    seen = []
    for n_entries, p in ((0, cc.params()), (1, cc.params(min_votes=1)), (2, cc.params(min_votes=2, max_support=1)), (7, cc.params(min_votes=3, window=2, min_pixels=9))):
        entries = [(0, moved(v, k), frame(v, k, band=(n == 3072))) for k in range(n_entries)]
        want, = check(box, carver, [(surf, cc.TICK)], [p], entries, (geom, n, n_entries))
        seen.append(want)
    assert seen[0]["counts"]["n_carved"] == 0 and seen[0]["counts"]["n_judged"] == 0
    if n >= 63 and geom != "1x1":
        assert all(0 < w["counts"]["n_carved"] < n for w in seen[1:]), [w["counts"] for w in seen]
        assert seen[3]["counts"]["n_supported"] > 0 and seen[3]["counts"]["n_occluded"] > 0 and (seen[3]["votes"] >> 16).max() > 1
    if n == 3072 and geom == "64x48":
        blocks = seen[1]["carved"].reshape(12, 256).any(1)  # a block that carves nothing between two that do
        assert blocks[:4].all() and not blocks[4:6].any() and blocks[6:].all(), blocks


def test_everything_and_nothing(box, carver):
    v = GEOMS["64x48"]
    surf = random_surfels(700, v, seed=5, ordered=False)
    surf = surf[np.isfinite(surf).all(1) & (surf[:, 2] < 3.5)]
    u, w = surf[:, 0] / surf[:, 2] * v.fx + v.cx, surf[:, 1] / surf[:, 2] * v.fy + v.cy
    surf = surf[(u > 2) & (u < v.cols - 3) & (w > 2) & (w < v.rows - 3)]
    surf[:, 8:11] = (0.0, 0.0, -1.0)
    far, near = np.full((48, 64), 6.0, np.float32), np.full((48, 64), 0.3, np.float32)
    p = cc.params(min_votes=1)
    want, = check(box, carver, [(surf, cc.TICK)], [p], [(0, v, far)], "everything")
    assert want["counts"]["n_carved"] == surf.shape[0] > 300 and want["out"].shape[0] == 0
    want, = check(box, carver, [(surf, cc.TICK)], [p], [(0, v, near)], "nothing")
    assert want["counts"]["n_carved"] == 0 and want["counts"]["n_occluded"] == surf.shape[0]


# ---- 2. maps that are not touched, and what holds after a real carve --------------------------------------------------------------------
def fused_map_that_faces_the_camera(api):
    """predict -> load -> solve -> fuse (the walk of tests/test_gpu_view.py): a map with an index image. The library's own fuse
    stores normals that point AWAY from the camera that saw them (the cross product of data.vert: d > 0 in OBSERVE), so under
    the rule as the header states it every surfel of a fused map is UNSEEN -- asserted here, recorded in DESIGN.md section 34.
    To have a fused map, with its index image, that a carve can change, the normals are turned round (download, negate,
    upload) and the stream's frame is fused once more, which renders the index image again."""
    s, m, _ = walk(api, 2, render_between=False)
    crv = carve.Carver(s)
    v = view.default_view(s, m)
    v.min_confidence = 0.0
    far = np.full((v.rows, v.cols), 7.5, np.float32)
    (c,) = crv.carve([m], carve.Params(min_votes=1), [(0, v, far)])
    assert c["n_in"] > 1000 and c["n_judged"] == 0 and c["n_carved"] == 0 and m.index_map().any()  # as fused: nothing faces the camera
    info, surf = m.info(), m.download()
    surf[:, 8:11] *= -1
    m.upload(surf, info["pose"], info["tick"])
    SurfelMap.fuse_frames(s, [0], [m], list(s.batch_results()[0]), 1.0, s.default_model_params())
    assert m.index_map().any()
    return s, m, crv


def test_dry_runs_and_real_carves_on_a_fused_map(hip_auto):
    s, m, crv = fused_map_that_faces_the_camera(hip_auto)
    v = view.default_view(s, m)
    v.min_confidence = 0.0
    far = np.full((v.rows, v.cols), 7.5, np.float32)
    state = lambda: (repr(m.info()), m.download().tobytes(), m.index_map().tobytes())  # noqa: E731
    before, surf, info = state(), m.download(), m.info()
    plain = cc.plain_view(pose=view.view_pose(v), cx=v.cx, cy=v.cy, fx=v.fx, fy=v.fy, rows=v.rows, cols=v.cols, min_confidence=0.0, max_depth=v.max_depth)
    want = cr.carve_map(surf, info["tick"], cc.params(min_votes=1), [(plain, far)])
    assert 100 < want["counts"]["n_carved"] < surf.shape[0]
    # a dry run, a map without entries, and a carve that finds nothing: not touched at all, the index image still answers
    (c,), (words,) = crv.carve([m], carve.Params(min_votes=1, dry_run=True), [(0, v, far)], votes=True)
    assert c == want["counts"] and np.array_equal(words, want["votes"]) and state() == before
    (c,) = crv.carve([m], carve.Params(min_votes=1), [])
    assert c["n_carved"] == 0 and c["n_judged"] == 0 and c["n_out"] == surf.shape[0] and state() == before
    (c,) = crv.carve([m], carve.Params(min_votes=2), [(0, v, far)])
    assert c["n_carved"] == 0 and c["n_through"] == want["counts"]["n_through"] and state() == before
    # the real one
    (c,) = crv.carve([m], carve.Params(min_votes=1), [(0, v, far)])
    assert c == want["counts"]
    after = m.info()
    assert after["count"] == c["n_out"] and after["tick"] == info["tick"] and after["stats"] == info["stats"] and np.array_equal(after["pose"], info["pose"])
    assert m.download().tobytes() == want["out"].tobytes()
    with pytest.raises(SfError, match="failed with -3"):
        m.index_map()  # surfel indices have moved
    mp = s.default_model_params()
    SurfelMap.predict_frames(s, [0], [m], mp)
    assert s.prediction()[0].shape == (60, 80)
    SurfelMap.fuse_frames(s, [0], [m], list(s.batch_results()[0]), 1.0, mp)
    assert m.info()["tick"] == info["tick"] + 1 and m.info()["count"] > 0 and m.index_map().any() and m.download().shape[0] == m.info()["count"]
    for x in (crv, m):
        x.close()
    s.close()


# ---- 3. batches, orders, forms ----------------------------------------------------------------------------------------------------------
def three_maps():
    v = GEOMS["64x48"]
    specs = [(random_surfels(n, v, seed=40 + n, ordered=True), cc.TICK + k) for k, n in enumerate((300, 65, 1000))]
    params = [cc.params(min_votes=1), cc.params(min_votes=2, max_support=1, dry_run=1), cc.params(min_votes=2, window=3, min_pixels=20)]
    small = GEOMS["37x29"]
    entries = [(2, moved(v, 0), frame(v, 0)), (0, moved(v, 1), frame(v, 1)), (2, moved(small, 2), frame(small, 2)), (1, moved(v, 3), frame(v, 3)),
               (2, moved(v, 4), frame(v, 4)), (1, moved(v, 5), frame(v, 5)), (0, moved(small, 6), frame(small, 6))]
    return specs, params, entries


def test_one_call_with_three_maps_equals_the_three_single_calls(box, carver):
    specs, params, entries = three_maps()
    want = check(box, carver, specs, params, entries, "batch")
    assert want[0]["counts"]["n_carved"] > 0 and want[2]["counts"]["n_carved"] > 0 and want[1]["out"].tobytes() == specs[1][0].tobytes()  # (the dry run)
    for m in range(3):
        mine = [(0, v, img) for k, v, img in entries if k == m]
        counts, words, after, maps = call(box, carver, [specs[m]], [params[m]], mine)
        assert counts[0] == want[m]["counts"] and np.array_equal(words[0], want[m]["votes"]) and after[0].tobytes() == np.ascontiguousarray(want[m]["out"]).tobytes()
        maps[0].close()


def test_permuting_the_entries_changes_nothing(box, carver):
    specs, params, entries = three_maps()
    first = call(box, carver, specs, params, entries)
    for order in ([6, 5, 4, 3, 2, 1, 0], [3, 0, 6, 2, 5, 1, 4]):
        again = call(box, carver, specs, params, [entries[k] for k in order])
        assert again[0] == first[0] and all(np.array_equal(a, b) for a, b in zip(again[1], first[1])) and all(a.tobytes() == b.tobytes() for a, b in zip(again[2], first[2]))
        for m in again[3]:
            m.close()
    for m in first[3]:
        m.close()
    # votes asked for one map only, and for none
    maps = [uploaded(box, surf, tick=tick) for surf, tick in specs]
    b = carver.b
    words = np.full(specs[2][0].shape[0] + 4, 0xABABABAB, np.uint32)
    vp = (C.c_void_p * 3)(None, None, words.ctypes.data)
    n = len(entries)
    counts = (carve.SfeCounts * 3)()
    frames = [np.ascontiguousarray(img.T) for _, _, img in entries]
    args = (carver.c, 3, (C.c_void_p * 3)(*[m.m.value for m in maps]), (carve.SfeParams * 3)(*[cc.as_product(p) for p in params]), n,
            (C.c_int32 * n)(*[k for k, _, _ in entries]), (carve.SfvView * n)(*[cc.as_product_view(v) for _, v, _ in entries]),
            (C.c_void_p * n)(*[f.ctypes.data for f in frames]), counts)
    assert b.carve_images(*args, vp) == 0
    assert np.array_equal(words[:-4], first[1][2]) and (words[-4:] == 0xABABABAB).all() and [c.as_dict() for c in counts] == first[0]
    for m in maps:
        m.close()


def test_the_streams_form_equals_the_images_form(hip_auto):
    p = driver_params(hip_auto)
    p.ctf_levels = 2
    s = make_solver(hip_auto, 48, 64, p, batch=2)
    crv = carve.Carver(s)
    v = GEOMS["64x48"]
    for st in (0, 1):
        d = frame(v, st)
        d[~np.isfinite(d)] = 0.0
        s.set_current(st, d, np.full_like(d, 0.5))
    held = [s.current(st)[0] for st in (0, 1)]  # what sf_get_current returns
    surf = random_surfels(1000, v, seed=3, ordered=True)
    pv = [cc.as_product_view(moved(v, k)) for k in range(3)]
    by_stream = [(0, pv[0], 1), (0, pv[1], 0), (0, pv[2], 1)]
    got = {}
    for form, entries in (("streams", by_stream), ("images", [(m, w, held[st]) for m, w, st in by_stream])):
        m = uploaded(s, surf)
        counts, words = crv.carve([m], carve.Params(min_votes=2), entries, votes=True)
        got[form] = (counts, words[0].tobytes(), m.download().tobytes())
        m.close()
    assert got["streams"] == got["images"] and 0 < got["streams"][0][0]["n_carved"] < 1000
    want = cr.carve_map(surf, 5, cc.params(min_votes=2), [(moved(v, k), held[st]) for k, (_, _, st) in enumerate(by_stream)])
    assert got["streams"][0][0] == want["counts"] and got["streams"][2] == want["out"].tobytes()
    assert all(np.array_equal(s.current(st)[0], held[st]) for st in (0, 1))  # nothing is written into a stream
    with pytest.raises(SfError):
        crv.carve([uploaded(s, surf)], None, [(0, pv[0], 0), (0, pv[1], held[0])])  # streams and images in one call
    crv.close()
    s.close()


# ---- 4. what a carve leaves alone -------------------------------------------------------------------------------------------------------
def test_a_carve_moves_nothing_else(hip_auto):
    s, m, crv = fused_map_that_faces_the_camera(hip_auto)
    SurfelMap.predict_frames(s, [0], [m], s.default_model_params())
    other = uploaded(s, m.download(), pose=m.info()["pose"], tick=m.info()["tick"])
    v = view.default_view(s, m)
    v.min_confidence = 0.0
    orbit = view.View(view.look_at((0.5, -0.3, -0.5), (0.0, 0.0, 2.0)), 50.0, 40.0, 90.0, 90.0, 77, 101, min_confidence=0.0)
    view.render([m, m], [orbit, v])

    def readable():
        i = m.info()
        return (i["count"], i["tick"], i["pose"].tobytes(), tuple(i["stats"]), m.download().tobytes(), m.index_map().tobytes(), s.prediction()[0].tobytes(),
                s.prediction()[1].tobytes(), s.prediction_dense_stream(0), s.current(0)[0].tobytes(), s.current(0)[1].tobytes(),
                tuple(view.last_large_sprites(s, 2)), score.score_streams([m], [v], [0], score.Params(use_b=False)).tobytes())

    before = readable()
    far = np.full((v.rows, v.cols), 7.5, np.float32)
    counts = crv.carve([other, m], [carve.Params(min_votes=1), carve.Params(min_votes=1, dry_run=True)], [(0, v, far), (1, v, far)])
    assert counts[0]["n_carved"] > 100 and counts[1]["n_carved"] > 100 and other.info()["count"] == counts[0]["n_out"]
    assert readable() == before  # the streams, the untouched map with its index image, the predictions, the view scratch, a score
    crv.carve([other], carve.Params(min_votes=1), [(0, v, 0)])  # the streams form reads the stream where it lies
    assert readable() == before
    for x in (crv, other, m):
        x.close()
    s.close()


def test_the_carvers_block_reused_small_large_small(box, hip_auto):
    """as tests/test_gpu_call_blocks.py: a small call, one large enough to grow the block and move every offset, the small one again"""
    v = GEOMS["64x48"]
    small = ([(random_surfels(65, v, seed=8, ordered=True), cc.TICK)], [cc.params(min_votes=1)], [(0, v, frame(v, 0))])

    def run(s, crv, size):
        specs, params, entries = small if size == "small" else three_maps()
        counts, words, after, maps = call(s, crv, specs, params, entries)
        for m in maps:
            m.close()
        return repr(counts).encode() + b"".join(w.tobytes() for w in words) + b"".join(a.tobytes() for a in after)

    fresh = small_solver(hip_auto, 48, 64)
    used_c, fresh_c = carve.Carver(box), carve.Carver(fresh)
    first = run(box, used_c, "small")
    large = run(box, used_c, "large")
    third = run(box, used_c, "small")
    assert len(large) > 3 * len(first) and third == first
    assert run(fresh, fresh_c, "small") == first and run(fresh, fresh_c, "large") == large
    used_c.close()
    fresh_c.close()
    fresh.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(box, carver, hip_auto):
    v = GEOMS["64x48"]
    surf = random_surfels(300, v, seed=2, ordered=True)
    other = small_solver(hip_auto, 48, 64)
    m1, m2, foreign_map = uploaded(box, surf), uploaded(box, surf[:65]), uploaded(other, surf[:50])
    foreign_carver = carve.Carver(other)
    b = carver.b
    state = lambda: tuple((repr(m.info()), m.download().tobytes()) for m in (m1, m2, foreign_map))  # noqa: E731
    before = state()
    counts = (carve.SfeCounts * 3)()  # (one more than any call fills: a guard)
    C.memset(counts, 0xFB, C.sizeof(counts))
    sentinel = bytes(counts)
    words = [np.full(300 + 4, 0xABABABAB, np.uint32), np.full(65 + 4, 0xABABABAB, np.uint32)]
    guard = [w.tobytes() for w in words]
    vp = (C.c_void_p * 2)(*[w.ctypes.data for w in words])
    img = np.ascontiguousarray(frame(v, 0).T)
    two = lambda x, y: (C.c_void_p * 2)(x, y)  # noqa: E731
    maps, pr = two(m1.m.value, m2.m.value), (carve.SfeParams * 2)(carve.Params(min_votes=1), carve.Params(min_votes=1))
    map_of, views, frames, streams = (C.c_int32 * 2)(0, 1), (carve.SfvView * 2)(cc.as_product_view(v), cc.as_product_view(v)), two(img.ctypes.data, img.ctypes.data), (C.c_int32 * 2)(0, 0)

    def refused(code, crv=carver.c, n_maps=2, a_maps=maps, a_pr=pr, n=2, a_map_of=map_of, a_views=views, a_frames=frames, a_streams=streams, a_counts=counts,
                forms=("images", "streams")):
        for form in forms:
            fn, fr = (b.carve_images, a_frames) if form == "images" else (b.carve_streams, a_streams)
            assert fn(crv, n_maps, a_maps, a_pr, n, a_map_of, a_views, fr, a_counts, vp) == code, form
            assert box.api.last_error()
            assert bytes(counts) == sentinel and [w.tobytes() for w in words] == guard and state() == before

    refused(-1, crv=None)                                                # a null carver
    refused(-1, n_maps=-1)
    refused(-1, n=-1)
    refused(-1, n=65536, a_map_of=(C.c_int32 * 65536)(), a_views=None)   # (the bound comes before the null check)
    refused(-1, n_maps=65536)
    refused(-1, a_maps=None)                                             # null arguments
    refused(-1, a_pr=None)
    refused(-1, a_counts=None)
    refused(-1, a_map_of=None)
    refused(-1, a_views=None)
    refused(-1, a_frames=None, forms=("images",))
    refused(-1, a_streams=None, forms=("streams",))
    refused(-1, a_maps=two(m1.m.value, None))                            # a null map
    refused(-1, a_map_of=(C.c_int32 * 2)(0, 2))                          # map_of out of range
    refused(-1, a_map_of=(C.c_int32 * 2)(-1, 1))
    refused(-1, n_maps=0)                                                # entries and no map: every map_of is out of range
    refused(-1, a_maps=two(m1.m.value, m1.m.value))                      # the same map twice
    refused(-1, a_maps=two(m1.m.value, foreign_map.m.value))             # a map of another handle than the carver's
    refused(-1, crv=foreign_carver.c)                                    # ... and the carver of another handle than the maps'
    for field, value in (("fx", 0.0), ("rows", 0), ("cols", 4097), ("max_depth", 0.4), ("shade", 7), ("cx", float("nan"))):  # views sfv_check_view refuses
        bad = (carve.SfvView * 2)(cc.as_product_view(v), cc.as_product_view(v))
        setattr(bad[1], field, value)
        refused(-1, a_views=bad)
    bad = (carve.SfvView * 2)(cc.as_product_view(v), cc.as_product_view(GEOMS["37x29"]))
    refused(-1, a_views=bad, forms=("streams",))                         # a view that is not the handle's size
    refused(-1, a_streams=(C.c_int32 * 2)(0, 1), forms=("streams",))     # a stream index out of range (the handle has one stream)
    refused(-1, a_streams=(C.c_int32 * 2)(-1, 0), forms=("streams",))
    refused(-1, a_frames=two(img.ctypes.data, None), forms=("images",))  # a null depth image
    nan, inf = float("nan"), float("inf")
    bad_params = [dict(tol_abs=nan), dict(tol_rel=inf), dict(z_max=nan), dict(min_cos=nan), dict(tol_abs=-1.0), dict(tol_rel=-1.0), dict(z_max=0.0), dict(z_max=32.5),
                  dict(min_cos=-0.1), dict(min_cos=1.5), dict(window=-1), dict(window=4), dict(min_pixels=0), dict(min_pixels=10), dict(min_votes=0), dict(min_votes=65536),
                  dict(max_support=-1), dict(max_support=65536), dict(dry_run=2)]
    for kw in bad_params:
        refused(-1, a_pr=(carve.SfeParams * 2)(carve.Params(min_votes=1), carve.Params(**kw)))  # ... in a later map
    assert b.carve_images(carver.c, 0, None, None, 0, None, None, None, None, None) == 0 and bytes(counts) == sentinel  # nothing at all: SF_OK
    # maps and no entries: SF_OK, the counts say that nothing was judged; map_of, views and the frames may be null
    assert b.carve_streams(carver.c, 2, maps, pr, 0, None, None, None, counts, vp) == 0
    assert [counts[k].as_dict() for k in (0, 1)] == [dict(n_in=k, n_judged=0, n_through=0, n_supported=0, n_occluded=0, n_carved=0, n_out=k) for k in (300, 65)]
    assert bytes(counts)[64:] == sentinel[64:] and not words[0][:300].any() and not words[1][:65].any() and (words[0][300:] == 0xABABABAB).all() and state() == before
    # and the call still works
    C.memset(counts, 0xFB, C.sizeof(counts))
    assert b.carve_images(carver.c, 2, maps, pr, 2, map_of, views, frames, counts, vp) == 0
    want = cr.carve([(surf, 5), (surf[:65], 5)], [cc.params(min_votes=1)] * 2, [(0, v, frame(v, 0)), (1, v, frame(v, 0))])
    assert [counts[k].as_dict() for k in (0, 1)] == [w["counts"] for w in want] and bytes(counts)[64:] == sentinel[64:] and counts[0].reserved == 0
    assert np.array_equal(words[0][:300], want[0]["votes"]) and (words[0][300:] == 0xABABABAB).all() and (words[1][65:] == 0xABABABAB).all()
    for x in (m1, m2, foreign_map, foreign_carver):
        x.close()
    other.close()


def test_the_lifetime_of_a_carver(hip_auto):
    v = GEOMS["64x48"]
    surf = random_surfels(300, v, seed=2, ordered=True)
    s = small_solver(hip_auto, 48, 64)
    crv, m = carve.Carver(s), uploaded(s, surf)
    args = ([m], carve.Params(min_votes=1, dry_run=True), [(0, cc.as_product_view(v), frame(v, 0))])
    first = crv.carve(*args)
    assert first[0]["n_carved"] > 0
    gone = C.c_void_p(s.h.value)
    s.close()  # the handle goes first: the carver is a shell
    with pytest.raises(SfError, match="failed with -3"):
        crv.carve(*args)
    out_c = C.c_void_p()
    assert crv.b.carver_create(gone, C.byref(out_c)) == -3 and crv.b.carver_create(None, C.byref(out_c)) == -1
    crv.close()  # (frees the shell)
    crv.close()
    m.close()
    alive, dead = small_solver(hip_auto, 48, 64), small_solver(hip_auto, 48, 64)  # a live carver handed a map whose handle is gone: SF_ERR_STATE too
    crv2, orphan = carve.Carver(alive), uploaded(dead, surf)
    dead.close()
    counts = (carve.SfeCounts * 1)()
    assert crv2.b.carve_images(crv2.c, 1, (C.c_void_p * 1)(orphan.m.value), C.byref(carve.Params()), 0, None, None, None, counts, None) == -3
    # the carver goes first: clean, and the handle goes on working with another one
    m2 = uploaded(alive, surf)
    assert crv2.carve([m2], args[1], args[2]) == first
    crv2.close()
    crv3 = carve.Carver(alive)
    assert crv3.carve([m2], args[1], args[2]) == first
    for x in (orphan, m2, crv3):
        x.close()
    alive.close()


# ---- 6. the scene -----------------------------------------------------------------------------------------------------------------------
def test_the_box_that_was_carried_away(box, carver):
    sc = scene()
    kind, views = sc["kind"], sc["views"]
    entries = [(0, views[k], sc["gone"][k]) for k in "ABE"]
    want, = check(box, carver, [(sc["surf"], cc.TICK)], [cc.params()], entries, "box gone")
    assert want["counts"]["n_carved"] == 208 and np.array_equal(want["carved"], kind == 2)
    want, = check(box, carver, [(sc["surf"], cc.TICK)], [cc.params()], [(0, views[k], sc["present"][k]) for k in "ABE"], "box present")
    assert want["counts"]["n_carved"] == 0
    # the score of a box-gone frame against the map before and after: the frame no longer sees through the map
    m = uploaded(box, sc["surf"], tick=cc.TICK)
    vb, sp = cc.as_product_view(views["B"]), score.Params(use_grey=False, use_b=False)
    behind = [int(score.score_images([m], [vb], [sc["gone"]["B"]], params=sp)["n_behind"][0])]
    counts = carver.carve([m], carve.Params(), [(0, cc.as_product_view(v), img) for _, v, img in entries])
    assert counts[0]["n_carved"] == 208
    behind.append(int(score.score_images([m], [vb], [sc["gone"]["B"]], params=sp)["n_behind"][0]))
    ref = [score_ref.score(surf, vb, sc["gone"]["B"], params=sp, tick=cc.TICK)[0]["n_behind"] for surf in (sc["surf"], sc["surf"][kind != 2])]
    assert behind == ref and behind[0] - behind[1] > 200, (behind, ref)  # the 26 x 8 pixels of the face, seen from B
    m.close()
