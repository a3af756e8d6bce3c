"""Pose refinement (include/sf_align.h, staticfusion_amd/align.py) on the GPU. Every system of every iteration is held to
integer equality and every result to bit equality with the restatement of the header in tests/align_ref.py: view sizes around
the wave and workgroup sizes crossed with surfel counts around those of the splat, strides, iteration counts, every flag,
frames with 0 / NaN / inf / negative / too-far depths, a batch against single calls, entries that stop beside one that runs
on, the three forms against one another, the state a refine call must leave alone, every refusal, the twelve displaced
poses of the ranking fixture and the other two libraries."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import align_cases as ac
import align_ref
import score_cases as sc
import test_gpu_view as tv
from conftest import ROOT, hip_runtime
from staticfusion_amd import SfError, SurfelMap, align, keyframes, regions, score, view
from test_gpu_view import TICK, random_surfels, small_solver, uploaded, walk

pytestmark = pytest.mark.gpu

# cols, rows, cx, cy, fx, fy
GEOMS = [(1, 1, 0.5, 0.5, 1.3, 1.1), (1, 65, 0.5, 33.0, 40.0, 40.0), (16, 16, 8.0, 7.5, 20.0, 21.0), (53, 37, 25.25, 19.5, 47.0, -44.0),
         (64, 48, 30.5, 25.0, 61.0, 58.5), (80, 60, 39.5, 29.5, 72.0, 72.0)]
PARAMS = [dict(iterations=3, min_pairs=6, damping=1e-3), dict(iterations=1, stride=2, min_pairs=6, use_b=False, damping=1e-3),
          dict(iterations=10, stride=3, min_pairs=6, damping=1e-2, dist_max=0.3), dict(iterations=3, use_b=False, z_max=3.0, damping=1e-4, min_pairs=6),
          dict(iterations=3, b_min=0.2, min_pairs=6, dist_max=0.05, damping=1e-3), dict(iterations=1, min_pairs=6, use_b=False),
          dict(iterations=10, min_pairs=6, stride=2, damping=1e-3, use_b=False)]
POSE = tv.se3_exp(np.array([0.01, -0.015, 0.02, 0.01, -0.01, 0.02])).astype(np.float32)


@pytest.fixture(scope="module")
def box(hip_auto):
    s = small_solver(hip_auto, 60, 80)
    yield s
    s.close()


def geom_view(g, pose=POSE, **kw):
    cols, rows, cx, cy, fx, fy = g
    kw.setdefault("min_confidence", 0.0)
    return view.View(pose, cx, cy, fx, fy, rows, cols, **kw)


def expect(surf, v, frame, p, tick=TICK, slots=None):
    return align_ref.refine(surf, v, frame[0], frame[1], p, tick=tick, slots=slots)


def same_bits32(a, b):
    """float32 arrays bit for bit (NaNs: a NaN in both at the same place)"""
    a, b = np.ascontiguousarray(a, np.float32).ravel(), np.ascontiguousarray(b, np.float32).ravel()
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def assert_entry(got_res, got_sys, want, where):
    res, systems = want
    if got_sys is not None:
        got = np.ascontiguousarray(got_sys).view(np.int64).reshape(-1, 32)
        assert got.shape == systems.shape, where
        for it in range(systems.shape[0]):
            assert got[it].tolist() == systems[it].tolist(), (where, "system", it)
    for k in ("status", "iterations_done", "n_first", "ss_first", "n_last", "ss_last"):
        assert int(got_res[k]) == res[k], (where, k, int(got_res[k]), res[k])
    assert same_bits32(got_res["pose"], res["pose"]), (where, got_res["pose"], res["pose"])
    assert not np.asarray(got_res["reserved"]).any(), where


# ---- 1. sizes x counts x strides x iterations x flags, frames with every special value ------------------------------------
@pytest.mark.parametrize("n", [0, 1, 65, 513])
def test_sizes_counts_strides_iterations_and_flags(box, n):
    views = [geom_view(g) for g in GEOMS]
    ps = [align.Params(**PARAMS[(q + n) % len(PARAMS)]) for q in range(len(GEOMS))]
    data = [random_surfels(n, geom_view(g, pose=np.eye(4)), seed=n + g[1], ordered=(n % 2 == 1)) for g in GEOMS]
    if n == 1:  # one surfel that fills the view: pairs everywhere
        data = [ac.flat_surfel(0.0, 0.0, 2.0, 8.0)[None] for g in GEOMS]
    maps = [uploaded(box, d) for d in data]
    frames = [ac.special_frame(d, v, seed=100 + q) for q, (d, v) in enumerate(zip(data, views))]
    res, systems = align.refine_images(maps, views, [f[0] for f in frames], [f[1] for f in frames], ps, systems=True)
    plain = align.refine_images(maps, views, [f[0] for f in frames], [f[1] for f in frames], ps)  # NULL systems_out: same results
    assert plain.tobytes() == res.tobytes()
    slots = max(p.iterations for p in ps) + 1
    assert systems.shape == (len(GEOMS), slots)
    pairs = 0
    for q, v in enumerate(views):
        want = expect(data[q], v, frames[q], ps[q], slots=slots)
        assert_entry(res[q], systems[q], want, (n, GEOMS[q]))
        pairs += want[0]["n_first"]
    assert pairs > (1000 if n == 1 else 100) if n in (1, 513) else (n > 0 or pairs == 0)
    for m in maps:
        m.close()


def test_every_flag_stride_and_iteration_count_at_64_by_48(box):
    g = GEOMS[4]
    v = geom_view(g)
    surf = random_surfels(513, geom_view(g, pose=np.eye(4)), seed=9, ordered=True)
    m = uploaded(box, surf)
    frame = ac.special_frame(surf, v, seed=5)
    ps = [align.Params(**kw) for kw in PARAMS]
    n = len(ps)
    res, systems = align.refine_images([m] * n, [v] * n, [frame[0]] * n, [frame[1]] * n, ps, systems=True)
    model = align_ref.model_image(surf, v, TICK)
    for q in range(n):
        want = align_ref.refine(surf, v, frame[0], frame[1], ps[q], tick=TICK, slots=11, model=model)
        assert_entry(res[q], systems[q], want, PARAMS[q])
    assert res["n_first"][5] > res["n_first"][0] > 0  # use_b masks pairs
    # a flag that is clear: its pointer is not read (a NULL array, NULL entries)
    off = align.Params(use_b=False, iterations=1, min_pairs=6)
    a = align.refine_images([m], [v], [frame[0]], None, off)
    b_ = align.refine_images([m], [v], [frame[0]], [None], off)
    assert a.tobytes() == b_.tobytes() == res[5:6].tobytes()
    m.close()


# ---- 2. a batch against single calls; stops; the forms -----------------------------------------------------------------------
def batch_case(s):
    maps, data, views, order = tv.batch_case(s)
    frames = [ac.special_frame(data[o], v, seed=60 + q, tick=TICK + o) for q, (o, v) in enumerate(zip(order, views))]
    frames[3] = frames[0]  # entries 0 and 3 (48 x 64 both) look at the same frame from two poses
    ps = [align.Params(**PARAMS[q]) for q in range(6)]
    return maps, data, views, order, frames, ps


def test_a_batch_equals_single_calls_and_numpy(box):
    maps, data, views, order, frames, ps = batch_case(box)
    ms = [maps[o] for o in order]
    res, systems = align.refine_images(ms, views, [f[0] for f in frames], [f[1] for f in frames], ps, systems=True)
    slots = systems.shape[1]
    assert slots == 11
    for q, o in enumerate(order):
        f = frames[q]
        single, ssys = align.refine_images([ms[q]], [views[q]], [f[0]], [f[1]], [ps[q]], systems=True)
        assert single.tobytes() == res[q:q + 1].tobytes(), q
        k = ps[q].iterations + 1
        assert ssys[0].tobytes() == systems[q, :k].tobytes() and not systems[q, k:].view(np.int64).any(), q  # unused slots are zeros
        assert_entry(res[q], systems[q], expect(data[o], views[q], f, ps[q], tick=maps[o].info()["tick"], slots=slots), q)
    assert res["n_first"][5] == 0 and res["status"][5] == align.FEW_PAIRS and res["n_first"][4] > 0
    # at the C interface: the record of a seventh slot and its systems are left alone
    b = align._bind(box.api)
    n = 6
    col = [[np.ascontiguousarray(f[k].T) for f in frames] for k in range(2)]
    ptrs = [(C.c_void_p * n)(*[a.ctypes.data for a in col[k]]) for k in range(2)]
    raw = np.full(7, -77, align.RESULT_DTYPE)
    rsys = np.full((7, slots), -77, align.SYSTEM_DTYPE)
    mp = (C.c_void_p * n)(*[m.m.value for m in ms])
    assert b.refine_images(box.h, n, mp, (view.SfvView * n)(*views), ptrs[0], ptrs[1], (align.SfaParams * n)(*ps), raw.ctypes.data, rsys.ctypes.data) == 0
    assert raw[:6].tobytes() == res.tobytes() and rsys[:6].tobytes() == systems.tobytes()
    assert raw[6:].tobytes() == np.full(1, -77, align.RESULT_DTYPE).tobytes() and rsys[6].tobytes() == np.full(slots, -77, align.SYSTEM_DTYPE).tobytes()
    # device pointers (plain hipMalloc memory) with room behind both outputs: the same records, the room untouched
    rt = hip_runtime()

    def dev(a):
        p = C.c_void_p()
        assert rt.hipMalloc(C.byref(p), C.c_size_t(max(a.nbytes, 1))) == 0
        assert rt.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
        return p

    dptr = [[dev(a) for a in col[k]] for k in range(2)]
    dres, dsys = dev(np.full(8, -77, align.RESULT_DTYPE)), dev(np.full((8, slots), -77, align.SYSTEM_DTYPE))
    align.refine_images_device(ms, views, [p.value for p in dptr[0]], [p.value for p in dptr[1]], ps, dres.value, dsys.value)
    box.synchronize()
    back, bsys = np.zeros(8, align.RESULT_DTYPE), np.zeros((8, slots), align.SYSTEM_DTYPE)
    assert rt.hipMemcpy(back.ctypes.data_as(C.c_void_p), dres, C.c_size_t(back.nbytes), 2) == 0
    assert rt.hipMemcpy(bsys.ctypes.data_as(C.c_void_p), dsys, C.c_size_t(bsys.nbytes), 2) == 0
    assert back[:6].tobytes() == res.tobytes() and bsys[:6].tobytes() == systems.tobytes()
    assert back[6:].tobytes() == np.full(2, -77, align.RESULT_DTYPE).tobytes() and bsys[6:].tobytes() == np.full((2, slots), -77, align.SYSTEM_DTYPE).tobytes()
    # and without systems
    assert rt.hipMemcpy(dres, np.full(8, -77, align.RESULT_DTYPE).ctypes.data_as(C.c_void_p), C.c_size_t(back.nbytes), 1) == 0
    align.refine_images_device(ms, views, [p.value for p in dptr[0]], [p.value for p in dptr[1]], ps, dres.value, None)
    box.synchronize()
    assert rt.hipMemcpy(back.ctypes.data_as(C.c_void_p), dres, C.c_size_t(back.nbytes), 2) == 0
    assert back[:6].tobytes() == res.tobytes() and back[6:].tobytes() == np.full(2, -77, align.RESULT_DTYPE).tobytes()
    for p in [x for k in dptr for x in k] + [dres, dsys]:
        rt.hipFree(p)
    for m in maps:
        m.close()


def test_stopped_entries_beside_one_that_runs_on(box):
    v = ac.plane_view(16, 16)
    plane = ac.flat_surfel(0.0, 0.0, 2.0, 4.0)[None]
    wall = random_surfels(513, geom_view(GEOMS[4], pose=np.eye(4)), seed=9, ordered=True)
    vw = geom_view(GEOMS[4])
    m_plane, m_wall = uploaded(box, plane), uploaded(box, wall)
    depth = np.full((16, 16), 2.03, np.float32)
    fw = ac.special_frame(wall, vw, seed=5)
    ps = [align.Params(iterations=4, min_pairs=257, use_b=False, damping=1e-3),  # at most 256 pairs: FEW_PAIRS at once
          align.Params(iterations=4, min_pairs=6, use_b=False, damping=0.0),   # a single plane: DEGENERATE at once
          align.Params(iterations=4, min_pairs=6, use_b=False, damping=1e-3),   # the same plane, damped: runs on
          align.Params(iterations=4, min_pairs=6, use_b=False, damping=1e-3)]
    res, systems = align.refine_images([m_plane, m_plane, m_plane, m_wall], [v, v, v, vw], [depth, depth, depth, fw[0]], None, ps, systems=True)
    assert res["status"].tolist() == [align.FEW_PAIRS, align.DEGENERATE, align.OK, align.OK]
    pairs = int(res["n_first"][0])  # (a frame pixel projects onto the border between two drawn pixels: not all 256 need pair)
    assert res["iterations_done"].tolist() == [0, 0, 4, 4] and res["n_first"][:3].tolist() == [pairs] * 3 and 200 < pairs <= 256
    for q, (surf, vv, d) in enumerate([(plane, v, depth)] * 3 + [(wall, vw, fw[0])]):
        assert_entry(res[q], systems[q], align_ref.refine(surf, vv, d, None, ps[q], tick=TICK), q)
    for q in (0, 1):
        assert not systems[q, 1:].view(np.int64).any() and systems[q, 0]["n"] == pairs
        assert res["n_last"][q] == pairs and res["ss_last"][q] == res["ss_first"][q]
        assert same_bits32(res["pose"][q], np.eye(4, dtype=np.float32))  # D before the refused step: T0 itself
    assert systems[2, 4]["n"] > 200 and res["ss_last"][2] < res["ss_first"][2]
    assert abs(float(res["pose"][2][14]) + 0.03) < 1e-4
    m_plane.close()
    m_wall.close()


TORCH_CHILD = r"""
import sys
import numpy as np
import torch  # first, as bench.py does: the process then holds the HIP runtime torch brought
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import staticfusion_amd as sf
from staticfusion_amd import align
import test_gpu_align as t
s = t.small_solver(sf.load(), 60, 80)
maps, data, views, order, frames, ps = t.batch_case(s)
ms = [maps[o] for o in order]
host, hsys = align.refine_images(ms, views, [f[0] for f in frames], [f[1] for f in frames], ps, systems=True)
dev = [[torch.from_numpy(np.ascontiguousarray(f[k].T)).cuda() for f in frames] for k in range(2)]  # column-major, like sf_get_current
res = torch.full((len(views) + 1, 128), 0x55, dtype=torch.uint8, device="cuda")
rsys = torch.full((len(views) + 1, hsys.shape[1], 32), -5, dtype=torch.int64, device="cuda")
torch.cuda.synchronize()
align.refine_images_device(ms, views, [x.data_ptr() for x in dev[0]], [x.data_ptr() for x in dev[1]], ps, res.data_ptr(), rsys.data_ptr())
s.synchronize()
got = res.cpu().numpy()
assert got[:-1].tobytes() == host.tobytes() and (got[-1] == 0x55).all()
gs = rsys.cpu().numpy()
assert gs[:-1].tobytes() == hsys.tobytes() and (gs[-1] == -5).all()
print("torch tensors ok", int(host["n_first"].sum()))
"""


def test_refine_torch_tensors_in_a_fresh_process():
    """sfa_refine_images_device on torch tensors equals the host form (a fresh process with torch imported first, for the
    reason test_gpu_view.py gives)"""
    out = subprocess.run([sys.executable, "-c", TORCH_CHILD, ROOT], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0 and "torch tensors ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert int(out.stdout.split("torch tensors ok")[1].split()[0]) > 1000


# ---- 3. the stream form after a real solve; what a refine call leaves alone ---------------------------------------------------
@pytest.fixture(scope="module")
def walked(hip_auto):
    s, m, out = walk(hip_auto, 5, render_between=False)
    yield s, m, out
    m.close()
    s.close()


def test_stream_form_equals_image_form_and_numpy(walked):
    s, m, out = walked
    v = view.default_view(s, m)
    moved = view.default_view(s, m)
    moved.pose[12] += 0.02
    d, g = s.current(0)
    b = s.b_image(0)
    assert (d > 0).mean() > 0.5 and 0 < (b > 0.5).mean()
    ps = [align.Params(iterations=3), align.Params(iterations=2, use_b=False, stride=2, dist_max=0.1)]
    res, systems = align.refine_streams([m, m], [v, moved], [0, 0], ps, systems=True)
    img, isys = align.refine_images([m, m], [v, moved], [d, d], [b, b], ps, systems=True)
    assert res.tobytes() == img.tobytes() and systems.tobytes() == isys.tobytes()
    surf, tick = m.download(), m.info()["tick"]
    assert_entry(res[0], systems[0], align_ref.refine(surf, v, d, b, ps[0], tick=tick, slots=4), "own pose")
    assert_entry(res[1], systems[1], align_ref.refine(surf, moved, d, b, ps[1], tick=tick, slots=4), "moved")
    assert res["n_first"][0] > 1000 and res["status"].tolist() == [0, 0]


def test_a_refine_call_leaves_everything_else_alone(walked):
    s, m, out = walked
    SurfelMap.predict_frames(s, [0], [m], s.default_model_params())
    v = view.default_view(s, m)
    big = view.View(view.look_at((0.4, 0.2, -0.6), (0.0, 0.0, 2.0)), 150.0, 100.0, 250.0, 250.0, 200, 300, min_confidence=0.0)
    db = keyframes.KeyframeDb(s, 10, n_ferns=64)
    db.add_streams([0], [np.eye(4)], [0])
    view.render([m, m], [v, big])

    def readable():
        i = m.info()
        sc_ = score.score_streams([m], [v], [0])
        summ, reg = regions.label_streams(s, [0])
        return (i["count"], i["tick"], i["pose"].tobytes(), tuple(i["stats"]), m.download().tobytes(), m.index_map().tobytes(),
                s.prediction()[0].tobytes(), s.prediction()[1].tobytes(), s.prediction_dense_stream(0), s.current(0)[0].tobytes(), s.b_image(0).tobytes(),
                sc_.tobytes(), db.query_streams([0]).tobytes(), db.encode_streams([0]).tobytes(), summ.tobytes(), tuple(view.last_large_sprites(s, 2)))

    before = readable()
    res = align.refine_streams([m], [v], [0], align.Params(iterations=2))
    assert res["status"][0] == 0 and res["n_first"][0] > 1000
    assert readable() == before
    # a larger call grows the scratch: a view of 200 x 300 with a frame of its own, twice
    frame = np.full((200, 300), 2.0, np.float32)
    res = align.refine_images([m, m], [big, big], [frame, frame], None, align.Params(iterations=2, use_b=False, min_pairs=6, damping=1e-3))
    assert res[0].tobytes() == res[1].tobytes()
    assert readable() == before
    db.close()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(hip_auto):
    s = small_solver(hip_auto, 30, 40)
    other = small_solver(hip_auto, 30, 40)
    b = align._bind(s.api)
    good = view.View(np.eye(4), 20.0, 15.0, 33.0, 33.0, 30, 40, min_confidence=0.0)
    surf = random_surfels(300, good, seed=1, ordered=True)
    m1, m2, mo = uploaded(s, surf), uploaded(s, surf[:65]), uploaded(other, surf)
    images = ac.special_frame(surf, good, seed=3)
    s.set_current(0, images[0], np.zeros_like(images[0]))
    frame = [np.ascontiguousarray(a.T) for a in images]  # column-major, as the C interface takes them
    rec = np.full(2, -77, align.RESULT_DTYPE)
    rsys = np.full((2, 11), -77, align.SYSTEM_DTYPE)
    r, y = rec.ctypes.data, rsys.ctypes.data
    dp, bp = ((C.c_void_p * 2)(frame[k].ctypes.data, frame[k].ctypes.data) for k in range(2))
    two = (C.c_void_p * 2)(m1.m.value, m2.m.value)
    foreign = (C.c_void_p * 2)(m1.m.value, mo.m.value)
    with_null = (C.c_void_p * 2)(m1.m.value, None)
    vs = (view.SfvView * 2)(good, good)
    ps = (align.SfaParams * 2)(align.Params(), align.Params())
    st = (C.c_int32 * 2)(0, 0)
    nan, inf = float("nan"), float("inf")
    bad_pose = np.eye(4)
    bad_pose[2, 3] = nan
    bad_views = [dict(pose=bad_pose), dict(cx=inf), dict(cy=nan), dict(fx=nan), dict(fy=inf), dict(min_confidence=nan), dict(max_depth=inf),
                 dict(rows=0), dict(rows=4097), dict(cols=0), dict(cols=4097), dict(fx=0.0), dict(fy=0.0), dict(max_depth=0.4), dict(max_depth=-2.0),
                 dict(shade=2), dict(shade=-1)]
    bad_params = [dict(dist_max=nan), dict(z_max=inf), dict(b_min=nan), dict(damping=inf), dict(dist_max=0.0), dict(dist_max=1.5), dict(z_max=0.0),
                  dict(z_max=32.5), dict(damping=-0.1), dict(iterations=0), dict(iterations=65), dict(stride=0), dict(stride=17), dict(min_pairs=5),
                  dict(use_b=2), dict(use_b=-1)]

    def bad_view(**kw):
        base = dict(pose=np.eye(4), cx=20.0, cy=15.0, fx=33.0, fy=33.0, rows=30, cols=40, min_confidence=0.0)
        base.update(kw)
        return (view.SfvView * 2)(good, view.View(**base))

    def bad_param(**kw):
        return (align.SfaParams * 2)(align.Params(), align.Params(**kw))

    big = 65536
    many = ((C.c_void_p * big)(*([m1.m.value] * big)), (view.SfvView * big)(*([good] * big)), (C.c_int32 * big)(), (align.SfaParams * big)(*([align.Params(iterations=1)] * big)),
            (C.c_void_p * big)(*([frame[0].ctypes.data] * big)))
    huge = np.full(big, -77, align.RESULT_DTYPE)
    # -- the stream form
    cases = [(None, 2, two, vs, st, ps, r, y), (s.h, 2, None, vs, st, ps, r, y), (s.h, 2, two, None, st, ps, r, y), (s.h, 2, two, vs, None, ps, r, y),
             (s.h, 2, two, vs, st, None, r, y), (s.h, 2, two, vs, st, ps, None, y), (s.h, -1, two, vs, st, ps, r, y), (s.h, 2, foreign, vs, st, ps, r, y),
             (other.h, 2, two, vs, st, ps, r, y), (s.h, 2, with_null, vs, st, ps, r, y), (s.h, big, many[0], many[1], many[2], many[3], huge.ctypes.data, None),
             (s.h, 2, two, vs, (C.c_int32 * 2)(0, 1), ps, r, y), (s.h, 2, two, vs, (C.c_int32 * 2)(-1, 0), ps, r, y),
             (s.h, 2, two, bad_view(rows=29), st, ps, r, y), (s.h, 2, two, bad_view(cols=41), st, ps, r, y)]
    cases += [(s.h, 2, two, bad_view(**kw), st, ps, r, y) for kw in bad_views]
    cases += [(s.h, 2, two, vs, st, bad_param(**kw), r, y) for kw in bad_params]
    d1 = np.zeros((40, 30), np.float32)
    getter = s.api.get_current(s.h, 1, d1.ctypes.data_as(C.POINTER(C.c_float)), None)  # the getters' own code for a stream out of range
    assert getter != 0
    for q, args in enumerate(cases):
        code = b.refine_streams(*args)
        assert code == (getter if q in (11, 12) else -1), q
        assert s.api.last_error(), q
    assert b.refine_streams(s.h, 0, None, None, None, None, None, None) == 0  # an empty batch is fine
    # -- the image forms
    half = (C.c_void_p * 2)(frame[0].ctypes.data, None)
    for fn in (b.refine_images, b.refine_images_device):
        cases = [(None, 2, two, vs, dp, bp, ps, r, y), (s.h, 2, None, vs, dp, bp, ps, r, y), (s.h, 2, two, None, dp, bp, ps, r, y),
                 (s.h, 2, two, vs, None, bp, ps, r, y), (s.h, 2, two, vs, dp, bp, None, r, y), (s.h, 2, two, vs, dp, bp, ps, None, y),
                 (s.h, -1, two, vs, dp, bp, ps, r, y), (s.h, 2, foreign, vs, dp, bp, ps, r, y), (other.h, 2, two, vs, dp, bp, ps, r, y),
                 (s.h, 2, with_null, vs, dp, bp, ps, r, y), (s.h, big, many[0], many[1], many[4], many[4], many[3], huge.ctypes.data, None),
                 (s.h, 2, two, vs, half, bp, ps, r, y),  # a missing depth image
                 (s.h, 2, two, vs, dp, None, ps, r, y), (s.h, 2, two, vs, dp, half, ps, r, y)]  # use_b without b
        cases += [(s.h, 2, two, bad_view(**kw), dp, bp, ps, r, y) for kw in bad_views]
        cases += [(s.h, 2, two, vs, dp, bp, bad_param(**kw), r, y) for kw in bad_params]
        for q, args in enumerate(cases):
            assert fn(*args) == -1, (fn, q)  # (host addresses in a device call: a refused call never looks at them)
            assert s.api.last_error(), q
        assert fn(s.h, 0, None, None, None, None, None, None, None) == 0
    with pytest.raises(SfError):
        align.refine_streams([m1, mo], [good, good], [0, 0])  # maps of two solvers
    with pytest.raises(SfError):
        align.refine_streams([m1], [good, good], [0])
    with pytest.raises(SfError):
        align.refine_images([m1], [good], [np.zeros((40, 30), np.float32)])  # an image of another shape
    # the handle goes first: the map is an empty shell that fails cleanly
    other.close()
    one = (C.c_void_p * 1)(mo.m.value)
    assert b.refine_streams(s.h, 1, one, vs, st, ps, r, y) == -3 and b.refine_images(s.h, 1, one, vs, dp, bp, ps, r, y) == -3  # SF_ERR_STATE
    # nothing was written
    assert rec.tobytes() == np.full(2, -77, align.RESULT_DTYPE).tobytes() and rsys.tobytes() == np.full((2, 11), -77, align.SYSTEM_DTYPE).tobytes()
    assert huge.tobytes() == np.full(big, -77, align.RESULT_DTYPE).tobytes()
    # and the same arguments, valid, still refine
    off = (align.SfaParams * 2)(align.Params(use_b=False), align.Params(use_b=False))
    assert b.refine_streams(s.h, 2, two, vs, st, off, r, y) == 0
    assert rec["n_first"][0] > rec["n_first"][1] > 0 and (rsys["reserved"] == 0).all()
    for m in (m1, m2, mo):
        m.close()
    s.close()


# ---- 5. convergence --------------------------------------------------------------------------------------------------
def test_twelve_displaced_poses_converge_in_one_call(box):
    depth, surf, views = ac.convergence_case()
    ref = ac.convergence_reference()
    m = uploaded(box, surf, tick=1)
    box.set_current(0, depth, np.zeros_like(depth))
    p = align.Params(iterations=10, dist_max=0.15, stride=1, use_b=False)
    res, systems = align.refine_streams([m] * 12, views, [0] * 12, p, systems=True)  # one call: the same map and stream twelve times
    for q in range(12):
        assert_entry(res[q], systems[q], ref[q], q)
    sp = sc.ranking_params()
    before = score.score_streams([m] * 12, views, [0] * 12, sp)
    after_views = [view.View(align.pose_matrix(res[q]), rows=sc.RANK_ROWS, cols=sc.RANK_COLS, min_confidence=0.0, max_depth=20.0, **sc.RANK_INTRINSICS) for q in range(12)]
    after = score.score_streams([m] * 12, after_views, [0] * 12, sp)
    for q in range(12):
        trans, rot = ac.pose_error(res["pose"][q])
        assert trans < 0.01 and rot < 0.01, (q, trans, rot)  # a fifth of the displacement of 0.05
        assert res["ss_last"][q] < res["ss_first"][q] and res["status"][q] == align.OK and res["iterations_done"][q] == 10
        assert after["n_inlier"][q] >= before["n_inlier"][q], (q, before["n_inlier"][q], after["n_inlier"][q])  # an order, not a threshold
    m.close()


# ---- 6. the other two libraries link the same object ---------------------------------------------------------------------
@pytest.mark.parametrize("lib", ["libsf_hip_precise.so", "libsf_hip_reforder.so"])
def test_the_precise_and_reference_order_libraries_refine_the_same(lib):
    import staticfusion_amd as sf

    api = sf.Api(os.path.join(os.path.dirname(sf.LIB), lib), "sf_")
    s = small_solver(api, 60, 80)
    g = GEOMS[3]
    v = geom_view(g)
    surf = random_surfels(513, geom_view(g, pose=np.eye(4)), seed=21, ordered=False)
    m = uploaded(s, surf)
    frame = ac.special_frame(surf, v, seed=8)
    p = align.Params(iterations=3, min_pairs=6, damping=1e-3)
    res, systems = align.refine_images([m], [v], [frame[0]], [frame[1]], p, systems=True)
    assert_entry(res[0], systems[0], expect(surf, v, frame, p), lib)
    assert res[0]["n_first"] > 100
    m.close()
    s.close()
