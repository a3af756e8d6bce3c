"""Pose scoring (include/sf_score.h, staticfusion_amd/score.py) on the GPU. Every comparison is integer equality with the NumPy
statement of the header in tests/score_ref.py, class images pixel for pixel: view sizes around the wave and workgroup sizes
of the flat pixel index crossed with surfel counts around those of the splat, frames with 0 / NaN / inf / negative / exact-tie
depths, every flag, sums that need 64 bits, a batch against single calls, the three forms against one another, the state a
score call must leave alone, every refusal, a ranking of thirteen poses and a five-frame walk."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import score_cases as sc
import score_ref
import test_gpu_view as tv
import view_ref
from conftest import ROOT, hip_runtime
from staticfusion_amd import SfError, map_window, score, streams, view
from test_gpu_view import TICK, random_surfels, small_solver, uploaded, walk

pytestmark = pytest.mark.gpu

# cols, rows, cx, cy, fx, fy: sizes around the wave (64), the workgroup (256 lanes, 1024 pixels) and the row length
GEOMS = [(1, 1, 0.5, 0.5, 1.3, 1.1), (1, 63, 0.5, 30.0, 40.0, 40.0), (1, 64, 0.5, 31.0, 40.0, 40.0), (1, 65, 0.5, 33.0, 40.0, 40.0),
         (16, 16, 8.0, 7.5, 20.0, 21.0), (257, 1, 128.0, 0.5, 150.0, 150.0), (53, 37, 25.25, 19.5, 47.0, -44.0), (64, 48, 30.5, 25.0, 61.0, 58.5)]
PARAMS = [dict(), dict(use_b=False), dict(use_grey=False), dict(tol_rel=0.0), dict(tol_abs=0.0), dict(tol_abs=0.0, tol_rel=0.0, use_b=False, max_residual=0.05),
          dict(b_min=0.2, max_residual=32.0), dict(use_b=False, use_grey=False, tol_abs=0.1)]
POSE = tv.se3_exp(np.array([0.02, -0.03, 0.05, 0.03, -0.02, 0.05])).astype(np.float32)


@pytest.fixture(scope="module")
def box(hip_auto):
    s = small_solver(hip_auto, 60, 80)
    yield s
    s.close()


def geom_view(g, pose=POSE, **kw):
    cols, rows, cx, cy, fx, fy = g
    kw.setdefault("min_confidence", 0.0)
    return view.View(pose, cx, cy, fx, fy, rows, cols, **kw)


def make_frame(surf, v, seed, tick=TICK):
    """depth, grey and b images for view v: the map's own depth plus noise, and by position 0, NaN, inf, negative and
    exact-tie depths, NaN grey, NaN b and b equal to the default b_min"""
    rng = np.random.default_rng(seed)
    rows, cols = v.rows, v.cols
    zm = view_ref.render(surf, v, tick=tick)["depth"]
    depth = np.where(zm > 0, zm + rng.normal(0, 0.04, zm.shape), rng.uniform(0.5, 4.0, zm.shape)).astype(np.float32)
    flat = np.arange(rows * cols).reshape(rows, cols)
    depth = np.where(flat % 7 == 3, zm, depth)  # an exact tie: r == 0
    for mod, rem, val in ((17, 5, 0.0), (19, 6, np.nan), (23, 7, np.inf), (29, 8, -1.5)):
        depth[flat % mod == rem] = val
    grey = rng.random((rows, cols)).astype(np.float32)
    grey[flat % 31 == 9] = np.nan
    b = rng.random((rows, cols)).astype(np.float32)
    b[flat % 37 == 10] = np.nan
    b[flat % 41 == 11] = 0.5
    return depth, grey, b


def expect(surf, v, frame, p, tick=TICK):
    return score_ref.score(surf, v, frame[0], frame[1], frame[2], p, tick=tick)


def assert_entry(got_rec, got_cls, want, where):
    assert score_ref.as_dict(got_rec) == want[0], (where, score_ref.as_dict(got_rec), want[0])
    if got_cls is not None:
        assert got_cls.dtype == np.uint8 and np.array_equal(got_cls, want[1]), where


# ---- 1. sizes x counts, frames with every special value, every flag, class images --------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 513])
def test_sizes_counts_flags_and_class_images(box, n):
    views = [geom_view(g, shade=(view.SHADE_NORMAL if q % 2 else view.SHADE_COLOUR)) for q, g in enumerate(GEOMS)]
    ps = [score.Params(**PARAMS[(q + n) % len(PARAMS)]) for q in range(len(GEOMS))]
    data = [random_surfels(n, geom_view(g, pose=np.eye(4)), seed=n + g[1], ordered=(n % 2 == 1)) for g in GEOMS]
    maps = [uploaded(box, d) for d in data]
    frames = [make_frame(d, v, seed=100 + q) for q, (d, v) in enumerate(zip(data, views))]
    rec, cls = score.score_images(maps, views, [f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], ps, classes=True)
    plain = score.score_images(maps, views, [f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], ps)  # no class image: same numbers
    assert plain.tobytes() == rec.tobytes()
    total = 0
    for q, v in enumerate(views):
        want = expect(data[q], v, frames[q], ps[q])
        assert_entry(rec[q], cls[q], want, (n, GEOMS[q]))
        assert cls[q].shape == (v.rows, v.cols)
        total += want[0]["n_both"]
    assert total > 0 if n >= 63 else (n > 0 or total == 0)
    for m in maps:
        m.close()


def test_every_flag_at_64_by_48(box):
    g = GEOMS[-1]
    v = geom_view(g)
    surf = random_surfels(513, geom_view(g, pose=np.eye(4)), seed=9, ordered=True)
    m = uploaded(box, surf)
    frame = make_frame(surf, v, seed=5)
    ps = [score.Params(**kw) for kw in PARAMS]
    n = len(ps)
    rec, cls = score.score_images([m] * n, [v] * n, [frame[0]] * n, [frame[1]] * n, [frame[2]] * n, ps, classes=True)
    seen = set()
    for q in range(n):
        want = expect(surf, v, frame, ps[q])
        assert_entry(rec[q], cls[q], want, PARAMS[q])
        seen |= set(np.unique(want[1]).tolist())
    assert seen == set(range(7))  # every class code occurs
    assert rec[0]["n_masked"] > 0 == rec[1]["n_masked"] and rec[0]["sum_grey"] > 0 == rec[2]["sum_grey"]
    assert 0 < rec[5]["n_inlier"] < rec[1]["n_inlier"]  # with both tolerances 0 only the exact ties are inliers
    # a flag that is clear: its pointer is not read (NULL arrays, NULL entries)
    off = score.Params(use_b=False, use_grey=False)
    a = score.score_images([m], [v], [frame[0]], None, None, off)
    b_ = score.score_images([m], [v], [frame[0]], [None], [None], off)
    assert a.tobytes() == b_.tobytes() and score_ref.as_dict(a[0]) == expect(surf, v, frame, off)[0]
    m.close()


# ---- 2. sums that need 64 bits ---------------------------------------------------------------------------------------
def test_sum_of_squares_needs_64_bits(box):
    v = view.View(np.eye(4), 32.0, 24.0, 64.0, 64.0, 48, 64, min_confidence=0.0, max_depth=20.0)
    surf = tv.flat_surfel(0.0, 0.0, 1.0, 4.0, (10, 20, 30))[None]
    m = uploaded(box, surf)
    depth = np.full((48, 64), 100.0, np.float32)
    p = score.Params(max_residual=32.0, use_b=False, use_grey=False)
    rec, cls = score.score_images([m], [v], [depth], None, None, p, classes=True)
    r = score_ref.as_dict(rec[0])
    assert r["n_both"] == 3072 == r["n_behind"] == r["n_map"] and (cls[0] == 5).all()
    assert r["sum_abs"] == 3072 * 2 ** 19 and r["sum_sq"] == 3072 * 2 ** 38
    assert r == score_ref.score(surf, v, depth, None, None, p, tick=TICK)[0]
    d = score.derived(rec)
    assert d["mean_abs"][0] == 32.0 and d["rms"][0] == 32.0 and d["inlier_ratio"][0] == 0.0 and d["overlap"][0] == 1.0
    m.close()


# ---- 3. a batch against single calls; the three forms ------------------------------------------------------------------
def batch_case(s):
    maps, data, views, order = tv.batch_case(s)
    frames = [make_frame(data[o], v, seed=60 + q, tick=TICK + o) for q, (o, v) in enumerate(zip(order, views))]
    frames[3] = frames[0]  # entries 0 and 3 (48 x 64 both) look at the same frame from two poses
    ps = [score.Params(**PARAMS[q]) for q in range(6)]
    return maps, data, views, order, frames, ps


def test_a_batch_equals_single_calls_and_numpy(box):
    maps, data, views, order, frames, ps = batch_case(box)
    ms = [maps[o] for o in order]
    rec, cls = score.score_images(ms, views, [f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], ps, classes=True)
    for q, o in enumerate(order):
        f = frames[q]
        single = score.score_images([ms[q]], [views[q]], [f[0]], [f[1]], [f[2]], [ps[q]], classes=True)
        assert single[0].tobytes() == rec[q:q + 1].tobytes() and np.array_equal(single[1][0], cls[q]), q
        assert_entry(rec[q], cls[q], expect(data[o], views[q], f, ps[q], tick=maps[o].info()["tick"]), q)
    assert rec[5]["n_map"] == 0 and rec[4]["n_both"] > 0
    # at the C interface: the record of a seventh slot is left alone, a NULL class entry is skipped
    b = score._bind(box.api)
    n = 6
    col = [[np.ascontiguousarray(f[k].T) for f in frames] for k in range(3)]
    ptrs = [(C.c_void_p * n)(*[a.ctypes.data for a in col[k]]) for k in range(3)]
    raw = np.full(7, -77, score.SCORE_DTYPE)
    raw["reserved"] = -77
    ci = [np.full((v.cols, v.rows), 99, np.uint8) for v in views]
    cp = (C.c_void_p * n)(*[None if q == 2 else a.ctypes.data for q, a in enumerate(ci)])
    mp = (C.c_void_p * n)(*[m.m.value for m in ms])
    assert b.score_images(box.h, n, mp, (view.SfvView * n)(*views), ptrs[0], ptrs[1], ptrs[2], (score.SfsParams * n)(*ps), raw.ctypes.data, cp) == 0
    for k in score.FIELDS:
        assert np.array_equal(raw[k][:6], rec[k]), k
        assert raw[k][6] == -77
    assert not raw["reserved"][:6].any() and (raw["reserved"][6] == -77).all()  # reserved is written as 0
    for q in range(n):
        assert (ci[q] == 99).all() if q == 2 else np.array_equal(ci[q].T, cls[q]), q
    # device pointers (plain hipMalloc memory): the same records and class images after the handle's stream has drained
    rt = hip_runtime()

    def dev(a):
        p = C.c_void_p()
        assert rt.hipMalloc(C.byref(p), C.c_size_t(max(a.nbytes, 1))) == 0
        assert rt.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
        return p

    dptr = [[dev(a) for a in col[k]] for k in range(3)]
    dcls = [dev(a) for a in ci]
    drec = dev(np.full(7, -77, score.SCORE_DTYPE))
    score.score_images_device(ms, views, [p.value for p in dptr[0]], [p.value for p in dptr[1]], [p.value for p in dptr[2]], ps, drec.value,
                              [None if q == 2 else p.value for q, p in enumerate(dcls)])
    box.synchronize()
    back = np.zeros(7, score.SCORE_DTYPE)
    assert rt.hipMemcpy(back.ctypes.data_as(C.c_void_p), drec, C.c_size_t(back.nbytes), 2) == 0
    assert back[:6].tobytes() == raw[:6].tobytes() and back["n_frame"][6] == -77
    for q in range(n):
        out = np.zeros_like(ci[q])
        assert rt.hipMemcpy(out.ctypes.data_as(C.c_void_p), dcls[q], C.c_size_t(out.nbytes), 2) == 0
        assert np.array_equal(out, ci[q]), q
    for p in [x for k in dptr for x in k] + dcls + [drec]:
        rt.hipFree(p)
    for m in maps:
        m.close()


TORCH_CHILD = r"""
import sys
import numpy as np
import torch  # first, as bench.py does: the process then holds the HIP runtime torch brought
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import staticfusion_amd as sf
from staticfusion_amd import score
import test_gpu_score as t
s = t.small_solver(sf.load(), 60, 80)
maps, data, views, order, frames, ps = t.batch_case(s)
ms = [maps[o] for o in order]
host, hcls = score.score_images(ms, views, [f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], ps, classes=True)
dev = [[torch.from_numpy(np.ascontiguousarray(f[k].T)).cuda() for f in frames] for k in range(3)]  # column-major, like sf_get_current
cls = [torch.full((v.cols, v.rows), 99, dtype=torch.uint8, device="cuda") for v in views]
rec = torch.full((len(views), 12), -5, dtype=torch.int64, device="cuda")
torch.cuda.synchronize()
score.score_images_device(ms, views, [x.data_ptr() for x in dev[0]], [x.data_ptr() for x in dev[1]], [x.data_ptr() for x in dev[2]], ps, rec.data_ptr(),
                          [x.data_ptr() for x in cls])
s.synchronize()
got = rec.cpu().numpy()
for q in range(len(views)):
    assert [int(x) for x in got[q, :10]] == [int(host[q][k]) for k in score.FIELDS], q
    assert not got[q, 10:].any()
    assert np.array_equal(cls[q].cpu().numpy().T, hcls[q]), q
print("torch tensors ok", int(host["n_both"].sum()))
"""


def test_score_torch_tensors_in_a_fresh_process():
    """sfs_score_images_device on torch tensors equals the host form (a fresh process with torch imported first, for the
    reason test_gpu_view.py gives)"""
    out = subprocess.run([sys.executable, "-c", TORCH_CHILD, ROOT], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0 and "torch tensors ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert int(out.stdout.split("torch tensors ok")[1].split()[0]) > 1000


# ---- 4. the stream form after a real solve; end to end ---------------------------------------------------------------------
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
    moved.pose[12] += 0.05
    d, g = s.current(0)
    b = s.b_image(0)
    assert (d > 0).mean() > 0.5 and 0 < (b > 0.5).mean()
    ps = [score.Params(), score.Params(use_b=False, tol_abs=0.01, tol_rel=0.0)]
    rec, cls = score.score_streams([m, m], [v, moved], [0, 0], ps, classes=True)
    img, icls = score.score_images([m, m], [v, moved], [d, d], [g, g], [b, b], ps, classes=True)
    assert rec.tobytes() == img.tobytes() and all(np.array_equal(x, y) for x, y in zip(cls, icls))
    surf, tick = m.download(), m.info()["tick"]
    assert_entry(rec[0], cls[0], score_ref.score(surf, v, d, g, b, ps[0], tick=tick), "own pose")
    assert_entry(rec[1], cls[1], score_ref.score(surf, moved, d, g, b, ps[1], tick=tick), "moved")
    assert rec[0]["n_both"] > 1000 and rec[0]["n_inlier"] > 0


def test_five_frame_walk_scored_at_the_maps_own_pose(walked):
    """a condition on the order, not a threshold: the pose the pipeline arrived at explains the frame better than one 0.3 m
    to the side"""
    s, m, out = walked
    v = view.default_view(s, m)
    aside = view.default_view(s, m)
    aside.pose[12] += 0.3
    rec = score.score_streams([m, m], [v, aside], [0, 0])
    assert rec[0]["n_both"] > 0.5 * rec[0]["n_frame"]
    assert rec[0]["n_inlier"] > rec[1]["n_inlier"]
    d = score.derived(rec)
    assert d["inlier_ratio"][0] > d["inlier_ratio"][1] and 0.5 < d["overlap"][0] <= 1.0


# ---- 5. a score call leaves state alone ------------------------------------------------------------------------------
def test_a_score_call_leaves_the_last_render_alone(box):
    v = tv.large_view(min_confidence=0.0)
    small = random_surfels(300, v, seed=17, ordered=True)
    surf = np.concatenate([small[:150], tv.flat_surfel(0.01, -0.02, 0.45, 2.0, (9, 8, 7))[None], small[150:]])
    m = uploaded(box, surf)
    view.render([m, m], [v, geom_view(GEOMS[4])])
    counts = view.last_large_sprites(box, 2)
    assert counts[0] == 1
    frame = make_frame(surf, v, seed=2)
    rec = score.score_images([m] * 3, [v] * 3, [frame[0]] * 3, [frame[1]] * 3, [frame[2]] * 3)
    assert score_ref.as_dict(rec[2]) == expect(surf, v, frame, score.Params())[0]  # (a large sprite drawn by the score call too)
    assert view.last_large_sprites(box, 2) == counts  # still the render's n and the render's counts
    with pytest.raises(SfError):
        view.last_large_sprites(box, 3)
    m.close()


def test_a_walk_with_score_calls_in_between_equals_the_walk_without(hip_auto, walked, monkeypatch):
    plain = walked[2]
    calls = []

    def score_instead(maps, views, **kw):
        """stands in for view.render inside walk(): the same maps and views, scored in all three ways"""
        s = maps[0].solver
        own = [q for q, v in enumerate(views) if (v.rows, v.cols) == (s.rows, s.cols)]
        r = score.score_streams([maps[q] for q in own], [views[q] for q in own], [0] * len(own), classes=True)[0]
        rng = np.random.default_rng(len(calls))
        fr = [rng.uniform(0.5, 3.0, (v.rows, v.cols)).astype(np.float32) for v in views]
        score.score_images(maps, views, fr, fr, fr, classes=True)
        calls.append(int(r["n_frame"][0]))

    monkeypatch.setattr(tv.view, "render", score_instead)
    s2, m2, scored = walk(hip_auto, 5, render_between=True)
    monkeypatch.undo()
    assert len(calls) == 10 and max(calls) > 1000
    tv.same_walk(plain, scored)  # maps, index images, predictions, trajectories
    # ---- after other companions: straight after a cull (indices have moved) and after the map has followed its stream
    surf = m2.download()
    kept = map_window.cull([m2], [map_window.Filter(min_confidence=0.25)])[0]
    assert 0 < kept < surf.shape[0]
    small = view.View(view.view_pose(view.default_view(s2, m2)), 20.0, 15.0, 33.0, 33.0, 30, 40, min_confidence=0.0)
    after = m2.download()
    frame = make_frame(after, small, seed=4, tick=m2.info()["tick"])
    want = expect(after, small, frame, score.Params(), tick=m2.info()["tick"])
    rec, cls = score.score_images([m2], [small], [frame[0]], [frame[1]], [frame[2]], classes=True)
    assert_entry(rec[0], cls[0], want, "after a cull")
    assert rec[0]["n_both"] > 300
    s3 = small_solver(hip_auto, 60, 80)
    streams.rebind_map(m2, s3)
    rec, cls = score.score_images([m2], [small], [frame[0]], [frame[1]], [frame[2]], classes=True)
    assert_entry(rec[0], cls[0], want, "after a rebind")
    b = score._bind(hip_auto)
    one = np.full(1, -77, score.SCORE_DTYPE)
    dp = (C.c_void_p * 1)(np.ascontiguousarray(frame[0].T).ctypes.data)
    off = score.Params(use_b=False, use_grey=False)
    assert b.score_images(s2.h, 1, (C.c_void_p * 1)(m2.m.value), C.byref(small), dp, None, None, C.byref(off), one.ctypes.data, None) == -1  # the old handle no longer owns it
    assert one["n_frame"][0] == -77
    m2.close()
    s3.close()
    s2.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(hip_auto):
    s = small_solver(hip_auto, 30, 40)
    other = small_solver(hip_auto, 30, 40)
    b = score._bind(s.api)
    good = view.View(np.eye(4), 20.0, 15.0, 33.0, 33.0, 30, 40, min_confidence=0.0)
    surf = random_surfels(300, good, seed=1, ordered=True)
    m1, m2, mo = uploaded(s, surf), uploaded(s, surf[:65]), uploaded(other, surf)
    images = make_frame(surf, good, seed=3)
    s.set_current(0, images[0], images[1])
    frame = [np.ascontiguousarray(a.T) for a in images]  # column-major, as the C interface takes them
    rec = np.full(2, -77, score.SCORE_DTYPE)
    cls = [np.full((40, 30), 99, np.uint8) for _ in range(2)]
    cp = (C.c_void_p * 2)(*[a.ctypes.data for a in cls])
    dp, gp, bp = ((C.c_void_p * 2)(frame[k].ctypes.data, frame[k].ctypes.data) for k in range(3))
    two = (C.c_void_p * 2)(m1.m.value, m2.m.value)
    foreign = (C.c_void_p * 2)(m1.m.value, mo.m.value)
    with_null = (C.c_void_p * 2)(m1.m.value, None)
    vs = (view.SfvView * 2)(good, good)
    ps = (score.SfsParams * 2)(score.Params(), score.Params())
    st = (C.c_int32 * 2)(0, 0)
    nan, inf = float("nan"), float("inf")
    bad_pose = np.eye(4)
    bad_pose[2, 3] = nan
    bad_views = [dict(pose=bad_pose), dict(cx=inf), dict(cy=nan), dict(fx=nan), dict(fy=inf), dict(min_confidence=nan), dict(max_depth=inf),
                 dict(rows=0), dict(rows=4097), dict(cols=0), dict(cols=4097), dict(fx=0.0), dict(fy=0.0), dict(max_depth=0.4), dict(max_depth=-2.0),
                 dict(shade=2), dict(shade=-1)]
    bad_params = [dict(tol_abs=nan), dict(tol_rel=inf), dict(max_residual=nan), dict(b_min=inf), dict(tol_abs=-0.01), dict(tol_rel=-1.0),
                  dict(max_residual=0.0), dict(max_residual=32.5), dict(use_grey=2), dict(use_b=-1)]

    def bad_view(**kw):
        base = dict(pose=np.eye(4), cx=20.0, cy=15.0, fx=33.0, fy=33.0, rows=30, cols=40, min_confidence=0.0)
        base.update(kw)
        return (view.SfvView * 2)(good, view.View(**base))

    def bad_param(**kw):
        return (score.SfsParams * 2)(score.Params(), score.Params(**kw))

    r = rec.ctypes.data
    big = 65536
    many = ((C.c_void_p * big)(*([m1.m.value] * big)), (view.SfvView * big)(*([good] * big)), (C.c_int32 * big)(), (score.SfsParams * big)(*([score.Params()] * big)),
            (C.c_void_p * big)(*([frame[0].ctypes.data] * big)))
    huge = np.full(big, -77, score.SCORE_DTYPE)
    # -- the stream form
    cases = [(None, 2, two, vs, st, ps, r, cp), (s.h, 2, None, vs, st, ps, r, cp), (s.h, 2, two, None, st, ps, r, cp), (s.h, 2, two, vs, None, ps, r, cp),
             (s.h, 2, two, vs, st, None, r, cp), (s.h, 2, two, vs, st, ps, None, cp), (s.h, -1, two, vs, st, ps, r, cp), (s.h, 2, foreign, vs, st, ps, r, cp),
             (other.h, 2, two, vs, st, ps, r, cp), (s.h, 2, with_null, vs, st, ps, r, cp), (s.h, big, many[0], many[1], many[2], many[3], huge.ctypes.data, None),
             (s.h, 2, two, vs, (C.c_int32 * 2)(0, 1), ps, r, cp), (s.h, 2, two, vs, (C.c_int32 * 2)(-1, 0), ps, r, cp),
             (s.h, 2, two, bad_view(rows=29), st, ps, r, cp), (s.h, 2, two, bad_view(cols=41), st, ps, r, cp)]
    cases += [(s.h, 2, two, bad_view(**kw), st, ps, r, cp) for kw in bad_views]
    cases += [(s.h, 2, two, vs, st, bad_param(**kw), r, cp) for kw in bad_params]
    d1 = np.zeros((40, 30), np.float32)
    getter = s.api.get_current(s.h, 1, d1.ctypes.data_as(C.POINTER(C.c_float)), None)  # the getters' own code for a stream out of range
    assert getter != 0
    for q, args in enumerate(cases):
        code = b.score_streams(*args)
        assert code == (getter if q in (11, 12) else -1), q
        assert s.api.last_error(), q
    assert b.score_streams(s.h, 0, None, None, None, None, None, None) == 0  # an empty batch is fine
    # -- the image forms
    half = (C.c_void_p * 2)(frame[0].ctypes.data, None)
    for fn in (b.score_images, b.score_images_device):
        cases = [(None, 2, two, vs, dp, gp, bp, ps, r, cp), (s.h, 2, None, vs, dp, gp, bp, ps, r, cp), (s.h, 2, two, None, dp, gp, bp, ps, r, cp),
                 (s.h, 2, two, vs, None, gp, bp, ps, r, cp), (s.h, 2, two, vs, dp, gp, bp, None, r, cp), (s.h, 2, two, vs, dp, gp, bp, ps, None, cp),
                 (s.h, -1, two, vs, dp, gp, bp, ps, r, cp), (s.h, 2, foreign, vs, dp, gp, bp, ps, r, cp), (other.h, 2, two, vs, dp, gp, bp, ps, r, cp),
                 (s.h, 2, with_null, vs, dp, gp, bp, ps, r, cp), (s.h, big, many[0], many[1], many[4], many[4], many[4], many[3], huge.ctypes.data, None),
                 (s.h, 2, two, vs, half, gp, bp, ps, r, cp),  # a missing depth image
                 (s.h, 2, two, vs, dp, None, bp, ps, r, cp), (s.h, 2, two, vs, dp, half, bp, ps, r, cp),  # use_grey without grey
                 (s.h, 2, two, vs, dp, gp, None, ps, r, cp), (s.h, 2, two, vs, dp, gp, half, ps, r, cp)]  # use_b without b
        cases += [(s.h, 2, two, bad_view(**kw), dp, gp, bp, ps, r, cp) for kw in bad_views]
        cases += [(s.h, 2, two, vs, dp, gp, bp, bad_param(**kw), r, cp) for kw in bad_params]
        for q, args in enumerate(cases):
            assert fn(*args) == -1, (fn, q)  # (host addresses in a device call: a refused call never looks at them)
            assert s.api.last_error(), q
        assert fn(s.h, 0, None, None, None, None, None, None, None, None) == 0
    with pytest.raises(SfError):
        score.score_streams([m1, mo], [good, good], [0, 0])  # maps of two solvers
    with pytest.raises(SfError):
        score.score_streams([m1], [good, good], [0])
    with pytest.raises(SfError):
        score.score_images([m1], [good], [np.zeros((40, 30), np.float32)])  # an image of another shape
    # the handle goes first: the map is an empty shell that fails cleanly
    other.close()
    one = (C.c_void_p * 1)(mo.m.value)
    assert b.score_streams(s.h, 1, one, vs, st, ps, r, cp) == -3 and b.score_images(s.h, 1, one, vs, dp, gp, bp, ps, r, cp) == -3  # SF_ERR_STATE
    # nothing was written
    assert (rec["n_frame"] == -77).all() and (rec["sum_grey"] == -77).all() and (rec["reserved"] == -77).all() and (huge["n_map"] == -77).all()
    assert all((a == 99).all() for a in cls)
    # and the same arguments, valid, still score
    assert b.score_streams(s.h, 2, two, vs, st, ps, r, cp) == 0
    assert rec["n_masked"][0] > 0 and rec["n_map"][0] > rec["n_map"][1] > 0 and not (cls[0] == 99).any()  # (no solve yet: b is 0 everywhere)
    for m in (m1, m2, mo):
        m.close()
    s.close()


# ---- 7. ranking ------------------------------------------------------------------------------------------------------
def test_the_true_pose_ranks_first_of_thirteen(box):
    intr = [sc.RANK_INTRINSICS[k] for k in ("cx", "cy", "fx", "fy")]
    depth, grey, surf, views = sc.ranking_case(*intr)
    ref = sc.ranking_reference(*intr)
    m = uploaded(box, surf, tick=1)
    box.set_current(0, depth, grey)
    p = sc.ranking_params()
    rec = score.score_streams([m] * 13, views, [0] * 13, p)  # one call: the same map and the same stream thirteen times
    for q in range(13):
        assert score_ref.as_dict(rec[q]) == ref[q], q
    assert rec["n_inlier"][0] > rec["n_inlier"][1:].max()
    assert int(np.argmax(score.derived(rec)["inlier_ratio"])) == 0
    m.close()


# ---- 8. the other two libraries link the same object ---------------------------------------------------------------------
@pytest.mark.parametrize("lib", ["libsf_hip_precise.so", "libsf_hip_reforder.so"])
def test_the_precise_and_reference_order_libraries_score_the_same(lib):
    import staticfusion_amd as sf

    api = sf.Api(os.path.join(os.path.dirname(sf.LIB), lib), "sf_")
    s = small_solver(api, 60, 80)
    g = GEOMS[6]
    v = geom_view(g)
    surf = random_surfels(513, geom_view(g, pose=np.eye(4)), seed=21, ordered=False)
    m = uploaded(s, surf)
    frame = make_frame(surf, v, seed=8)
    rec, cls = score.score_images([m], [v], [frame[0]], [frame[1]], [frame[2]], classes=True)
    assert_entry(rec[0], cls[0], expect(surf, v, frame, score.Params()), lib)
    assert rec[0]["n_both"] > 100
    m.close()
    s.close()
