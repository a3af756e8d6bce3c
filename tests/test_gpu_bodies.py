"""Region motion (include/sf_bodies.h, staticfusion_amd/bodies.py) on the GPU. Every comparison is integer or bit equality
with the NumPy statement of the header in tests/body_ref.py: every system of every iteration of every region, every motion
record with its D and W, for the frame pairs of tests/body_cases.py at image sizes below, at and past the tile of the linearise
kernel; region counts on both sides of the LDS budget of its workgroup table; labels that belong to no region; pairs; regions
that stop beside regions that run on; batches; depths and gates at their edges; both forms; every refusal; the state a call must
leave alone; a destroyed handle; and the other two libraries. No tolerance appears anywhere and nothing here asserts a time."""
import ctypes as C
import os

import numpy as np
import pytest

import body_cases as bc
import body_ref as br
import track_cases as tc
from conftest import hip_runtime
from staticfusion_amd import SfError, align, bodies, join, keyframes, regions, score, tracks, view
from test_gpu_regions import sphere_walk
from test_gpu_view import small_solver

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 2), (3, 3), (5, 7), (37, 53), (65, 33), (60, 80), (130, 66)]
SENT = -77
LOOSE = dict(min_pairs=6, iterations=4)  # small images hold few pairs: let their regions take steps


@pytest.fixture(scope="module")
def box(hip_auto):
    s = small_solver(hip_auto, 60, 80)
    yield s
    s.close()


def to_cam(c):
    return tracks.Camera(c["pose"], c["cx"], c["cy"], c["fx"], c["fy"])


def to_p(p):
    return bodies.Params(**p)


def entry(pair, K, pairs=None, **kw):
    z0, l0, z1, l1, c0, c1 = pair
    return dict(z0=z0, l0=l0, z1=z1, l1=l1, c0=c0, c1=c1, K=K, pairs=pairs, p=br.params(**kw))


def call(box, entries, M, systems=True):
    pr = None
    if any(e["pairs"] is not None for e in entries):
        pr = np.array([np.zeros(M, np.int32) if e["pairs"] is None else np.asarray(e["pairs"], np.int32) for e in entries])
    l1 = [e["l1"] for e in entries]
    return bodies.estimate_images(box, [e["z0"] for e in entries], [e["l0"] for e in entries], [e["z1"] for e in entries], None if all(x is None for x in l1) else l1,
                                  [to_cam(e["c0"]) for e in entries], [to_cam(e["c1"]) for e in entries], [e["K"] for e in entries], pr,
                                  [to_p(e["p"]) for e in entries], M, systems=systems)


def reference(entries, M):
    slots = max(int(e["p"]["iterations"]) for e in entries) + 1
    return [br.estimate(e["z0"], e["l0"], e["z1"], e["l1"], e["c0"], e["c1"], e["K"], e["pairs"], e["p"], M, slots) for e in entries]


def same(box, entries, M, what=""):
    """the call against the restatement: motions and systems byte for byte; the restatement's results"""
    got, systems = call(box, entries, M)
    ref = reference(entries, M)
    for q, (mot, sysm) in enumerate(ref):
        assert systems[q].tobytes() == sysm.tobytes(), (what, q, np.argwhere(systems[q].view(np.int64).reshape(sysm.shape) != sysm)[:4])
        assert got[q].tobytes() == mot.tobytes(), (what, q, got[q], mot)
    return ref


# ---- 1. sizes x scenes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_every_scene_equals_numpy(box, rows, cols):
    still = bc.pyramid_pair(rows, cols)
    moving = bc.pyramid_pair(rows, cols, *bc.MOVING_CAMERA)
    two = bc.with_wall_patch(rows, cols, moving)
    plane = bc.plane_pair(rows, cols)
    ref = same(box, [entry(still, 1, **LOOSE), entry(moving, 1, **LOOSE), entry(two, 2, **LOOSE), entry(two, 2, pairs=[1, 2, 0], **LOOSE),
                     entry(plane, 1, damping=1e-3, **LOOSE)], 3, (rows, cols))
    inner = max(rows - 2, 0) * max(cols - 2, 0)
    assert int(br.model(plane[2], plane[3], plane[5], br.params())["has"].sum()) == inner  # none below 3 x 3, one at 3 x 3
    assert 0 < int(ref[4][0][0]["n_first"]) <= inner if inner else int(ref[4][0][0]["n_first"]) == 0
    if rows < 3 or cols < 3:  # no interior: no normals, every region stops at once
        for mot, sysm in ref:
            assert all(int(r["status"]) == br.FEW_PAIRS and int(r["n_first"]) == 0 for r in mot[:1]) and not sysm.any()
    if rows >= 37:
        assert int(ref[0][0][0]["status"]) == br.OK and int(ref[0][0][0]["iterations_done"]) == 4
        assert int(ref[2][0][1]["n_first"]) > 0 and int(ref[2][0][0]["n_first"]) > 0
        assert ref[2][0][2].tobytes() == bytes(192)  # the slot above K


def test_qvga_once(box):
    pair = bc.with_wall_patch(240, 320, bc.pyramid_pair(240, 320, *bc.MOVING_CAMERA))
    ref = same(box, [entry(pair, 2, iterations=3)], 2, "qvga")
    r = ref[0][0][0]
    assert int(r["status"]) == br.OK and int(r["n_first"]) > 10000 and int(r["ss_last"]) * 25 * int(r["n_first"]) <= int(r["ss_first"]) * int(r["n_last"])


# ---- 2. region counts: the workgroup table, its budget exactly, one past it, the global path ----------------------------------
@pytest.mark.parametrize("K", [0, 1, 2, 64, 65, 256])
def test_region_counts_on_both_sides_of_the_lds_budget(box, K):
    """L0 = 1 + index % K along memory: every lane of a wave holds another label (K >= 64), so every trip of the reduction by
    region retires one lane"""
    rows, cols = 65, 33
    z0, _, z1, l1, c0, c1 = bc.pyramid_pair(rows, cols, *bc.MOVING_CAMERA)
    idx = np.arange(rows * cols).reshape(cols, rows).T  # v + u * rows
    l0 = (1 + idx % K).astype(np.int32) if K else np.zeros((rows, cols), np.int32)
    ref = same(box, [entry((z0, l0, z1, l1, c0, c1), K, damping=1e-3, min_pairs=6, iterations=2)], max(K, 1), K)
    if K:
        assert sum(int(r["n_first"]) for r in ref[0][0]) > rows * cols // 2
    if K == 2:
        assert all(int(r["iterations_done"]) == 2 for r in ref[0][0])


# ---- 3. labels and pairs -----------------------------------------------------------------------------------------------------
def test_labels_outside_the_regions_and_pairs(box):
    rows, cols = 37, 53
    z0, l0, z1, l1, c0, c1 = bc.with_wall_patch(rows, cols, bc.pyramid_pair(rows, cols))
    odd = l0.copy()
    odd[5:9, 44:52] = np.array([0, -1, 3, 2 ** 30], np.int32)[:, None]  # none of them is a region of K = 2; on wall pixels of no region
    odd[20, 2:6] = -2 ** 31
    base = entry((z0, l0, z1, l1, c0, c1), 2, **LOOSE)
    noisy = entry((z0, odd, z1, l1, c0, c1), 2, **LOOSE)
    ref = same(box, [base, noisy], 4, "labels")
    assert ref[0][1].tobytes() == ref[1][1].tobytes() and ref[0][0].tobytes() == ref[1][0].tobytes()
    # pairs: off, on, onto the other label, onto a label frame 1 does not have; frame-1 labels absent altogether
    cases = [entry((z0, l0, z1, l1, c0, c1), 2, pairs=p, **LOOSE) for p in ([0, 0, 0, 0], [1, 2, 0, 0], [2, 1, 0, 0], [1, 9, 0, 0], [0, 2, 7, 7])]
    cases.append(entry((z0, l0, z1, None, c0, c1), 2, pairs=[0, 0, 5, 0], **LOOSE))  # (a pair above K is not used: no L1 needed)
    ref = same(box, cases, 4, "pairs")
    n = [[int(r["n_first"]) for r in mot[:2]] for mot, _ in ref]
    assert n[0][0] >= n[1][0] > 0 and n[1][1] > 0 and n[2][0] < n[1][0]  # a pair only takes targets away
    assert n[3][1] == 0 and int(ref[3][0][1]["status"]) == br.FEW_PAIRS and n[3][0] == n[1][0]
    assert n[4] == [n[0][0], n[1][1]] and n[5] == n[0]


# ---- 4. regions that stop ----------------------------------------------------------------------------------------------------
def test_regions_stop_independently(box):
    rows, cols = 60, 80
    z0, l0, z1, l1, c0, c1 = bc.with_wall_patch(rows, cols, bc.pyramid_pair(rows, cols))
    l0 = l0.copy()
    l0[50:52, 60:62] = 3  # four pixels: fewer than min_pairs at iteration 0
    e = entry((z0, l0, z1, l1, c0, c1), 3, iterations=5, min_pairs=16)  # damping 0: the fronto-parallel wall patch is degenerate
    short = entry((z0, l0, z1, l1, c0, c1), 3, iterations=1, min_pairs=16)
    mid = entry((z0, l0, z1, l1, c0, c1), 2, iterations=3, min_pairs=16, damping=1e-4)
    ref = same(box, [e, short, mid], 3, "stops")
    mot = ref[0][0]
    assert [int(r["status"]) for r in mot] == [br.OK, br.DEGENERATE, br.FEW_PAIRS] and [int(r["iterations_done"]) for r in mot] == [5, 0, 0]
    assert int(mot[2]["n_first"]) == int(mot[2]["n_last"]) == 4 and int(mot[1]["n_first"]) == int(mot[1]["n_last"]) > 100
    assert not ref[0][1][1:, 1:].any() and ref[0][1][0, 5].any()  # the stopped regions have one system, the runner six
    assert [int(r["iterations_done"]) for r in ref[1][0]] == [1, 0, 0] and not ref[1][1][0, 2:].any()
    assert [int(r["status"]) for r in ref[2][0][:2]] == [br.OK, br.OK] and int(ref[2][0][1]["iterations_done"]) == 3  # damped: the wall patch runs


# ---- 5. batches --------------------------------------------------------------------------------------------------------------
def test_a_batch_equals_single_calls(box):
    rows, cols = 65, 33
    still = bc.pyramid_pair(rows, cols)
    moving = bc.with_wall_patch(rows, cols, bc.pyramid_pair(rows, cols, *bc.MOVING_CAMERA))
    entries = [entry(still, 1, iterations=2, min_pairs=6), entry(moving, 2, iterations=5, min_pairs=6), entry(moving, 0), entry(moving, 2, iterations=5, min_pairs=6),
               entry(still, 1, iterations=1, min_pairs=6, dist_max=0.02), entry(moving, 2, pairs=[1, 2, 0], iterations=3, min_pairs=6, damping=1e-3)]
    ref = same(box, entries, 3, "batch")
    got, systems = call(box, entries, 3)
    for q, e in enumerate(entries):
        one, sys1 = call(box, [e], 3)
        its = int(e["p"]["iterations"])
        assert one[0].tobytes() == got[q].tobytes() and sys1[0].tobytes() == systems[q][:, :its + 1].tobytes() and not systems[q][:, its + 1:].view(np.int64).any(), q
    assert got[1].tobytes() == got[3].tobytes() and systems[1].tobytes() == systems[3].tobytes()  # the same pair twice
    assert got[2].tobytes() == bytes(3 * 192)
    without = call(box, entries, 3, systems=False)  # systems_out NULL: one record per region slot is reused
    assert without.tobytes() == got.tobytes()
    assert ref[1][0][0]["iterations_done"] == 5


# ---- 6. depths and gates at their edges ----------------------------------------------------------------------------------------
def test_depths_that_do_not_count(box):
    rows, cols = 37, 53
    z0, l0, z1, l1, c0, c1 = bc.pyramid_pair(rows, cols, *bc.MOVING_CAMERA)
    v, u = np.nonzero(l0 == 1)
    bad = [0.0, -1.0, np.nan, np.inf, -np.inf, 4.0001]
    a0, a1 = z0.copy(), z1.copy()
    for k, val in enumerate(bad):
        a0[v[10 + 7 * k], u[10 + 7 * k]] = val
        a1[v[60 + 9 * k], u[60 + 9 * k]] = val
    kw = dict(z_max=4.0, **LOOSE)
    ref = same(box, [entry((z0, l0, z1, l1, c0, c1), 1, **kw), entry((a0, l0, z1, l1, c0, c1), 1, **kw), entry((z0, l0, a1, l1, c0, c1), 1, **kw),
                     entry((a0, l0, a1, l1, c0, c1), 1, z_max=1.4, **LOOSE)], 1, "depths")
    n = [int(m[0]["n_first"]) for m, _ in ref]
    assert n[0] - len(bad) <= n[1] < n[0] and n[2] < n[0] - len(bad) and 0 < n[3] < n[2]  # a bad target depth takes its neighbours' normals too


def test_normal_dz_met_exactly_and_one_ulp_beyond(box):
    rows, cols = 5, 7
    c = bc.cam(rows, cols)
    z1 = np.full((rows, cols), 2.0, np.float32)
    z1[2, 2] = 2.25  # its neighbours see a step of exactly normal_dz
    z1[2, 5] = np.nextafter(np.float32(2.25), np.float32(3))  # one ulp more
    p = br.params(normal_dz=0.25, min_pairs=6, iterations=2)
    has = br.model(z1, None, c, p)["has"]
    assert has[2, 2] and has[1, 2] and has[2, 1] and has[2, 3] and not has[2, 5] and not has[1, 5] and not has[2, 4] and has[1, 1]
    z0 = np.full((rows, cols), 2.0, np.float32)
    l0 = np.ones((rows, cols), np.int32)
    e = dict(z0=z0, l0=l0, z1=z1, l1=None, c0=c, c1=c, K=1, pairs=None, p=p)
    wider = br.params(normal_dz=0.2500003, min_pairs=6, iterations=2)  # the next float32 above the larger step
    assert br.model(z1, None, c, wider)["has"][1:4, 1:6].all()
    ref = same(box, [e, dict(e, p=wider)], 1, "normal_dz")
    assert int(ref[0][0][0]["n_first"]) < int(ref[1][0][0]["n_first"])


def test_warps_that_leave_the_image_or_land_behind_the_camera(box):
    rows, cols = 37, 53
    away = bc.pyramid_pair(rows, cols, None, bc.pose((0.0, 1.2, 0.0)))
    behind = bc.pyramid_pair(rows, cols, None, bc.pose((0.0, np.pi, 0.0)))
    ref = same(box, [entry(away, 1, **LOOSE), entry(behind, 1, **LOOSE)], 2, "warps")
    for mot, sysm in ref:
        assert int(mot[0]["status"]) == br.FEW_PAIRS and int(mot[0]["n_first"]) == 0 and not sysm.any()
        assert np.isfinite(mot[0]["w"]).all() and np.abs(mot[0]["w"].reshape(4, 4).T - np.eye(4)).max() < 1e-6  # D0: it did not move in the room


# ---- 7. the two forms ----------------------------------------------------------------------------------------------------------
def test_host_form_equals_device_form(box):
    rows, cols, m = 60, 80, 3
    pair = bc.with_wall_patch(rows, cols, bc.pyramid_pair(rows, cols, *bc.MOVING_CAMERA))
    entries = [entry(pair, 2, iterations=3, damping=1e-4), entry(bc.pyramid_pair(rows, cols), 1, iterations=2, pairs=[1, 0, 0])]
    got, systems = call(box, entries, m)
    rt = hip_runtime()
    blocks = []

    def dev(a):
        p = C.c_void_p()
        assert rt.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
        blocks.append(p)
        assert rt.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
        return p.value

    def back(ptr, like):
        out = np.zeros_like(like)
        assert rt.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0
        return out

    col = lambda a, t: np.ascontiguousarray(np.asarray(a, t).T)
    m_like = np.full(2 * m + 1, SENT, bodies.MOTION_DTYPE)
    s_like = np.full(2 * m * 4 + 1, SENT, align.SYSTEM_DTYPE)
    args = ([dev(col(e["z0"], np.float32)) for e in entries], [dev(col(e["l0"], np.int32)) for e in entries], [dev(col(e["z1"], np.float32)) for e in entries],
            [dev(col(e["l1"], np.int32)) for e in entries], [to_cam(e["c0"]) for e in entries], [to_cam(e["c1"]) for e in entries], [e["K"] for e in entries],
            np.array([[0, 0, 0], [1, 0, 0]], np.int32), [to_p(e["p"]) for e in entries], m)
    for with_systems in (True, False):
        dm, ds = dev(m_like), dev(s_like)
        bodies.estimate_images_device(box, rows, cols, *args, dm, ds if with_systems else None)  # asynchronous
        box.synchronize()
        gm, gs = back(dm, m_like), back(ds, s_like)
        assert gm[:2 * m].tobytes() == got.tobytes() and gm[2 * m].tobytes() == m_like[0].tobytes()  # past its end: untouched
        if with_systems:
            assert gs[:2 * m * 4].tobytes() == systems.tobytes() and gs[2 * m * 4].tobytes() == s_like[0].tobytes()
        else:
            assert gs.tobytes() == s_like.tobytes()
    for p in blocks:
        rt.hipFree(p)


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------
def raw(box, e, M, over=None):
    """sfb_estimate_images at the C interface on one entry with sentinel-filled outputs one record longer than the call needs;
    over: replacements of single arguments"""
    rows, cols = e["z0"].shape
    col = lambda a, t: np.ascontiguousarray(np.asarray(a, t).T)
    keep = [col(e["z0"], np.float32), col(e["l0"], np.int32), col(e["z1"], np.float32), None if e["l1"] is None else col(e["l1"], np.int32)]
    one = lambda a: None if a is None else (C.c_void_p * 1)(a.ctypes.data)
    its = int(e["p"]["iterations"])
    mot = np.full(M + 1, SENT, bodies.MOTION_DTYPE)
    sysm = np.full(M * (its + 1) + 1, SENT, align.SYSTEM_DTYPE)
    a = dict(h=box.h, rows=rows, cols=cols, n=1, z0=one(keep[0]), l0=one(keep[1]), z1=one(keep[2]), l1=one(keep[3]), c0=(bodies.SfbCamera * 1)(to_cam(e["c0"])),
             c1=(bodies.SfbCamera * 1)(to_cam(e["c1"])), K=(C.c_int32 * 1)(e["K"]), pairs=None if e["pairs"] is None else (C.c_int32 * M)(*e["pairs"]),
             p=(bodies.SfbParams * 1)(to_p(e["p"])), M=M, mot=mot.ctypes.data, sys=sysm.ctypes.data)
    a.update(over or {})
    code = bodies._bind(box.api).estimate_images(*[a[k] for k in ("h", "rows", "cols", "n", "z0", "l0", "z1", "l1", "c0", "c1", "K", "pairs", "p", "M", "mot", "sys")])
    untouched = (mot == np.full(1, SENT, bodies.MOTION_DTYPE)).all() and (sysm == np.full(1, SENT, align.SYSTEM_DTYPE)).all()
    return code, untouched, mot, sysm, keep


def test_refusals_write_nothing(box):
    rows, cols, M = 37, 53, 3
    pair = bc.with_wall_patch(rows, cols, bc.pyramid_pair(rows, cols))
    good = entry(pair, 2, pairs=[1, 2, 0], iterations=2)
    code, untouched, mot, sysm, _ = raw(box, good, M)
    assert code == 0 and not untouched and mot[M].tobytes() == np.full(1, SENT, bodies.MOTION_DTYPE).tobytes() and sysm[-1].tobytes() == np.full(1, SENT, align.SYSTEM_DTYPE).tobytes()
    nan, inf = float("nan"), float("inf")
    null1 = (C.c_void_p * 1)(None)
    bad_pose = np.eye(4, dtype=np.float32)
    bad_pose[1, 3] = nan
    inf_pose = np.eye(4, dtype=np.float32)
    inf_pose[0, 0] = inf
    cam_with = lambda **kw: (bodies.SfbCamera * 1)(to_cam(dict(pair[4], **kw)))
    par_with = lambda **kw: (bodies.SfbParams * 1)(to_p(br.params(**kw)))
    overs = [dict(h=C.c_void_p()), dict(n=-1), dict(n=65536), dict(rows=0), dict(cols=0), dict(rows=4097), dict(rows=4096, cols=4097),
             dict(z0=None), dict(l0=None), dict(z1=None), dict(c0=None), dict(c1=None), dict(K=None), dict(p=None), dict(mot=None),
             dict(z0=null1), dict(l0=null1), dict(z1=null1), dict(l1=null1), dict(l1=None),  # the last two: a non-zero pair without L1
             dict(M=0), dict(M=257), dict(M=-1), dict(K=(C.c_int32 * 1)(-1)), dict(K=(C.c_int32 * 1)(M + 1)), dict(pairs=(C.c_int32 * M)(1, -1, 0)), dict(pairs=(C.c_int32 * M)(0, 0, -5)),
             dict(c0=cam_with(fx=0.0)), dict(c1=cam_with(fy=0.0)), dict(c0=cam_with(cx=nan)), dict(c1=cam_with(fy=inf)), dict(c0=cam_with(pose=bad_pose)), dict(c1=cam_with(pose=inf_pose)),
             dict(p=par_with(dist_max=0.0)), dict(p=par_with(dist_max=1.5)), dict(p=par_with(dist_max=nan)), dict(p=par_with(z_max=0.0)), dict(p=par_with(z_max=33.0)),
             dict(p=par_with(normal_dz=0.0)), dict(p=par_with(normal_dz=33.0)), dict(p=par_with(normal_dz=inf)), dict(p=par_with(damping=-1.0)), dict(p=par_with(damping=nan)),
             dict(p=par_with(iterations=0)), dict(p=par_with(iterations=65)), dict(p=par_with(min_pairs=5))]
    for over in overs:
        code, untouched, *_ = raw(box, good, M, over)
        assert code == -1 and untouched and box.api.last_error(), list(over)
    b = bodies._bind(box.api)
    for fn in (b.estimate_images, b.estimate_images_device):
        assert fn(box.h, rows, cols, 0, None, None, None, None, None, None, None, None, None, M, None, None) == 0  # n == 0 is fine and touches nothing
        assert fn(None, rows, cols, 0, None, None, None, None, None, None, None, None, None, M, None, None) == -1
    # a pair above K needs no L1, and systems_out may be NULL; then the same call again gives the same bytes
    code, _, first, _, _ = raw(box, dict(good, l1=None, pairs=[0, 0, 4]), M, dict(sys=None))
    code2, _, second, _, _ = raw(box, dict(good, l1=None, pairs=[0, 0, 4]), M)
    assert code == 0 == code2 and first.tobytes() == second.tobytes()
    with pytest.raises(SfError):
        bodies.estimate_images(box, [pair[0]], [pair[1][:, :-1]], [pair[2]], None, [to_cam(pair[4])], [to_cam(pair[5])], [1])
    with pytest.raises(SfError):
        bodies.estimate_images(box, [pair[0]], [pair[1]], [pair[2]], None, [to_cam(pair[4])], [to_cam(pair[5])], [1, 1])


# ---- 9. the state a call leaves alone ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walked(hip_auto):
    s, m = sphere_walk(hip_auto, 5)
    yield s, m
    m.close()
    s.close()


def test_a_call_leaves_everything_else_alone(walked):
    s, m = walked
    own = view.default_view(s, m)
    db = keyframes.KeyframeDb(s, 4, n_ferns=64, capacity=4)
    db.add_streams([0], np.eye(4)[None], [0], [1])
    cam = tc.cam(s.rows, s.cols)
    t = tracks.Tracker(s, 2, 4)
    t.update_streams([0], [0], [tracks.Camera(cam["pose"], cam["cx"], cam["cy"], cam["fx"], cam["fy"])])

    def readable():
        i = m.info()
        return (s.current(0)[0].tobytes(), s.current(0)[1].tobytes(), s.b_image(0).tobytes(), i["count"], i["tick"], i["pose"].tobytes(), tuple(i["stats"]),
                m.download().tobytes(), m.index_map().tobytes(), s.prediction()[0].tobytes(), s.prediction()[1].tobytes(),
                score.score_streams([m], [own], [0]).tobytes(), db.query_streams([0], None, 2).tobytes(), regions.label_streams(s, [0], None, 8)[0].tobytes(),
                align.refine_streams([m], [own], [0]).tobytes(), repr(join.thin([m], join.Params(dry_run=True))), repr(t.slot_info(0)), repr(t.slot_info(1)), repr(t.info()))

    before = readable()
    small = bc.with_wall_patch(37, 53, bc.pyramid_pair(37, 53))
    first = call(s, [entry(small, 2, **LOOSE)], 2)
    big = bc.pyramid_pair(130, 66, *bc.MOVING_CAMERA)  # a larger call: the scratch grows
    call(s, [entry(big, 1, **LOOSE)] * 3, 256)
    again = call(s, [entry(small, 2, **LOOSE)], 2)
    assert readable() == before
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    nxt = t.update_streams([0], [0], [tracks.Camera(cam["pose"], cam["cx"], cam["cy"], cam["fx"], cam["fy"])])  # the tracker's slot goes on from its frame
    assert int(nxt[0]["n_matched"][0]) == int(nxt[0]["n_tracked"][0])
    t.close()
    db.close()


# ---- 10. a destroyed handle; the other libraries -------------------------------------------------------------------------------
def test_a_call_after_sf_destroy_is_refused(hip_auto):
    s = small_solver(hip_auto, 32, 40)
    pair = bc.pyramid_pair(32, 40)
    e = entry(pair, 1, **LOOSE)
    assert raw(s, e, 1)[0] == 0
    gone = C.c_void_p(s.h.value)
    s.close()
    code, untouched, *_ = raw(s, e, 1, dict(h=gone))
    assert code == -3 and untouched  # SF_ERR_STATE
    b = bodies._bind(hip_auto)
    assert b.estimate_images_device(gone, 32, 40, 0, None, None, None, None, None, None, None, None, None, 1, None, None) == -3
    s2 = small_solver(hip_auto, 32, 40)  # (a new handle, at the old address or another: alive)
    assert raw(s2, e, 1)[0] == 0
    s2.close()


@pytest.mark.parametrize("lib", ["libsf_hip_precise.so", "libsf_hip_reforder.so"])
def test_the_precise_and_reference_order_libraries_do_the_same(lib):
    import staticfusion_amd as sf

    api = sf.Api(os.path.join(os.path.dirname(sf.LIB), lib), "sf_")
    s = small_solver(api, 48, 64)
    pair = bc.with_wall_patch(65, 33, bc.pyramid_pair(65, 33, *bc.MOVING_CAMERA))
    same(s, [entry(pair, 2, iterations=3, min_pairs=6, damping=1e-4)], 2, lib)
    s.close()
