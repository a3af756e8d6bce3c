"""Region tracks (include/sf_tracks.h, staticfusion_amd/tracks.py) on the GPU. Every comparison is integer or bit equality
with the NumPy statement of the header in tests/track_ref.py: summaries, track records, id images and the slot counters of the
frame pairs of tests/track_cases.py at image sizes below, at and past the block sizes of the kernels, the LDS and the
global-atomic paths of the overlap kernel on both sides of the budget, five updates of one slot, resets, a batch against single
trackers, the three forms against one another, the stream form after real frames, the state an update must leave alone, every
refusal, a tracker that outlives its handle, and the other two libraries. No tolerance appears anywhere and nothing here
asserts a time."""
import ctypes as C
import os

import numpy as np
import pytest

import region_ref as rr
import track_cases as tc
import track_ref as tr
from conftest import hip_runtime
from staticfusion_amd import SfError, align, join, keyframes, regions, score, tracks, view
from test_gpu_regions import sphere_walk
from test_gpu_view import small_solver

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 7), (37, 53), (65, 33), (130, 66)]
SENT = -77


@pytest.fixture(scope="module")
def box(hip_auto):
    s = small_solver(hip_auto, 60, 80)
    yield s
    s.close()


def to_cam(c):
    return tracks.Camera(c["pose"], c["cx"], c["cy"], c["fx"], c["fy"])


def to_rp(p):
    return regions.Params(**{k: p[k] for k in ("z_max", "b_max", "dz_abs", "dz_rel", "connectivity", "min_pixels", "use_b")})


def to_tp(p):
    return tracks.Params(**p)


def same(got, ref, what):
    """one update: (summaries, records, id images) of the module against (summary, records, id image, O) of the reference"""
    summ, rec, ids = ref[:3]
    k = int(summ["n_tracked"])
    assert got[0][0].tobytes() == summ.tobytes(), (what, got[0][0], summ)
    assert got[1][0].tobytes() == rec[:k].tobytes(), (what, got[1][0], rec[:k])
    assert got[2][0].dtype == np.int32 and np.array_equal(got[2][0], ids), (what, np.argwhere(got[2][0] != ids)[:5])


def run_case(box, steps, max_tracks, what=""):
    """the steps on one slot of a fresh tracker and on a reference slot, compared after every update; the reference's results"""
    rows, cols = steps[0][0].shape
    t = tracks.Tracker(box, 1, max_tracks, rows, cols)
    slot, out = tr.Slot(), []
    assert t.slot_info(0) == slot.info() == dict(frames=0, next_id=1, n_tracks=0)
    for f, (z, b, cam, rp, tp) in enumerate(steps):
        got = t.update_images([0], [z], [b], [to_cam(cam)], [to_rp(rp)], [to_tp(tp)], ids=True)
        ref = tr.update(slot, z, b, cam, rp, tp, max_tracks)
        same(got, ref, (what, f))
        assert t.slot_info(0) == slot.info(), (what, f)
        out.append(ref)
    t.close()
    return out


# ---- 1. sizes x frame pairs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_every_frame_pair_equals_numpy(box, rows, cols):
    seen = {name: run_case(box, steps, 8, name) for name, steps in tc.cases_of(rows, cols).items()}
    first, second = seen["identical"]
    assert int(second[0]["n_matched"]) == int(first[0]["n_tracked"]) and int(second[0]["n_born"]) == 0
    assert all(int(r["overlap"]) == int(r["n"]) for r in second[1][:int(second[0]["n_tracked"])])
    assert int(seen["leaves"][1][0]["n_warped"]) == 0 == int(seen["behind"][1][0]["n_warped"])
    if rows >= 37:
        assert [int(s[0]["n_tracked"]) for s in seen["split"]] == [1, 2] and int(seen["split"][1][0]["n_matched"]) == 1
        assert [int(x) for x in seen["split"][1][1]["id"][:2]] == [1, 2]  # the larger part (region 1) keeps the id
        assert [int(s[0]["n_tracked"]) for s in seen["merge"]] == [2, 1] and int(seen["merge"][1][0]["n_ended"]) == 1
        assert int(seen["swap_gated"][1][0]["n_matched"]) == 0 and int(seen["swap_ungated"][1][0]["n_matched"]) == 2
        assert [int(x) for x in seen["swap_ungated"][1][1]["id"][:2]] == [1, 2]
        assert [int(x) for x in seen["gate_edge"][1][1]["prev_region"][:2]] == [1, 0]  # met exactly; one ulp beyond
        assert [int(x) for x in seen["gate_off"][1][1]["prev_region"][:2]] == [1, 2]
        back = seen["backwards"][1]
        assert int(back[0]["n_matched"]) == 1 and int(back[1]["overlap"][0]) > int(back[1]["n"][0])  # several sources per target
        assert int(seen["translation"][1][0]["n_matched"]) == 1 and int(seen["roll"][1][0]["n_warped"]) > 0
        assert int(seen["shift7"][1][0]["n_matched"]) == 1


def test_qvga_once(box):
    cases = tc.cases_of(240, 320)
    for name in ("translation", "split", "backwards"):
        out = run_case(box, cases[name], 8, name)
        assert int(out[1][0]["n_matched"]) == 1


@pytest.mark.parametrize("max_tracks", [1, 3])
def test_more_regions_than_tracks(box, max_tracks):
    out = run_case(box, tc.cases_of(37, 53)["five"], max_tracks)
    for summ, rec, ids, _ in out:
        assert int(summ["n_regions"]) == 5 and int(summ["n_tracked"]) == max_tracks and int(summ["n_untracked"]) == 5 - max_tracks
        assert sorted(set(ids.ravel().tolist())) == list(range(max_tracks + 1))
    assert int(out[1][0]["n_matched"]) == max_tracks


# ---- 2. the two paths of the overlap kernel ----------------------------------------------------------------------------------
@pytest.mark.parametrize("max_tracks", [8, 64, 65, 256])
def test_lds_and_global_atomic_paths(box, max_tracks):
    """a checkerboard of 1 x 1 regions: K_prev * K = max_tracks^2, against the LDS budget of 4096 pairs: 64 (LDS), 4096 (LDS, the
    budget exactly), 4225 and 65536 (global atomics)"""
    rows, cols = 37, 53
    z = tc.checkerboard(rows, cols)
    s = tc.step(z, tc.cam(rows, cols), rp=dict(connectivity=4))
    moved = tc.step(np.roll(z, 2, axis=0), tc.cam(rows, cols), rp=dict(connectivity=4))  # two rows down: square on square
    out = run_case(box, [s, s, moved], max_tracks)
    assert int(out[0][0]["n_regions"]) == (rows * cols + 1) // 2 and int(out[1][0]["n_matched"]) == max_tracks
    assert (np.diag(out[1][3]) == 1).all() and int(out[1][3].sum()) == max_tracks
    assert 0 < int(out[2][0]["n_matched"]) < max_tracks  # (the wrapped rows break the pattern: the numbering moves)


# ---- 3. five updates of one slot; resets -------------------------------------------------------------------------------------
def test_five_updates_of_one_slot(box):
    out = run_case(box, tc.long_case(60, 80), 8)
    walker = [int(o[1]["id"][0]) for o in out]
    assert walker == [1] * 5 and [int(o[1]["age"][0]) for o in out] == [0, 1, 2, 3, 4] and all(int(o[1]["birth_frame"][0]) == 0 for o in out)
    assert [int(o[0]["n_tracked"]) for o in out] == [2, 2, 1, 1, 2] and [int(o[0]["n_ended"]) for o in out] == [0, 0, 1, 0, 0]
    again = out[4][1][1]
    assert int(out[0][1]["id"][1]) == 2 and int(again["id"]) == 3 and int(again["birth_frame"]) == 4 and int(again["age"]) == 0  # same place, new id
    assert [int(o[0]["next_id"]) for o in out] == [3, 3, 3, 3, 4]


def test_reset_with_and_without_id_restart(box):
    rows, cols = 37, 53
    steps = tc.cases_of(rows, cols)["identical"]
    t = tracks.Tracker(box, 2, 8, rows, cols)
    slots = [tr.Slot(), tr.Slot()]

    def both(step):
        z, b, cam, rp, tp = step
        got = t.update_images([0, 1], [z, z], [b, b], [to_cam(cam)] * 2, [to_rp(rp)] * 2, [to_tp(tp)] * 2, ids=True)
        for q in range(2):
            same([[x[q]] for x in got], tr.update(slots[q], z, b, cam, rp, tp, 8), q)
            assert t.slot_info(q) == slots[q].info()
        return got

    both(steps[0])
    both(steps[1])
    t.reset([0], restart_ids=False)
    slots[0].reset(False)
    assert t.slot_info(0) == slots[0].info() == dict(frames=2, next_id=3, n_tracks=0) and t.slot_info(1) == slots[1].info()
    got = both(steps[0])
    assert [int(x) for x in got[1][0]["id"]] == [3, 4] and int(got[0][0]["n_born"]) == 2 and int(got[0][1]["n_matched"]) == 2
    t.reset([0, 1], restart_ids=True)
    slots[0].reset(True)
    slots[1].reset(True)
    assert t.slot_info(1) == dict(frames=0, next_id=1, n_tracks=0)
    got = both(steps[1])
    assert [int(x) for x in got[1][1]["id"]] == [1, 2] and [int(x) for x in got[1][1]["birth_frame"]] == [0, 0]
    t.close()


# ---- 4. batches; refusals ----------------------------------------------------------------------------------------------------
def raw_update(t, slots, steps, extra=1, ids=True, fn="update_images"):
    """sft_update_images at the C interface with sentinel-filled outputs one record longer than the call needs"""
    n, m = len(slots), t.max_tracks
    col = [[np.ascontiguousarray(np.asarray(s[k], np.float32).T) for s in steps] for k in range(2)]
    dp, bp = [(C.c_void_p * n)(*[a.ctypes.data for a in col[k]]) for k in range(2)]
    summ = np.full(n + extra, SENT, tracks.SUMMARY_DTYPE)
    rec = np.full(n * m + extra, SENT, tracks.TRACK_DTYPE)
    imgs = [np.full((t.cols, t.rows), SENT, np.int32) for _ in range(n)]
    ip = (C.c_void_p * n)(*[a.ctypes.data for a in imgs]) if ids else None
    code = t.b.update_images(t.t, t.rows, t.cols, n, (C.c_int32 * n)(*slots), dp, bp, (tracks.SftCamera * n)(*[to_cam(s[2]) for s in steps]),
                             (regions.SfrParams * n)(*[to_rp(s[3]) for s in steps]), (tracks.SftParams * n)(*[to_tp(s[4]) for s in steps]), summ.ctypes.data,
                             rec.ctypes.data, ip)
    return code, summ, rec, imgs


def test_a_batch_equals_single_trackers(box):
    rows, cols = 65, 33
    c = tc.cases_of(rows, cols)
    names = ["identical", "translation", "roll", "swap_ungated", "gate_edge", "backwards"]
    m = 5
    t = tracks.Tracker(box, 7, m, rows, cols)
    single = [tracks.Tracker(box, 1, m, rows, cols) for _ in range(7)]
    seventh = c["shift1"]
    for trk, slot in ((t, 6), (single[6], 0)):
        trk.update_images([slot], [seventh[0][0]], [seventh[0][1]], [to_cam(seventh[0][2])], [to_rp(seventh[0][3])], [to_tp(seventh[0][4])])
    order = [3, 0, 5, 1, 4, 2]  # slot of entry q
    for f in range(2):
        steps = [c[names[s]][f] for s in order]
        code, summ, rec, imgs = raw_update(t, order, steps)
        assert code == 0
        assert summ[6].tobytes() == np.full(1, SENT, tracks.SUMMARY_DTYPE).tobytes() and rec[6 * m].tobytes() == np.full(1, SENT, tracks.TRACK_DTYPE).tobytes()
        for q, s in enumerate(order):
            z, b, cam, rp, tp = steps[q]
            one = single[s].update_images([0], [z], [b], [to_cam(cam)], [to_rp(rp)], [to_tp(tp)], ids=True)
            k = int(one[0][0]["n_tracked"])
            assert summ[q].tobytes() == one[0][0].tobytes() and rec[q * m:q * m + k].tobytes() == one[1][0].tobytes(), (f, q)
            assert rec[q * m + k:(q + 1) * m].tobytes() == bytes(tracks.TRACK_DTYPE.itemsize * (m - k)), (f, q)  # the zeroed tail
            assert np.array_equal(imgs[q].T, one[2][0]) and t.slot_info(s) == single[s].slot_info(0), (f, q)
    assert t.slot_info(6) == single[6].slot_info(0) == dict(frames=1, next_id=2, n_tracks=1)
    a = t.update_images([6], [seventh[1][0]], [seventh[1][1]], [to_cam(seventh[1][2])], [to_rp(seventh[1][3])], [to_tp(seventh[1][4])], ids=True)
    o = single[6].update_images([0], [seventh[1][0]], [seventh[1][1]], [to_cam(seventh[1][2])], [to_rp(seventh[1][3])], [to_tp(seventh[1][4])], ids=True)
    assert a[0].tobytes() == o[0].tobytes() and a[1][0].tobytes() == o[1][0].tobytes() and np.array_equal(a[2][0], o[2][0]) and int(a[0][0]["n_matched"]) == 1
    for x in single + [t]:
        x.close()


def test_refusals_change_nothing(box):
    rows, cols, m = 37, 53, 4
    steps = tc.cases_of(rows, cols)["identical"]
    t = tracks.Tracker(box, 3, m, rows, cols)
    ref = tracks.Tracker(box, 3, m, rows, cols)
    for trk in (t, ref):
        assert raw_update(trk, [0, 1], [steps[0], steps[0]])[0] == 0
    nan, inf = float("nan"), float("inf")
    z, b, cam, rp, tp = steps[1]

    def variant(cam_kw=None, rp_kw=None, tp_kw=None, pose=None):
        c = dict(cam, **(cam_kw or {}))
        if pose is not None:
            c["pose"] = pose
        return (z, b, c, dict(rp, **(rp_kw or {})), dict(tp, **(tp_kw or {})))

    bad_pose = np.eye(4, dtype=np.float32)
    bad_pose[1, 3] = nan
    inf_pose = np.eye(4, dtype=np.float32)
    inf_pose[0, 0] = inf
    bad_entries = [variant(cam_kw=dict(fx=0.0)), variant(cam_kw=dict(fy=0.0)), variant(cam_kw=dict(cx=nan)), variant(cam_kw=dict(fy=inf)), variant(pose=bad_pose),
                   variant(pose=inf_pose), variant(rp_kw=dict(z_max=0.0)), variant(rp_kw=dict(connectivity=5)), variant(rp_kw=dict(min_pixels=0)),
                   variant(rp_kw=dict(dz_abs=nan)), variant(rp_kw=dict(use_b=2)), variant(tp_kw=dict(min_overlap=0)), variant(tp_kw=dict(min_share=-1)),
                   variant(tp_kw=dict(min_share=1025)), variant(tp_kw=dict(dz_abs=-0.1)), variant(tp_kw=dict(dz_rel=nan)), variant(tp_kw=dict(dz_abs=inf)),
                   variant(tp_kw=dict(use_depth_gate=2))]
    outs = []
    for q, e in enumerate(bad_entries):
        code, summ, rec, imgs = raw_update(t, [0, 1], [steps[1], e])
        assert code == -1 and box.api.last_error(), q
        outs.append((summ, rec, imgs))
    for slots in ([0, 0], [1, 2, 1], [0, 3], [-1, 0]):  # the same slot twice; a slot out of range
        code, summ, rec, imgs = raw_update(t, slots, [steps[1]] * len(slots))
        assert code == -1, slots
        outs.append((summ, rec, imgs))
    # sizes, counts and null arguments, at the C interface
    bd = t.b
    col = np.ascontiguousarray(z.T)
    one = (C.c_void_p * 1)(col.ctypes.data)
    sl, cm, rpp, tpp = (C.c_int32 * 1)(2), (tracks.SftCamera * 1)(to_cam(cam)), (regions.SfrParams * 1)(to_rp(rp)), (tracks.SftParams * 1)(to_tp(tp))
    summ, rec = np.full(2, SENT, tracks.SUMMARY_DTYPE), np.full(m + 1, SENT, tracks.TRACK_DTYPE)
    sp, rcp = summ.ctypes.data, rec.ctypes.data
    with_b = (regions.SfrParams * 1)(to_rp(dict(rp, use_b=1)))
    for fn in (bd.update_images, bd.update_images_device):
        for args in ((None, rows, cols, 1, sl, one, None, cm, rpp, tpp, sp, rcp, None), (t.t, rows, cols, -1, sl, one, None, cm, rpp, tpp, sp, rcp, None),
                     (t.t, rows, cols, 65536, sl, one, None, cm, rpp, tpp, sp, rcp, None), (t.t, rows + 1, cols, 1, sl, one, None, cm, rpp, tpp, sp, rcp, None),
                     (t.t, cols, rows, 1, sl, one, None, cm, rpp, tpp, sp, rcp, None), (t.t, rows, cols, 1, None, one, None, cm, rpp, tpp, sp, rcp, None),
                     (t.t, rows, cols, 1, sl, None, None, cm, rpp, tpp, sp, rcp, None), (t.t, rows, cols, 1, sl, (C.c_void_p * 1)(None), None, cm, rpp, tpp, sp, rcp, None),
                     (t.t, rows, cols, 1, sl, one, None, None, rpp, tpp, sp, rcp, None), (t.t, rows, cols, 1, sl, one, None, cm, None, tpp, sp, rcp, None),
                     (t.t, rows, cols, 1, sl, one, None, cm, rpp, None, sp, rcp, None), (t.t, rows, cols, 1, sl, one, None, cm, rpp, tpp, None, rcp, None),
                     (t.t, rows, cols, 1, sl, one, None, cm, rpp, tpp, sp, None, None), (t.t, rows, cols, 1, sl, one, None, cm, with_b, tpp, sp, rcp, None)):
            assert fn(*args) == -1, (fn.__name__, args[1:4])
        assert fn(t.t, rows, cols, 0, None, None, None, None, None, None, None, None, None) == 0  # n == 0 is fine and touches nothing
    # the stream form: the tracker's size is not the handle's; on a tracker of the handle's size, a stream out of range
    st = (C.c_int32 * 1)(0)
    assert bd.update_streams(t.t, 1, sl, st, cm, rpp, tpp, sp, rcp, None) == -1
    ts = tracks.Tracker(box, 1, m)
    img = np.zeros((box.cols, box.rows), np.float32)
    getter = box.api.get_current(box.h, 1, img.ctypes.data_as(C.POINTER(C.c_float)), None)
    assert getter != 0 and bd.update_streams(ts.t, 1, (C.c_int32 * 1)(0), (C.c_int32 * 1)(1), cm, rpp, tpp, sp, rcp, None) == getter
    assert bd.update_streams(ts.t, 1, (C.c_int32 * 1)(0), None, cm, rpp, tpp, sp, rcp, None) == -1 and ts.slot_info(0) == dict(frames=0, next_id=1, n_tracks=0)
    ts.close()
    assert bd.reset_slots(t.t, 1, (C.c_int32 * 1)(3), 0) == -1 and bd.reset_slots(t.t, -1, sl, 0) == -1 and bd.reset_slots(t.t, 1, None, 0) == -1
    assert bd.reset_slots(None, 1, sl, 0) == -1 and bd.reset_slots(t.t, 0, None, 1) == 0
    assert bd.slot_info(t.t, 3, sp) == -1 and bd.slot_info(t.t, 0, None) == -1 and bd.tracker_info(t.t, None) == -1 and bd.tracker_info(None, sp) == -1
    out = C.c_void_p()
    for args in ((None, rows, cols, 1, 1), (box.h, 0, cols, 1, 1), (box.h, rows, 4097, 1, 1), (box.h, 4096, 4097, 1, 1), (box.h, rows, cols, 0, 1), (box.h, rows, cols, 65536, 1),
                 (box.h, rows, cols, 1, 0), (box.h, rows, cols, 1, 257)):
        assert bd.tracker_create(*args, C.byref(out)) == -1 and not out, args[1:]
    assert bd.tracker_create(box.h, rows, cols, 1, 1, None) == -1
    # nothing was written and no state changed: every slot goes on as the tracker that saw none of this
    assert (summ == np.full(1, SENT, tracks.SUMMARY_DTYPE)).all() and (rec == np.full(1, SENT, tracks.TRACK_DTYPE)).all()
    for s_, r_, i_ in outs:
        assert (s_ == np.full(1, SENT, tracks.SUMMARY_DTYPE)).all() and (r_ == np.full(1, SENT, tracks.TRACK_DTYPE)).all() and all((a == SENT).all() for a in i_)
    assert t.info() == dict(rows=rows, cols=cols, n_slots=3, max_tracks=m)
    for s in range(3):
        assert t.slot_info(s) == ref.slot_info(s)
    a, o = raw_update(t, [2, 0, 1], [steps[1]] * 3), raw_update(ref, [2, 0, 1], [steps[1]] * 3)
    assert a[0] == 0 == o[0] and a[1].tobytes() == o[1].tobytes() and a[2].tobytes() == o[2].tobytes() and all(np.array_equal(x, y) for x, y in zip(a[3], o[3]))
    assert [int(x) for x in a[1]["n_matched"][:3]] == [0, 2, 2]
    with pytest.raises(SfError):
        t.update_images([0], [np.zeros((cols, rows), np.float32)], None, [to_cam(cam)], [to_rp(rp)])
    t.close()
    ref.close()


# ---- 5. the three forms ------------------------------------------------------------------------------------------------------
def test_the_three_forms_agree(box):
    rows, cols, m = box.rows, box.cols, 6
    c = tc.cases_of(rows, cols)
    names = ["translation", "swap_ungated", "five"]
    host, devt, strm = tracks.Tracker(box, 3, m), tracks.Tracker(box, 3, m), tracks.Tracker(box, 1, m)
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

    s_like, r_like, i_like = np.full(4, SENT, tracks.SUMMARY_DTYPE), np.full(3 * m + 1, SENT, tracks.TRACK_DTYPE), np.full((cols, rows), SENT, np.int32)
    slots = [tr.Slot() for _ in range(3)]
    for f in range(2):
        steps = [c[k][f] for k in names]
        cams, rps, tps = [to_cam(s[2]) for s in steps], [to_rp(s[3]) for s in steps], [to_tp(s[4]) for s in steps]
        h = host.update_images([0, 1, 2], [s[0] for s in steps], [s[1] for s in steps], cams, rps, tps, ids=True)
        dd = [dev(np.ascontiguousarray(s[0].T)) for s in steps]
        ds, dr = dev(s_like), dev(r_like)
        di = [dev(i_like), None, dev(i_like)]
        devt.update_images_device([0, 1, 2], dd, None, cams, rps, tps, ds, dr, di)  # asynchronous; b is not read without use_b
        box.synchronize()
        gs, gr = back(ds, s_like), back(dr, r_like)
        assert gs[3].tobytes() == s_like[3].tobytes() and gr[3 * m].tobytes() == r_like[0].tobytes()  # past their ends: untouched
        for q in range(3):
            ref = tr.update(slots[q], *steps[q], m)
            same([[x[q]] for x in h], ref, (f, q))
            assert gs[q].tobytes() == ref[0].tobytes() and gr[q * m:(q + 1) * m].tobytes() == ref[1].tobytes(), (f, q)
            if di[q]:
                assert np.array_equal(back(di[q], i_like).T, ref[2]), (f, q)
            assert devt.slot_info(q) == host.slot_info(q) == slots[q].info()
        # the stream form reads the stream's depth (use_b = 0: the b image belongs to the solver)
        z = steps[0][0]
        box.set_current(0, z, np.zeros_like(z))
        assert box.current(0)[0].tobytes() == z.tobytes()
        st = strm.update_streams([0], [0], [cams[0]], [rps[0]], [tps[0]], ids=True)
        assert st[0][0].tobytes() == h[0][0].tobytes() and st[1][0].tobytes() == h[1][0].tobytes() and np.array_equal(st[2][0], h[2][0])
    for p in blocks:
        rt.hipFree(p)
    for t in (host, devt, strm):
        t.close()


# ---- 6. real frames; the state an update leaves alone ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walked(hip_auto):
    s, m = sphere_walk(hip_auto, 5)
    yield s, m
    m.close()
    s.close()


def test_stream_form_after_real_frames_equals_image_form_and_numpy(walked):
    s, m = walked
    d, b = s.current(0)[0], s.b_image(0)
    rows, cols = d.shape
    cams = [tc.cam(rows, cols), tc.cam(rows, cols, tc.shift(x=0.01) @ tc.rot(1, 0.01))]
    rp, tp = dict(rr.params(min_pixels=4)), tr.params()
    a, c, slot = tracks.Tracker(s, 1, 16), tracks.Tracker(s, 1, 16), tr.Slot()
    for f in range(2):
        x = a.update_streams([0], [0], [to_cam(cams[f])], [to_rp(rp)], [to_tp(tp)], ids=True)
        y = c.update_images([0], [d], [b], [to_cam(cams[f])], [to_rp(rp)], [to_tp(tp)], ids=True)
        ref = tr.update(slot, d, b, cams[f], rp, tp, 16)
        same(x, ref, f)
        same(y, ref, f)
        print("real frames, update %d:" % f, ref[0])
    assert int(ref[0]["n_regions"]) > 0 and int(ref[0]["n_warped"]) > 0
    cen = tracks.centroids(x[1][0])
    assert cen.shape == (int(ref[0]["n_tracked"]), 3) and np.isfinite(cen).all()
    assert set(tracks.velocities(x[1][0], x[1][0], 1.0)) == set(int(i) for i in x[1][0]["id"])
    a.close()
    c.close()


def test_an_update_leaves_everything_else_alone(walked):
    s, m = walked
    own = view.default_view(s, m)
    db = keyframes.KeyframeDb(s, 4, n_ferns=64, capacity=4)
    db.add_streams([0], np.eye(4)[None], [0], [1])

    def readable():
        i = m.info()
        return (s.current(0)[0].tobytes(), s.current(0)[1].tobytes(), s.b_image(0).tobytes(), i["count"], i["tick"], i["pose"].tobytes(), tuple(i["stats"]),
                m.download().tobytes(), m.index_map().tobytes(), s.prediction()[0].tobytes(), s.prediction()[1].tobytes(),
                score.score_streams([m], [own], [0]).tobytes(), db.query_streams([0], None, 2).tobytes(), regions.label_streams(s, [0], None, 8)[0].tobytes(),
                align.refine_streams([m], [own], [0]).tobytes(), repr(join.thin([m], join.Params(dry_run=True))))

    before = readable()
    cam = tc.cam(s.rows, s.cols)
    t = tracks.Tracker(s, 2, 4)
    first = t.update_streams([0], [0], [to_cam(cam)])
    big = tracks.Tracker(s, 4, 256, 130, 66)  # a larger tracker and a larger call: both scratch blocks grow
    z = tc.checkerboard(130, 66)
    big.update_images([0, 1, 2], [z] * 3, None, [to_cam(tc.cam(130, 66))] * 3, [to_rp(rr.params(use_b=0, min_pixels=1, connectivity=4))] * 3)
    again = t.update_streams([1], [0], [to_cam(cam)])
    assert readable() == before
    assert first[0].tobytes() == again[0].tobytes() and first[1][0].tobytes() == again[1][0].tobytes()
    for x in (t, big, db):
        x.close()


# ---- 7. a tracker that outlives its handle; the other libraries ---------------------------------------------------------------
def test_a_tracker_outlives_its_handle(hip_auto):
    s = small_solver(hip_auto, 32, 40)
    t = tracks.Tracker(s, 2, 4)
    steps = tc.cases_of(32, 40)["identical"]
    assert raw_update(t, [0], [steps[0]])[0] == 0
    s.close()
    code, summ, rec, imgs = raw_update(t, [0], [steps[1]])
    assert code == -3 and (summ == np.full(1, SENT, tracks.SUMMARY_DTYPE)).all() and (imgs[0] == SENT).all()  # SF_ERR_STATE
    info = np.zeros(1, tracks.INFO_DTYPE)
    assert t.b.tracker_info(t.t, info.ctypes.data) == -3 and t.b.slot_info(t.t, 0, info.ctypes.data) == -3
    assert t.b.reset_slots(t.t, 1, (C.c_int32 * 1)(0), 0) == -3
    t.close()  # the shell
    s2 = small_solver(hip_auto, 32, 40)
    t2 = tracks.Tracker(s2, 2, 4)
    run = [raw_update(t2, [1], [st]) for st in steps]
    assert run[0][0] == 0 == run[1][0] and int(run[1][1]["n_matched"][0]) == 2
    t2.close()
    s2.close()


@pytest.mark.parametrize("lib", ["libsf_hip_precise.so", "libsf_hip_reforder.so"])
def test_the_precise_and_reference_order_libraries_do_the_same(lib):
    import staticfusion_amd as sf

    api = sf.Api(os.path.join(os.path.dirname(sf.LIB), lib), "sf_")
    s = small_solver(api, 48, 64)
    run_case(s, tc.cases_of(65, 33)["roll"], 8, lib)
    s.close()
