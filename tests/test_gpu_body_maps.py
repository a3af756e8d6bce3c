"""Body maps (include/sf_body_maps.h, staticfusion_amd/body_maps.py) on the GPU. Maps, counts, tick and pose are held to
tests/body_map_ref.py byte for byte (a NaN made by arithmetic: a NaN in both at the same place): frames below, at and past a
workgroup's tile and the scan's trip; maps of every size around a wave and a workgroup; the same frame fused twice; a cell that
holds many pixels; keys that collide and walks that wrap at 64 slots; labels that are absent, below and above the region's; two
entries on one frame; translations, rotations and the move alone; the normal gate met and one ulp beyond; special confidences,
weights, colours and positions; the weight cap; colour given and missing; a batch against single calls; the host form against
the device form; the capacity; every refusal; what a call leaves alone; the calls that take a fused map afterwards; a destroyed
handle; and the other two libraries. No tolerance appears anywhere and nothing here asserts a time."""
import ctypes as C
import os

import numpy as np
import pytest

import body_cases as bc
import body_map_cases as pc
import body_map_ref as pr
import join_cases as jc
import join_ref
from conftest import hip_runtime
from staticfusion_amd import SfError, SurfelMap, align, body_maps, join, keyframes, regions, score, view
from test_gpu_view import small_solver, uploaded, walk

pytestmark = pytest.mark.gpu

F = np.float32
TICK = 5
POSE = np.array([[0, -1, 0, 0.25], [1, 0, 0, -1.5], [0, 0, 1, 2.0], [0, 0, 0, 1]], F)
EMPTY = np.zeros((0, 12), F)
SHIFT = np.array([[1, 0, 0, 0.003], [0, 1, 0, -0.002], [0, 0, 1, 0.004], [0, 0, 0, 1]], F)
TURN = bc.motion(rotvec=(0.02, -0.03, 0.01), shift=(0.002, 0.001, -0.003), centre=(0.0, 0.0, 2.3)).astype(F)
_fp = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def box(hip_auto):
    s = small_solver(hip_auto, 60, 80)
    yield s
    s.close()


def to_cam(c):
    return body_maps.Camera(c["pose"], c["cx"], c["cy"], c["fx"], c["fy"])


def to_p(p):
    return body_maps.Params(**p)


def same_bits32(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    a, b = a.ravel(), b.ravel()
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def state(m):
    i = m.info()
    return i["count"], i["tick"], i["pose"].tobytes(), tuple(i["stats"]), m.download().tobytes()


def room(s, surf, rows, cols):
    return max(surf.shape[0] + rows * cols, s.rows * s.cols)


def check_fuse(s, surf, z, lab, cam, t, W=None, colour=None, p=None, tick=TICK, exact=True, where=""):
    """one fuse of one map against the reference; returns (the surfels afterwards, the counts, the detail of the reference)"""
    p = pr.params() if p is None else p
    detail = {}
    want, wc = pr.fuse(surf, tick, z, lab, cam, t, W, colour, p, detail)
    rows, cols = z.shape
    m = uploaded(s, surf, pose=POSE, tick=tick, capacity=room(s, surf, rows, cols))
    stats = m.info()["stats"]
    got = body_maps.fuse([m], [z], [lab], [to_cam(cam)], [t], None if W is None else [W], None if colour is None else [colour], to_p(p))
    assert got == [wc], (where, got, wc)
    info, out = m.info(), m.download()
    assert info["count"] == wc["n_out"] == out.shape[0] and info["tick"] == tick + 1 and info["stats"] == stats, where
    assert info["pose"].tobytes() == np.asarray(cam["pose"], F).tobytes(), where
    if exact:
        assert out.tobytes() == want.tobytes(), where
    else:
        assert same_bits32(out, want), where
        keep = [3, 5, 6, 7]
        finite = np.isfinite(want)
        assert np.array_equal(out[finite], want[finite]) and same_bits32(out[:, keep], want[:, keep]), where
    with pytest.raises(SfError, match="index map"):
        m.index_map()
    m.close()
    return want, wc, detail


def scene(rows, cols, shift=0.0, t=2):
    return pc.plane(rows, cols, shift), pc.labels_mixed(rows, cols, t), pc.cam(rows, cols), pc.colours(rows, cols)


# ---- 1. frames ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (2, 5), (3, 3), (5, 4), (66, 130), (60, 80)])
def test_frames_against_the_reference(box, shape):
    rows, cols = shape
    z, lab, cam, rgb = scene(rows, cols)
    first, c0, _ = check_fuse(box, EMPTY, z, lab, cam, 2, None, rgb, tick=1, where="first sighting")
    if rows < 3 or cols < 3:
        # no normals: nothing is fused, a map is only moved
        assert c0 == pr.counts(n_pixels=int((lab == 2).sum())) and c0["n_pixels"] > 0
        surf = jc.plain_surfels(40, seed=rows)
        want, wc, _ = check_fuse(box, surf, z, lab, cam, 2, TURN, rgb, where="moved only")
        assert wc["n_added"] == wc["n_merged"] == 0 and wc["n_out"] == 40 and want.tobytes() == pr.move(surf, TURN).tobytes() != surf.tobytes()
        return
    assert c0["n_added"] == c0["n_candidates"] > 0 and c0["n_voxels"] == 0  # (a pixel per voxel at this distance: all added, in pixel order)
    if rows * cols > 256:
        assert c0["n_pixels"] >= c0["n_candidates"] > 256  # several workgroups add
    # every other surfel of the first sighting, then the surface 2 mm nearer under a small motion: merges, adds and moves
    want, wc, detail = check_fuse(box, first[::2], z - F(0.002), lab, cam, 2, SHIFT, rgb, tick=2, where="second sighting")
    assert wc["n_voxels"] == first[::2].shape[0] and wc["n_merged"] + wc["n_added"] + wc["n_conflict"] <= wc["n_candidates"]
    if rows * cols > 256:
        assert wc["n_merged"] > 20 and wc["n_added"] > 20


def test_qvga_once(box):
    rows, cols = 240, 320
    cam = pc.cam(rows, cols)
    step = bc.motion(rotvec=(0.0, 0.02, 0.01), shift=(0.004, -0.002, 0.003), centre=pc.SPHERE_CENTRE).astype(F)
    z0, m0 = pc.sphere(rows, cols, cam)
    first, c0 = pr.fuse(EMPTY, 1, z0, m0.astype(np.int32), cam, 1)
    centre = step.astype(np.float64)[:3, :3] @ pc.SPHERE_CENTRE + step.astype(np.float64)[:3, 3]
    z1, m1 = pc.sphere(rows, cols, cam, centre)
    want, wc, _ = check_fuse(box, first, z1, m1.astype(np.int32), cam, 1, step, pc.colours(rows, cols), tick=2, where="qvga")
    assert wc["n_merged"] > 1000 and 100 < wc["n_added"] < c0["n_added"] and c0["n_added"] < c0["n_candidates"]


def test_the_second_trip_of_the_scan(box):
    rows, cols = 516, 512  # 1032 blocks of 256 pixels: the scan's second trip begins at block 1024
    assert (rows * cols + 255) // 256 > 1024
    z, cam = pc.plane(rows, cols), pc.cam(rows, cols)
    lab = np.ones((rows, cols), np.int32)
    want, wc, detail = check_fuse(box, EMPTY, z, lab, cam, 1, None, None, pr.params(cell=0.002), tick=1, where="516 x 512")
    assert wc["n_added"] > 200000 and pr.table_slots(0, rows, cols) == 1 << 19
    last = [v + u * rows for v, u in detail["added"][-50:]]
    assert min(last) >= 1024 * 256  # flagged pixels past the first trip get offsets that include it


# ---- 2. map sizes; fusing twice ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def workhorse():
    rows, cols = 60, 80
    z, lab, cam, rgb = scene(rows, cols)
    first, c = pr.fuse(EMPTY, 1, z, lab, cam, 2, None, rgb)
    assert first.shape[0] > 1000
    return z, lab, cam, rgb, first


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_map_sizes_against_the_reference(box, workhorse, n):
    z, lab, cam, rgb, first = workhorse
    want, wc, detail = check_fuse(box, first[:n], z, lab, cam, 2, None, rgb, tick=2, where=n)
    assert wc["n_merged"] == n == wc["n_voxels"] and wc["n_added"] == first.shape[0] - n  # the same frame: every surfel meets its own pixel again
    order = [v + u * 60 for v, u in detail["added"]]
    assert order == sorted(order)
    if n == 0:
        assert want.tobytes() == pr.fuse(EMPTY, 2, z, lab, cam, 2, None, rgb)[0].tobytes()  # first sighting: all added, in pixel order


def test_the_same_frame_fused_twice(box, workhorse):
    z, lab, cam, rgb, first = workhorse
    m = uploaded(box, EMPTY, pose=POSE, tick=1, capacity=room(box, first, 60, 80))
    lc, lp = to_cam(cam), to_p(pr.params())
    c1 = body_maps.fuse([m], [z], [lab], [lc], [2], None, [rgb], lp)[0]
    one = m.download()
    assert one.tobytes() == first.tobytes() and c1["n_added"] == first.shape[0]
    c2 = body_maps.fuse([m], [z], [lab], [lc], [2], None, [rgb], lp)[0]
    two = m.download()
    assert c2["n_added"] == 0 and c2["n_merged"] == c1["n_added"] and c2["n_out"] == c1["n_out"] and m.info()["tick"] == 3
    assert two[:, 0:3].tobytes() == one[:, 0:3].tobytes() and np.all(two[:, 5] == 2) and np.all(two[:, 3] > one[:, 3]) and np.all(two[:, 7] == 2) and np.all(two[:, 6] == 1)
    assert two.tobytes() == pr.fuse(first, 2, z, lab, cam, 2, None, rgb)[0].tobytes()
    m.close()


# ---- 3. the table under pressure -----------------------------------------------------------------------------------------------
def test_a_large_cell_holds_many_pixels(box, workhorse):
    z, lab, cam, rgb, first = workhorse
    p = pr.params(cell=0.5)
    want, wc, _ = check_fuse(box, EMPTY, z, lab, cam, 2, None, rgb, p, tick=1, where="cell 0.5, first")
    assert 0 < wc["n_added"] < 100 and wc["n_candidates"] > 1000  # a few addresses take all the bids
    want2, wc2, _ = check_fuse(box, want, z - F(0.01), lab, cam, 2, SHIFT, rgb, p, tick=2, where="cell 0.5, second")
    assert wc2["n_merged"] + wc2["n_conflict"] > 0 and wc2["n_voxels"] <= wc["n_added"]


def test_colliding_keys_and_a_walk_that_wraps_at_64_slots(box):
    rows, cols = 5, 4
    z, cam = pc.plane(rows, cols), pc.cam(rows, cols)
    lab = np.full((rows, cols), 2, np.int32)
    p = pr.params(cell=jc.CELL)
    has, S = pr.pixel_surfels(z, cam, None, p, F(TICK))
    assert int(has.sum()) == 6
    keys, inside = join_ref.voxel_keys(S[has][:, 0:3], jc.CELL)
    assert inside.all() and len(set(keys.tolist())) == 6
    assert pr.table_slots(26, rows, cols) == 64 == join.table_slots(26 + 6)
    first_slots = sorted(set(join_ref.hash_slot(int(k), 64) for k in keys.tolist()))
    # map surfels whose keys fall on the first slot of a pixel's key (the pixel walks past them), three on the last slot (their
    # walk wraps), and one in a pixel's own voxel; 4 surfels share each of the colliding cells
    cells = jc.cells_on_slot(64, first_slots[0], 3) + jc.cells_on_slot(64, 63, 3, start=5000)
    surf = jc.plain_surfels(25, seed=8)
    surf[:24, 0:3] = np.stack([jc.centre_of(cells[i % 6]) for i in range(24)])
    surf[24] = S[has][2]
    surf[24, 5] = 3
    sk, _ = join_ref.voxel_keys(surf[:, 0:3], jc.CELL)
    assert sorted(join.hash_slot(int(k), 64) for k in set(sk[:24].tolist())) == sorted([first_slots[0]] * 3 + [63] * 3)
    want, wc, _ = check_fuse(box, surf, z, lab, cam, 2, None, None, p, where="colliding keys")
    assert wc["n_voxels"] == 7 and wc["n_merged"] == 1 and wc["n_added"] == 5 and wc["n_out"] == 30


# ---- 4. labels; two entries on one frame -----------------------------------------------------------------------------------------
def test_labels_absent_below_and_above_and_two_entries_on_one_frame(box, workhorse):
    z, lab, cam, rgb, first = workhorse
    assert set(np.unique(lab).tolist()) == {-1, 0, 1, 2, 3}
    surf = first[:100]
    want, wc, _ = check_fuse(box, surf, z, lab, cam, 7, SHIFT, rgb, where="an absent label")
    assert wc == pr.counts(n_voxels=wc["n_voxels"], n_out=100) and want.tobytes() == pr.move(surf, SHIFT).tobytes()
    check_fuse(box, surf, z, lab, cam, 3, None, rgb, where="the highest label")
    # two entries share the frame, with different labels, maps, motions and parameters
    pa, pb = pr.params(), pr.params(cell=0.05, conf_new=0.3, gain=0.5)
    wa, ca = pr.fuse(first[::3], TICK, z, lab, cam, 2, SHIFT, rgb, pa)
    wb, cb = pr.fuse(EMPTY, 9, z, lab, cam, 1, None, rgb, pb)
    ma, mb = uploaded(box, first[::3], tick=TICK, capacity=room(box, first, 60, 80)), uploaded(box, EMPTY, tick=9)
    got = body_maps.fuse([ma, mb], [z, z], [lab, lab], [to_cam(cam)] * 2, [2, 1], [SHIFT, np.eye(4)], [rgb, rgb], [to_p(pa), to_p(pb)])
    assert got == [ca, cb] and ma.download().tobytes() == wa.tobytes() and mb.download().tobytes() == wb.tobytes()
    assert cb["n_added"] > 50 and ca["n_merged"] + ca["n_added"] > 50 and ma.info()["tick"] == TICK + 1 and mb.info()["tick"] == 10
    ma.close()
    mb.close()


# ---- 5. motion ---------------------------------------------------------------------------------------------------------------
def test_translation_rotation_and_the_move_alone(box, workhorse):
    z, lab, cam, rgb, first = workhorse
    surf = pc.special_map(first[:700])
    for W, where in ((SHIFT, "translation"), (TURN, "rotation"), (jc.rigid(3), "a large motion")):
        check_fuse(box, surf, z, lab, cam, 2, W, rgb, exact=False, where=where)
        m = uploaded(box, surf, pose=POSE, tick=TICK)
        before = m.info()
        body_maps.move([m], [W])
        after = m.info()
        assert same_bits32(m.download(), pr.move(surf, W)), where
        assert (after["count"], after["tick"], after["stats"]) == (before["count"], before["tick"], before["stats"]) and np.array_equal(after["pose"], POSE)
        body_maps.move([m])  # the identity, through the same arithmetic
        assert same_bits32(m.download(), pr.move(pr.move(surf, W), None)), where
        m.close()
    # a batch of moves, one map empty
    ms = [uploaded(box, surf[:65]), uploaded(box, EMPTY), uploaded(box, surf[:300])]
    body_maps.move(ms, [TURN, SHIFT, jc.rigid(4)])
    for m, s0, W in zip(ms, (surf[:65], EMPTY, surf[:300]), (TURN, SHIFT, jc.rigid(4))):
        assert same_bits32(m.download(), pr.move(s0, W))
        m.close()


# ---- 6. the normal gate; bad values; the weight cap --------------------------------------------------------------------------
def test_the_normal_gate_met_and_one_ulp_beyond(box):
    rows, cols = 3, 3
    z, cam = pc.plane(rows, cols), pc.cam(rows, cols)
    lab = np.full((rows, cols), 2, np.int32)
    p = pr.params()
    has, S = pr.pixel_surfels(z, cam, None, p, F(TICK))
    assert has.sum() == 1
    surf = S[1, 1][None].copy()
    nrm = np.array([0.3, -0.2, 1.0])
    surf[0, 8:11] = (nrm / np.linalg.norm(nrm)).astype(F)
    d = pr._dot(surf[0, 8:11], S[1, 1, 8:11])
    assert isinstance(d, F) and 0.5 < d < 1
    _, met, _ = check_fuse(box, surf, z, lab, cam, 2, None, None, pr.params(min_dot=float(d)), where="min_dot met")
    _, beyond, _ = check_fuse(box, surf, z, lab, cam, 2, None, None, pr.params(min_dot=float(np.nextafter(d, F(2)))), where="one ulp beyond")
    assert (met["n_merged"], met["n_conflict"]) == (1, 0) and (beyond["n_merged"], beyond["n_conflict"], beyond["n_added"]) == (0, 1, 0)


def test_special_values_and_the_weight_cap(box, workhorse):
    z, lab, cam, rgb, first = workhorse
    surf = pc.special_map(first)
    assert np.isnan(surf[:, 3]).any() and np.isinf(surf[:, 5]).any() and not np.isfinite(surf[:, 0:3]).all()
    want, wc, detail = check_fuse(box, surf, z, lab, cam, 2, None, rgb, exact=False, where="special values")
    assert wc["n_merged"] > 1000 and wc["n_voxels"] < surf.shape[0]  # out-of-grid surfels occupy nothing
    # two surfels in one voxel: the higher confidence is the representative, among equals the lower index
    twin = np.concatenate([first[:50], first[:50]])
    twin[50:75, 3] = F(0.5)
    want, wc, detail = check_fuse(box, twin, z, lab, cam, 2, None, rgb, where="twins")
    assert wc["n_voxels"] == 50 and sorted(detail["merged"]) == list(range(25, 50)) + list(range(50, 75))
    # the weight cap: weights below, at and above max_weight
    heavy = first[:300].copy()
    heavy[:, 5] = np.arange(300) % 7
    shifted = heavy.copy()
    for cap in (1.0, 3.0, 32.0):
        want, wc, _ = check_fuse(box, shifted, z - F(0.001), lab, cam, 2, None, rgb, pr.params(max_weight=cap), where="max_weight %g" % cap)
        assert wc["n_merged"] > 100
    capped = pr.fuse(heavy, TICK, z - F(0.001), lab, cam, 2, None, rgb, pr.params(max_weight=3.0))[0]
    free = pr.fuse(heavy, TICK, z - F(0.001), lab, cam, 2, None, rgb, pr.params(max_weight=32.0))[0]
    assert capped.tobytes() != free.tobytes()


# ---- 7. forms ----------------------------------------------------------------------------------------------------------------
def test_colour_given_and_missing_and_a_batch_against_single_calls(box, workhorse):
    z, lab, cam, rgb, first = workhorse
    grey, cg, _ = check_fuse(box, first[::2], z, lab, cam, 2, SHIFT, None, where="no colour")
    col, cc, _ = check_fuse(box, first[::2], z, lab, cam, 2, SHIFT, rgb, where="colour")
    assert cg == cc and grey[:, 4].tobytes() != col[:, 4].tobytes() and np.all(grey[cg["n_voxels"]:, 4] == F((128 << 16) + (128 << 8) + 128))
    maps0 = [first[::2], EMPTY, first[:65], first[:300]]
    frames = [(z, lab, 2, SHIFT, rgb), (z - F(0.002), lab, 2, None, None), (z, lab, 1, TURN, rgb), (z, lab, 3, None, None)]
    ps = [pr.params(), pr.params(cell=0.02), pr.params(min_dot=0.99), pr.params(gain=1.0, conf_new=0.0)]
    want = [pr.fuse(s0, TICK, f[0], f[1], cam, f[2], np.eye(4, dtype=F) if f[3] is None else f[3], f[4], p) for s0, f, p in zip(maps0, frames, ps)]
    results = []
    for batched in (True, False):
        ms = [uploaded(box, s0, tick=TICK, capacity=room(box, s0, 60, 80)) for s0 in maps0]
        Ws = [np.eye(4, dtype=F) if f[3] is None else f[3] for f in frames]
        if batched:
            got = body_maps.fuse(ms, [f[0] for f in frames], [f[1] for f in frames], [to_cam(cam)] * 4, [f[2] for f in frames], Ws, [f[4] for f in frames],
                                 [to_p(p) for p in ps])
        else:
            got = [body_maps.fuse([m], [f[0]], [f[1]], [to_cam(cam)], [f[2]], [W], [f[4]], to_p(p))[0] for m, f, W, p in zip(ms, frames, Ws, ps)]
        assert got == [w[1] for w in want], batched
        results.append([m.download() for m in ms])
        for m in ms:
            m.close()
    for q in range(4):
        assert results[0][q].tobytes() == want[q][0].tobytes() == results[1][q].tobytes(), q


def test_host_form_equals_device_form(box, workhorse):
    z, lab, cam, rgb, first = workhorse
    rt = hip_runtime()
    blocks = []

    def dev(a):
        p = C.c_void_p()
        assert rt.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
        blocks.append(p)
        assert rt.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
        return p.value

    col = lambda a, t: np.ascontiguousarray(np.asarray(a, t).T)  # noqa: E731
    dz, dl, dc = dev(col(z, F)), dev(col(lab, np.int32)), dev(np.ascontiguousarray(rgb))
    want = [pr.fuse(first[::2], TICK, z, lab, cam, 2, SHIFT, rgb), pr.fuse(first[:65], TICK, z, lab, cam, 1, None, None)]
    ms = [uploaded(box, first[::2], tick=TICK, capacity=room(box, first, 60, 80)), uploaded(box, first[:65], tick=TICK, capacity=room(box, first, 60, 80))]
    b = body_maps._bind(box.api)
    out = (body_maps.SfpCounts * 3)()
    C.memset(out, 0xFB, C.sizeof(out))  # a sentinel past the end of the counts
    sentinel = bytes(out)[64:]
    Ws = np.ascontiguousarray(np.stack([SHIFT.T, np.eye(4, dtype=F)])).reshape(-1)
    code = b.fuse_images_device(box.h, 60, 80, 2, (C.c_void_p * 2)(dz, dz), (C.c_void_p * 2)(dl, dl), (C.c_void_p * 2)(dc, None),
                                (body_maps.SfpCamera * 2)(to_cam(cam), to_cam(cam)), (C.c_int32 * 2)(2, 1), (C.c_void_p * 2)(ms[0].m.value, ms[1].m.value),
                                Ws.ctypes.data_as(_fp), (body_maps.SfpParams * 2)(to_p(pr.params()), to_p(pr.params())), out)
    assert code == 0 and [out[0].as_dict(), out[1].as_dict()] == [w[1] for w in want] and bytes(out)[64:] == sentinel
    assert out[0].reserved == 0 and out[1].reserved == 0
    for m, w in zip(ms, want):
        assert m.download().tobytes() == w[0].tobytes() and m.info()["tick"] == TICK + 1
        m.close()
    # the wrapper, one entry, on the same device frame
    m = uploaded(box, first[::2], tick=TICK, capacity=room(box, first, 60, 80))
    assert body_maps.fuse_device([m], 60, 80, [dz], [dl], [to_cam(cam)], [2], [SHIFT], [dc]) == [want[0][1]] and m.download().tobytes() == want[0][0].tobytes()
    m.close()
    for p in blocks:
        rt.hipFree(p)


# ---- 8. capacity -------------------------------------------------------------------------------------------------------------
def test_the_capacity_exceeded_in_one_entry_changes_no_map(hip_auto):
    s = small_solver(hip_auto, 30, 40)
    cap = s.rows * s.cols
    rows, cols = 30, 40
    z, lab, cam, rgb = scene(rows, cols)
    first, c0 = pr.fuse(EMPTY, 1, z, lab, cam, 2, None, rgb)
    n_new = c0["n_added"]
    assert 100 < n_new < cap
    far = jc.plain_surfels(cap - n_new + 1, seed=54)
    far[:, 0] += 50.0
    ok_map, full = uploaded(s, first[::2], pose=POSE, tick=TICK, capacity=cap), uploaded(s, far, pose=POSE, tick=TICK, capacity=cap)
    before = state(ok_map), state(full)
    b = body_maps._bind(s.api)
    out = (body_maps.SfpCounts * 2)()
    keep = [np.ascontiguousarray(z.T), np.ascontiguousarray(lab.T)]
    two = lambda a: (C.c_void_p * 2)(a.ctypes.data, a.ctypes.data)  # noqa: E731
    Ws = np.ascontiguousarray(np.stack([SHIFT.T, SHIFT.T])).reshape(-1)
    args = (s.h, rows, cols, 2, two(keep[0]), two(keep[1]), None, (body_maps.SfpCamera * 2)(to_cam(cam), to_cam(cam)), (C.c_int32 * 2)(2, 2),
            (C.c_void_p * 2)(ok_map.m.value, full.m.value), Ws.ctypes.data_as(_fp), (body_maps.SfpParams * 2)(to_p(pr.params()), to_p(pr.params())), out)
    assert b.fuse_images(*args) == -3  # SF_ERR_STATE: the second entry does not fit
    assert b"capacity" in s.api.last_error()
    assert (state(ok_map), state(full)) == before  # not even the move
    want_ok, want_full = pr.fuse(first[::2], TICK, z, lab, cam, 2, SHIFT)[1], pr.fuse(far, TICK, z, lab, cam, 2, SHIFT)[1]
    assert [out[0].as_dict(), out[1].as_dict()] == [want_ok, want_full] and want_full["n_added"] == n_new and want_full["n_out"] == cap + 1
    with pytest.raises(SfError, match="capacity"):
        body_maps.fuse([full], [z], [lab], [to_cam(cam)], [2], [SHIFT])
    assert state(full) == before[1]
    full.upload(far[:-1], POSE, TICK)  # one surfel fewer: exactly the capacity
    assert body_maps.fuse([full], [z], [lab], [to_cam(cam)], [2], [SHIFT])[0]["n_out"] == cap == full.info()["count"]
    assert full.download().tobytes() == pr.fuse(far[:-1], TICK, z, lab, cam, 2, SHIFT)[0].tobytes()
    for m in (ok_map, full):
        m.close()
    s.close()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(box, hip_auto, workhorse):
    z, lab, cam, rgb, first = workhorse
    s = box
    b = body_maps._bind(s.api)
    rows, cols = 60, 80
    m1, m2 = uploaded(s, first[:300], pose=POSE, tick=TICK, capacity=room(s, first, rows, cols)), uploaded(s, first[:65], pose=POSE, tick=TICK)
    other = small_solver(hip_auto, 60, 80)
    mo = uploaded(other, first[:65], pose=POSE, tick=TICK)
    before = [state(m) for m in (m1, m2, mo)]
    keep = [np.ascontiguousarray(z.T), np.ascontiguousarray(lab.T), np.ascontiguousarray(rgb)]
    two = lambda a: (C.c_void_p * 2)(a.ctypes.data, a.ctypes.data)  # noqa: E731
    arr = lambda *ms: (C.c_void_p * len(ms))(*[None if m is None else m.m.value for m in ms])  # noqa: E731
    with_null = lambda a: (C.c_void_p * 2)(a.ctypes.data, None)  # noqa: E731
    nan, inf = float("nan"), float("inf")
    out = (body_maps.SfpCounts * 2)()
    C.memset(out, 0xFB, C.sizeof(out))  # a sentinel in every field
    sentinel = bytes(out)
    w_ok = np.tile(np.eye(4, dtype=F).reshape(-1), 2)

    def w_with(v):
        w = w_ok.copy()
        w[16 + 13] = v
        return w.ctypes.data_as(_fp), w  # (the array travels with its pointer: it stays alive)

    holders = [w_with(nan), w_with(inf), w_with(-inf)]
    cams = lambda **kw: (body_maps.SfpCamera * 2)(to_cam(cam), to_cam(dict(cam, **kw)))  # noqa: E731
    pars = lambda **kw: (body_maps.SfpParams * 2)(to_p(pr.params()), to_p(pr.params(**kw)))  # noqa: E731
    bad_pose = np.eye(4, dtype=F)
    bad_pose[1, 3] = nan
    good = dict(h=s.h, rows=rows, cols=cols, n=2, z=two(keep[0]), lab=two(keep[1]), rgb=two(keep[2]), cams=cams(), t=(C.c_int32 * 2)(2, 1), maps=arr(m1, m2),
                W=w_ok.ctypes.data_as(_fp), p=pars(), out=out)
    order = ("h", "rows", "cols", "n", "z", "lab", "rgb", "cams", "t", "maps", "W", "p", "out")
    overs = [dict(h=None), dict(n=-1), dict(n=65536), dict(rows=0), dict(cols=0), dict(rows=4097), dict(rows=4096, cols=4097), dict(z=None), dict(lab=None),
             dict(cams=None), dict(t=None), dict(maps=None), dict(p=None), dict(out=None), dict(z=with_null(keep[0])), dict(lab=with_null(keep[1])),
             dict(t=(C.c_int32 * 2)(2, 0)), dict(t=(C.c_int32 * 2)(-1, 1)), dict(maps=arr(m1, mo)), dict(maps=arr(m1, m1)), dict(maps=arr(m1, None)), dict(h=other.h),
             dict(cams=cams(fx=0.0)), dict(cams=cams(fy=0.0)), dict(cams=cams(cx=nan)), dict(cams=cams(fy=inf)), dict(cams=cams(pose=bad_pose)),
             dict(W=holders[0][0]), dict(W=holders[1][0]), dict(W=holders[2][0]),
             dict(p=pars(cell=0.0)), dict(p=pars(cell=nan)), dict(p=pars(cell=1e-45)), dict(p=pars(cell=-1.0)), dict(p=pars(z_max=0.0)), dict(p=pars(z_max=33.0)),
             dict(p=pars(normal_dz=0.0)), dict(p=pars(normal_dz=inf)), dict(p=pars(min_dot=1.5)), dict(p=pars(min_dot=-1.5)), dict(p=pars(conf_new=-0.1)),
             dict(p=pars(conf_new=1.5)), dict(p=pars(gain=0.0)), dict(p=pars(gain=1.5)), dict(p=pars(max_weight=0.5)), dict(p=pars(max_weight=nan))]
    for fn in (b.fuse_images, b.fuse_images_device):  # (the device form refuses before it looks at a pointer's target)
        for q, over in enumerate(overs):
            a = dict(good, **over)
            assert fn(*[a[k] for k in order]) == -1, (q, list(over))
            assert s.api.last_error(), q
        assert fn(s.h, rows, cols, 0, None, None, None, None, None, None, None, None, None) == 0  # an empty batch is fine
        assert fn(None, rows, cols, 0, None, None, None, None, None, None, None, None, None) == -1
    move_cases = [(None, 2, arr(m1, m2), None), (s.h, -1, arr(m1, m2), None), (s.h, 65536, arr(m1, m2), None), (s.h, 2, None, None), (s.h, 2, arr(m1, mo), None),
                  (s.h, 2, arr(m1, m1), None), (s.h, 2, arr(m1, None), None), (other.h, 2, arr(m1, m2), None), (s.h, 2, arr(m1, m2), holders[0][0]),
                  (s.h, 2, arr(m1, m2), holders[1][0])]
    for q, args in enumerate(move_cases):
        assert b.move_maps(*args) == -1, q
    assert b.move_maps(s.h, 0, None, None) == 0
    # colour may be missing altogether or in single entries; W may be missing
    assert bytes(out) == sentinel and [state(m) for m in (m1, m2, mo)] == before
    with pytest.raises(SfError):
        body_maps.fuse([m1, mo], [z, z], [lab, lab], [to_cam(cam)] * 2, [2, 2])  # maps of two solvers
    with pytest.raises(SfError):
        body_maps.fuse([m1], [z], [lab[:, :-1]], [to_cam(cam)], [2])
    with pytest.raises(SfError):
        body_maps.fuse([m1], [z], [lab], [to_cam(cam)], [2], params=to_p(pr.params(gain=nan)))
    assert [state(m) for m in (m1, m2, mo)] == before
    # the handle goes first: its map is an empty shell that fails cleanly
    other.close()
    a = dict(good, n=1, maps=arr(mo))
    assert b.fuse_images(*[a[k] for k in order]) == -3 and b.move_maps(s.h, 1, arr(mo), None) == -3  # SF_ERR_STATE
    assert bytes(out) == sentinel and [state(m) for m in (m1, m2)] == before[:2]
    # and the live maps still work, with colour missing in one entry and W missing
    a = dict(good, rgb=with_null(keep[2]), W=None)
    assert b.fuse_images(*[a[k] for k in order]) == 0
    want = [pr.fuse(first[:300], TICK, z, lab, cam, 2, None, rgb), pr.fuse(first[:65], TICK, z, lab, cam, 1, None, None)]
    assert [out[0].as_dict(), out[1].as_dict()] == [w[1] for w in want]
    assert m1.download().tobytes() == want[0][0].tobytes() and m2.download().tobytes() == want[1][0].tobytes()
    for m in (m1, m2, mo):
        m.close()


# ---- 10. what a call leaves alone; the calls that take a fused map afterwards ------------------------------------------------
@pytest.fixture(scope="module")
def walked(hip_auto):
    s, m, out = walk(hip_auto, 5, render_between=False)
    yield s, m, out
    m.close()
    s.close()


def test_a_call_leaves_everything_else_alone_and_a_fused_map_serves_the_other_calls(walked, workhorse):
    s, m, out = walked
    z, lab, cam, rgb, first = workhorse
    SurfelMap.predict_frames(s, [0], [m], s.default_model_params())
    v = view.default_view(s, m)
    db = keyframes.KeyframeDb(s, 10, n_ferns=64)
    db.add_streams([0], [np.eye(4)], [0])
    uninvolved = uploaded(s, first[:300], pose=POSE, tick=TICK)

    def readable():
        i = m.info()
        sc_ = score.score_streams([m], [v], [0])
        summ, reg = regions.label_streams(s, [0])
        res = align.refine_streams([m], [v], [0], align.Params(iterations=2))
        return (i["count"], i["tick"], i["pose"].tobytes(), tuple(i["stats"]), m.download().tobytes(), m.index_map().tobytes(),
                s.prediction()[0].tobytes(), s.prediction()[1].tobytes(), s.prediction_dense_stream(0), s.current(0)[0].tobytes(), s.b_image(0).tobytes(),
                sc_.tobytes(), db.query_streams([0]).tobytes(), db.encode_streams([0]).tobytes(), summ.tobytes(), res.tobytes(),
                repr(join.thin([m], join.Params(dry_run=True))), state(uninvolved))

    before = readable()
    body = uploaded(s, EMPTY, tick=1, capacity=room(s, first, 240, 320))
    assert body_maps.fuse([body], [z], [lab], [to_cam(cam)], [2], None, [rgb])[0] == pr.fuse(EMPTY, 1, z, lab, cam, 2, None, rgb)[1]
    assert readable() == before
    # a larger call grows the scratch
    zq, mq = pc.sphere(240, 320, pc.cam(240, 320))
    big = uploaded(s, EMPTY, tick=1, capacity=240 * 320)
    body_maps.fuse([big, body], [zq, zq], [mq.astype(np.int32)] * 2, [to_cam(pc.cam(240, 320))] * 2, [1, 7])
    body_maps.move([body], [TURN])
    assert readable() == before
    # the fused map is a map like any other: a view, a score, a refinement, a thin, a prediction, a fuse of the static pipeline
    own = view.default_view(s, big)
    images = view.render([big], [own])
    assert images is not None
    assert score.score_streams([big], [own], [0]) is not None and align.refine_streams([big], [own], [0], align.Params(iterations=2)) is not None
    n_before = big.info()["count"]
    kept = join.thin([big], join.Params(cell=0.02))[0]
    assert 0 < kept["n_out"] <= kept["n_in"] == n_before and big.info()["count"] == kept["n_out"]
    with pytest.raises(SfError, match="index map"):
        big.index_map()
    big.predict(0)
    for x in (body, big, uninvolved):
        x.close()
    db.close()


# ---- 11. a destroyed handle; the other libraries ---------------------------------------------------------------------------------
def test_a_call_after_sf_destroy_is_refused(hip_auto, workhorse):
    z, lab, cam, rgb, first = workhorse
    s = small_solver(hip_auto, 60, 80)
    m = uploaded(s, first[:65], tick=TICK)
    assert body_maps.fuse([m], [z], [lab], [to_cam(cam)], [2])[0]["n_merged"] == 65
    b = body_maps._bind(hip_auto)
    gone, shell = C.c_void_p(s.h.value), C.c_void_p(m.m.value)
    s.close()
    keep = [np.ascontiguousarray(z.T), np.ascontiguousarray(lab.T)]
    out = (body_maps.SfpCounts * 1)()
    C.memset(out, 0xFB, C.sizeof(out))
    sentinel = bytes(out)
    one = lambda a: (C.c_void_p * 1)(a.ctypes.data)  # noqa: E731
    args = (gone, 60, 80, 1, one(keep[0]), one(keep[1]), None, (body_maps.SfpCamera * 1)(to_cam(cam)), (C.c_int32 * 1)(2), (C.c_void_p * 1)(shell.value), None,
            (body_maps.SfpParams * 1)(to_p(pr.params())), out)
    assert b.fuse_images(*args) == -3 and b.fuse_images_device(*args) == -3 and bytes(out) == sentinel  # SF_ERR_STATE
    assert b.move_maps(gone, 1, (C.c_void_p * 1)(shell.value), None) == -3
    assert b.fuse_images(gone, 60, 80, 0, None, None, None, None, None, None, None, None, None) == -3
    m.close()
    s2 = small_solver(hip_auto, 60, 80)  # (a new handle, at the old address or another: alive)
    m2 = uploaded(s2, first[:65], tick=TICK)
    assert body_maps.fuse([m2], [z], [lab], [to_cam(cam)], [2])[0]["n_merged"] == 65
    m2.close()
    s2.close()


@pytest.mark.parametrize("lib", ["libsf_hip_precise.so", "libsf_hip_reforder.so"])
def test_the_precise_and_reference_order_libraries_fuse_the_same(lib, workhorse):
    import staticfusion_amd as sf

    z, lab, cam, rgb, first = workhorse
    api = sf.Api(os.path.join(os.path.dirname(sf.LIB), lib), "sf_")
    s = small_solver(api, 60, 80)
    want, wc, _ = check_fuse(s, pc.special_map(first[::2]), z - F(0.002), lab, cam, 2, SHIFT, rgb, exact=False, where=lib)
    assert wc["n_merged"] > 100 and wc["n_added"] > 100
    s.close()
