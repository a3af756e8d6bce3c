"""Region tracks (include/sf_tracks.h), the pure-host functions against tests/track_ref.py, bit for bit and integer for
integer, and the premises the GPU tests rest on, checked on the reference alone. No GPU."""
import numpy as np
import pytest

import track_cases as tc
import track_ref as tr
from staticfusion_amd import SfError, tracks
from staticfusion_amd.synth import LCG64

F = np.float32


def pose_of(g, scale=1.0):
    T = tc.rot(0, g.uniform(-3, 3)) @ tc.rot(1, g.uniform(-3, 3)) @ tc.rot(2, g.uniform(-3, 3))
    T[:3, 3] = [g.uniform(-5, 5) * scale for _ in range(3)]
    return T.astype(F)


def same_relative(p0, p1):
    got, want = tracks.relative(p0, p1), tr.relative(p0, p1)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (got, want)
    return got


def test_relative_equals_the_reference_bit_for_bit():
    eye = np.eye(4, dtype=F)
    assert same_relative(eye, eye).tobytes() == eye.tobytes()
    d = same_relative(tc.shift(0.25, -1.5, 3.0), tc.shift(1.0, 0.5, -2.0))
    assert d[:3, :3].tobytes() == eye[:3, :3].tobytes() and d[:3, 3].tolist() == [-0.75, -2.0, 5.0] and d[3].tolist() == [0, 0, 0, 1]
    for axis in range(3):
        d = same_relative(eye, tc.rot(axis, 0.3))
        assert d.tobytes() != eye.tobytes() and np.allclose(d, tc.rot(axis, -0.3), atol=1e-7)
        same_relative(tc.rot(axis, 0.3), eye)
        p = (tc.shift(0.1, 0.2, 0.3) @ tc.rot(axis, 0.3)).astype(F)
        assert same_relative(p, p).tobytes() == eye.tobytes()  # equal poses: the exact identity
    g = LCG64(20261020)
    for _ in range(1000):
        p0, p1 = pose_of(g), pose_of(g, 10.0)
        d = same_relative(p0, p1)
        assert np.allclose(d.astype(np.float64), np.linalg.inv(p1.astype(np.float64)) @ p0.astype(np.float64), atol=2e-5)
    bad = eye.copy()
    bad[2, 1] = np.nan
    for a, b in ((bad, eye), (eye, bad)):
        assert tr.relative(a, b) is None
        with pytest.raises(SfError, match="failed with -1"):
            tracks.relative(a, b)
    bad[2, 1] = np.inf
    with pytest.raises(SfError, match="failed with -1"):
        tracks.relative(eye, bad)


def both_assign(O, n_prev, n_cur, min_overlap=1, min_share=256):
    got, want = tracks.assign(O, n_prev, n_cur, min_overlap, min_share), tr.assign(O, n_prev, n_cur, min_overlap, min_share)
    assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist() and got[2] == want[2], (got, want)
    return got[0].tolist(), got[1].tolist(), got[2]


def test_assign_on_hand_tables():
    # a split: the larger overlap keeps the id
    assert both_assign([[30, 50]], [100], [35, 60]) == ([0, 1], [2], 1)
    # a merge
    assert both_assign([[40], [25]], [40, 25], [70]) == ([1], [1, 0], 1)
    # equal overlaps: t ascending, then k ascending
    assert both_assign([[5, 5], [5, 5]], [10, 10], [10, 10]) == ([1, 2], [1, 2], 2)
    assert both_assign([[0, 5], [5, 5]], [10, 10], [10, 10]) == ([2, 1], [2, 1], 2)
    assert both_assign([[5, 5, 5]], [10], [10, 10, 10]) == ([1, 0, 0], [1], 1)
    # min_overlap met exactly and one below
    assert both_assign([[4]], [4], [4], min_overlap=4) == ([1], [1], 1)
    assert both_assign([[4]], [4], [4], min_overlap=5) == ([0], [0], 0)
    # min_share at equality (1024 * 25 == 256 * 100) and one pixel below
    assert both_assign([[25]], [100], [200]) == ([1], [1], 1) and both_assign([[25]], [200], [100]) == ([1], [1], 1)
    assert both_assign([[24]], [100], [200]) == ([0], [0], 0)
    assert both_assign([[1]], [100], [200], min_share=0) == ([1], [1], 1) and both_assign([[99]], [100], [200], min_share=1024) == ([0], [0], 0)
    # int64: the products pass 2^31
    assert both_assign([[2 ** 24]], [2 ** 24], [2 ** 24], min_share=1024) == ([1], [1], 1)
    # an empty table, on either side and both
    assert both_assign(np.zeros((0, 3)), [], [7, 7, 7]) == ([0, 0, 0], [], 0)
    assert both_assign(np.zeros((3, 0)), [7, 7, 7], []) == ([], [0, 0, 0], 0) and both_assign(np.zeros((0, 0)), [], []) == ([], [], 0)
    assert both_assign(np.zeros((2, 2)), [7, 7], [7, 7]) == ([0, 0], [0, 0], 0)
    # one track against 256 regions: the first of the largest
    row = [(c * 37) % 101 + 1 for c in range(256)]
    best = row.index(max(row))
    poc, cop, n = both_assign([row], [1000], [1000] * 256, min_share=0)
    assert n == 1 and cop == [best + 1] and poc == [1 if c == best else 0 for c in range(256)]
    # 256 against 256 with a permutation on the diagonal
    perm = [(t * 77 + 5) % 256 for t in range(256)]
    assert sorted(perm) == list(range(256))
    O = np.zeros((256, 256), np.int32)
    O[np.arange(256), perm] = 10
    poc, cop, n = both_assign(O, [10] * 256, [10] * 256)
    assert n == 256 and cop == [p + 1 for p in perm] and [poc[perm[t]] for t in range(256)] == list(range(1, 257))
    b = tracks._product()
    assert b.assign(257, 1, None, None, None, 1, 256, None, None, None) == -1 and b.assign(1, -1, None, None, None, 1, 256, None, None, None) == -1
    one = (np.ones(1, np.int32)).ctypes.data_as(tracks._ip)
    assert b.assign(1, 1, one, one, one, 0, 256, one, None, None) == -1 and b.assign(1, 1, one, one, one, 1, 1025, one, None, None) == -1
    assert b.assign(1, 1, None, one, one, 1, 256, one, None, None) == -1


def test_assign_on_random_tables():
    g = LCG64(77)
    for _ in range(2000):
        kp, k = int(g.uniform(0, 9)), int(g.uniform(0, 9))
        O = np.array([[int(g.uniform(0, 6)) for _ in range(k)] for _ in range(kp)], np.int32).reshape(kp, k)
        n_prev, n_cur = [int(g.uniform(1, 24)) for _ in range(kp)], [int(g.uniform(1, 24)) for _ in range(k)]
        poc, cop, n = both_assign(O, n_prev, n_cur, int(g.uniform(1, 4)), int(g.uniform(0, 1025)))
        assert n == sum(1 for x in poc if x) == sum(1 for x in cop if x) and all(cop[t - 1] == c + 1 for c, t in enumerate(poc) if t)


# ---- premises, on the reference alone ------------------------------------------------------------------------------------------
def test_a_frame_against_itself_matches_every_region_to_itself():
    rows, cols = 60, 80
    for name in ("identical", "five"):
        steps = tc.cases_of(rows, cols)[name]
        slot = tr.Slot()
        first, second = [tr.update(slot, *s, 8) for s in steps]
        k = int(first[0]["n_tracked"])
        assert k >= 2 and int(second[0]["n_matched"]) == k and second[1]["id"][:k].tolist() == first[1]["id"][:k].tolist() == list(range(1, k + 1))
        assert second[1]["overlap"][:k].tolist() == second[1]["n"][:k].tolist() and second[1]["prev_region"][:k].tolist() == list(range(1, k + 1))
        assert second[1]["age"][:k].tolist() == [1] * k and int(second[0]["n_warped"]) == int(first[1]["n"][:k].sum())
        assert np.array_equal(second[2], first[2])


def test_a_camera_translation_of_three_pixels():
    rows, cols = 60, 80
    fx = tc.intrinsics(rows, cols)["fx"]
    moved_cam = tc.cam(rows, cols, tc.shift(x=3 * 2.0 / fx))
    # a rectangle that stays inside the image, and one at the left edge that loses three columns
    for u0, lost in ((10, 0), (0, 3)):
        prev = tc.rects(rows, cols, [(10, 40, u0, u0 + 20, 2.0)])
        cur = tc.rects(rows, cols, [(10, 40, u0 - 3, u0 + 17, 2.0)])
        slot = tr.Slot()
        tr.update(slot, *tc.step(prev, tc.cam(rows, cols)), 8)
        summ, rec, ids, O = tr.update(slot, *tc.step(cur, moved_cam), 8)
        n_prev = 30 * 20
        assert int(summ["n_matched"]) == 1 and int(rec["id"][0]) == 1 and int(rec["overlap"][0]) == n_prev - 30 * lost == int(summ["n_warped"])
        assert int(rec["n"][0]) == 30 * (20 - lost)
    # the world box does not move with the camera: the same points, seen from two places, to the quantum
    slot = tr.Slot()
    a = tr.update(slot, *tc.step(tc.rects(rows, cols, [(10, 40, 10, 30, 2.0)]), tc.cam(rows, cols)), 8)
    b = tr.update(slot, *tc.step(tc.rects(rows, cols, [(10, 40, 7, 27, 2.0)]), moved_cam), 8)
    assert np.abs(a[1]["qmin"][0] - b[1]["qmin"][0]).max() <= 1 and np.abs(a[1]["sum_q"][0] - b[1]["sum_q"][0]).max() <= 600


def test_the_round_trip_lands_on_its_own_pixel_at_qvga():
    rows, cols = 240, 320
    v, u = [a.ravel() for a in np.indices((rows, cols))]
    c0 = tc.cam(rows, cols)
    z = np.full(rows * cols, 2.0, F)
    kept, vi, ui, hz = tr.warp(np.eye(4, dtype=F), c0, c0, v, u, z, rows, cols)
    assert kept.all() and np.array_equal(vi, v) and np.array_equal(ui, u) and (hz == F(2)).all()
    D = tr.relative(np.eye(4, dtype=F), tc.shift(x=3 * 2.0 / c0["fx"]).astype(F))
    kept, vi, ui, _ = tr.warp(D, c0, c0, v, u, z, rows, cols)
    assert np.array_equal(kept, u >= 3) and np.array_equal(ui[kept], u[kept] - 3) and np.array_equal(vi[kept], v[kept])


def test_centroids_and_velocities():
    slot = tr.Slot()
    rows, cols = 60, 80
    a = tr.update(slot, *tc.step(tc.moved(rows, cols, 0), tc.cam(rows, cols)), 4)[1][:1]
    b = tr.update(slot, *tc.step(tc.moved(rows, cols, 4), tc.cam(rows, cols)), 4)[1][:1]
    ca, cb = tracks.centroids(a), tracks.centroids(b)
    assert ca.shape == (1, 3) and abs(ca[0, 2] - 2.0) < 1e-3 and abs((cb - ca)[0, 0] - 4 * 2.0 / 80) < 2e-3
    vel = tracks.velocities(a, b, 0.5)
    assert list(vel) == [1] and np.allclose(vel[1], (cb - ca)[0] / 0.5)
    assert tracks.centroids(np.zeros(2, tracks.TRACK_DTYPE)).tolist() == [[0, 0, 0]] * 2
