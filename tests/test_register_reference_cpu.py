"""The restatement of the map registration (tests/register_ref.py) on the corner scene of tests/register_cases.py, before any
device runs: the conditions that keep the scene meaningful. From the identity, with the default parameters, the loop recovers
the scene's motion; a start ten times further away pairs nothing; a single plane leaves the system singular without damping and
solvable with it. These are conditions on the scene and the rule, not tolerances on the device: the device is held to the
restatement bit for bit elsewhere."""
import numpy as np

import register_cases as rc
import register_ref as rr


def test_the_scene_is_what_the_cases_say():
    dst, src, R, t = rc.corner()
    assert dst.shape == (1587, 12) and 1587 % 64 == 51 and src.shape == (529, 12)
    assert len(set(dst[:, 3].tolist())) == 1587  # distinct confidences: every voxel has one representative whatever the order
    for k in range(3):  # plane k is perpendicular to axis k and passes through the corner
        plane = dst[529 * k:529 * (k + 1)]
        assert (plane[:, k] == np.float32(rc.CORNER[k])).all() and (plane[:, 8 + k] == 1).all() and np.abs(plane[:, 8:11]).sum() == 529
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and np.linalg.det(R) > 0
    back = src[:, 0:3].astype(np.float64) @ R.T + t  # E = [R t] puts the source back onto every third surfel of the reversed destination
    assert np.abs(back - dst[::-1][::3][:, 0:3]).max() < 2e-7


def test_the_loop_recovers_the_motion_of_the_scene():
    dst, src, R, t = rc.corner()
    res, systems, pairs, E = rr.register(dst, src)
    err = rc.estimate_error(E, R, t)
    print("pairs first %d last %d, max|E - [R t]| = %.3g" % (res["n_first"], res["n_last"], err))
    assert res["status"] == rr.OK and res["iterations_done"] == 10 and res["n_sampled"] == 529 and res["n_outside"] == 0
    assert err <= 1e-4
    assert res["n_last"] >= res["n_first"] >= 64 and (systems[:, 0] > 0).all() and int((pairs >= 0).sum()) == res["n_last"]
    assert res["ss_last"] * res["n_first"] < res["ss_first"] * res["n_last"]  # the mean squared residual went down
    assert np.array_equal(res["T"].reshape(4, 4).T[:3], np.array(E, np.float64).reshape(3, 4).astype(np.float32)) and list(res["T"][3::4]) == [0, 0, 0, 1]


def test_a_finer_table_from_half_the_motion():
    dst, src, R, t = rc.corner()
    res, _, _, E = rr.register(dst, src, T0=rc.as_matrix(*rc.motion(0.5)), params=rr.Params(cell=0.05, dist_max=0.025))
    assert res["status"] == rr.OK and rc.estimate_error(E, R, t) <= 1e-4


def test_a_start_ten_times_further_away_pairs_nothing():
    dst, _, _, _ = rc.corner()
    R, t = rc.motion(1.0, 10.0)
    res, systems, pairs, _ = rr.register(dst, rc.moved_by_inverse(dst[::-1][::3], R, t))
    assert res["status"] == rr.FEW_PAIRS and res["iterations_done"] == 0 and res["n_first"] == res["n_last"] == 0
    assert (systems == 0).all() and (pairs == rr.NOT_PAIRED).all() and np.array_equal(res["T"], np.eye(4, dtype=np.float32).ravel())


def test_a_single_plane_is_degenerate_without_damping_and_runs_with_it():
    dst, src, _, _ = rc.corner(axes=(2,))
    assert dst.shape[0] == 529 and src.shape[0] == 177
    res, systems, _, _ = rr.register(dst, src)
    assert res["status"] == rr.DEGENERATE and res["iterations_done"] == 0 and res["n_first"] >= 64 and (systems[1:] == 0).all()
    res, systems, _, _ = rr.register(dst, src, params=rr.Params(damping=1e-3))
    assert res["status"] == rr.OK and res["iterations_done"] == 10 and (systems[:, 0] >= 64).all()
