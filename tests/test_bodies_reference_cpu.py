"""Region motion (include/sf_bodies.h) without a GPU: the pure-host sfb_world_motion against the restatement of tests/body_ref.py
bit for bit, and the premises of the method on the restatement alone -- a pyramid that did not move under a camera that moved
stays where the "did not move" hypothesis puts it, and the moved pyramid of tests/body_cases.py is found."""
import numpy as np
import pytest

import body_cases as bc
import body_ref as br
import track_ref as tr


def rms_mm(n, ss):
    return 1000.0 * np.sqrt(float(ss) / max(int(n), 1)) / 65536.0


# ---- sfb_world_motion ------------------------------------------------------------------------------------------------------
def both(pose0, pose1, D):
    from staticfusion_amd import bodies

    got = bodies.world_motion(pose0, pose1, D)
    ref = br.world_motion(pose0, pose1, D)
    assert got.dtype == np.float32 and got.T.ravel().tobytes() == ref.tobytes(), (got, ref.reshape(4, 4).T)
    return got


def rows12(T):
    return [float(x) for x in np.asarray(T, np.float64)[:3, :].ravel()]


def test_world_motion_hand_cases_bit_for_bit():
    I = np.eye(4)
    assert both(I, I, rows12(I)).tobytes() == np.eye(4, dtype=np.float32).tobytes()
    shift = bc.pose(shift=(0.25, -0.5, 2.0))
    assert both(I, I, rows12(shift)).tobytes() == shift.astype(np.float32).tobytes()  # a pure translation, exactly
    for axis in range(3):
        w = np.zeros(3)
        w[axis] = 0.3
        turn = bc.pose(w, (0.1, -0.2, 0.05))
        got = both(I, I, rows12(turn))
        assert np.abs(got - turn).max() < 1e-7
        # the same body motion seen by a camera that moved: D = T1^-1 W T0 gives W back
        T0, T1 = bc.MOVING_CAMERA
        D = np.linalg.inv(T1.astype(np.float32).astype(np.float64)) @ turn @ T0.astype(np.float32).astype(np.float64)
        assert np.abs(both(T0, T1, rows12(D)) - turn).max() < 1e-6
        # and a body that did not move: W = I to the rounding of the poses
        D = tr.relative(T0, T1)
        assert np.abs(both(T0, T1, rows12(D)) - I).max() < 1e-6


def test_world_motion_seeded_triples_bit_for_bit():
    from staticfusion_amd.synth import LCG64

    g = LCG64(20261020)
    for _ in range(1000):
        T0, T1, D = (bc.pose([g.uniform(-3, 3) for _ in range(3)], [g.uniform(-5, 5) for _ in range(3)]) for _ in range(3))
        D = D + np.array([[g.uniform(-1e-3, 1e-3) for _ in range(4)] for _ in range(4)])  # (an estimate is not exactly rigid)
        both(T0, T1, rows12(D))


def test_world_motion_refuses_nan_and_inf():
    from staticfusion_amd import SfError, bodies

    I = np.eye(4)
    for bad in (float("nan"), float("inf"), -float("inf")):
        for which in range(3):
            args = [I.copy(), I.copy(), np.array(rows12(I))]
            args[which].ravel()[5 if which < 2 else 7] = bad
            assert br.world_motion(*args) is None
            with pytest.raises(SfError, match="failed with -1"):
                bodies.world_motion(*args)
    b = bodies._product()
    assert b.world_motion(None, None, None, None) == -1


# ---- the premises, on the restatement alone --------------------------------------------------------------------------------
def test_a_pyramid_that_did_not_move_stays_put():
    """60 x 80, the camera moves, the pyramid does not: D0 from the poses already explains frame 1 to the depth quantisation
    (depths are rounded to millimetres: an error of at most 0.5 mm, rms 0.29 mm, seen through normals that are themselves taken
    from quantised depths). Measured on the restatement: rms 0.357 mm at D0 and 0.351 mm after every step, |W - I| <= 7.5e-4."""
    z0, l0, z1, l1, c0, c1 = bc.pyramid_pair(60, 80, *bc.MOVING_CAMERA, moved=False)
    out, systems = br.estimate(z0, l0, z1, l1, c0, c1, 1, None, br.params(), 2)
    r = out[0]
    assert int(r["status"]) == br.OK and int(r["iterations_done"]) == 10 and int(r["n_first"]) > 1000
    for it in range(11):
        assert rms_mm(systems[0, it, 0], systems[0, it, 1]) <= 1.0, it  # twice the largest quantisation error of a depth
    W = r["w"].reshape(4, 4).T
    ang, dist = bc.pose_error(W, np.eye(4))
    assert ang <= 3e-3 and dist <= 1e-3  # 1 mm: the same bound as a motion
    assert (out[1].tobytes() == bytes(192)) and not systems[1].any()


def test_the_moved_pyramid_is_found_at_60_x_80():
    """The moved pyramid at 60 x 80 (fx = fy = 70, principal point at the image centre), 10 iterations, camera at rest. Measured
    on this fp32 restatement with the quantised sums: 1106 of 1296 region pixels paired, rms 16.54 mm -> 1.17 mm after one
    step -> 0.447 mm from the second on, rotation error 3.8e-4 rad, translation error 0.13 mm at the body's centre (under the
    moving camera of body_cases: 16.41 -> 0.565 mm, 9.2e-4 rad, 0.36 mm). The bounds are the issue's: the squared rms falls at
    least 25-fold, the pose is within 3e-3 rad and 4 mm."""
    for cams in ((None, None), bc.MOVING_CAMERA):
        z0, l0, z1, l1, c0, c1 = bc.pyramid_pair(60, 80, *cams)
        out, systems = br.estimate(z0, l0, z1, l1, c0, c1, 1, None, br.params(), 1)
        r = out[0]
        print("moved pyramid 60 x 80:", dict(n_first=int(r["n_first"]), n_last=int(r["n_last"]), rms_first_mm=rms_mm(r["n_first"], r["ss_first"]),
                                            rms_last_mm=rms_mm(r["n_last"], r["ss_last"]), error=bc.pose_error(r["w"].reshape(4, 4).T, bc.motion())))
        assert int(r["status"]) == br.OK and int(r["iterations_done"]) == 10
        assert int(r["n_first"]) >= 1000 and int(r["n_last"]) >= 1000
        assert float(r["ss_last"]) / float(r["n_last"]) <= float(r["ss_first"]) / float(r["n_first"]) / 25.0
        ang, dist = bc.pose_error(r["w"].reshape(4, 4).T, bc.motion())
        assert ang <= 3e-3 and dist <= 4e-3
        assert r["d"][3] == 0 and r["d"][7] == 0 and r["d"][11] == 0 and r["d"][15] == 1
