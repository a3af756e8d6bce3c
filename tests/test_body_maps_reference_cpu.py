"""The premise of the body maps, on the restatement alone (tests/body_map_ref.py; no GPU, no library): a sphere ray-cast with
depths rounded to millimetres moves by a known rigid motion over 8 frames and is fused with that motion at the parameter
defaults. Seeing the surface again must add less than seeing it first, and the surfels seen at least three times must lie
nearer the true sphere than the surfels of the first frame did. The assertions are inequalities within the run; the measured
values are printed and recorded in DESIGN.md section 29. Plus the properties of the restatement the GPU tests lean on."""
import numpy as np

import body_cases as bc
import body_map_cases as pc
import body_map_ref as pr

F = np.float32
ROWS, COLS, FRAMES = 240, 320, 8
STEP = bc.motion(rotvec=(0.0, 0.02, 0.01), shift=(0.004, -0.002, 0.003), centre=pc.SPHERE_CENTRE)


def sphere_run(p=None):
    """[(counts, count, seen3, rms3 in metres)] per frame and the rms of the first frame's surfels"""
    cam = pc.cam(ROWS, COLS)
    surf, centre, out = np.zeros((0, 12), F), pc.SPHERE_CENTRE.copy(), []
    rms_first = None
    for k in range(FRAMES):
        if k:
            centre = STEP[:3, :3] @ centre + STEP[:3, 3]
        depth, mask = pc.sphere(ROWS, COLS, cam, centre)
        surf, c = pr.fuse(surf, k + 1, depth, mask.astype(np.int32), cam, 1, STEP if k else None, None, p)
        dist = np.abs(np.linalg.norm(surf[:, 0:3].astype(np.float64) - centre, axis=1) - pc.SPHERE_RADIUS)
        if k == 0:
            rms_first = float(np.sqrt(np.mean(dist ** 2)))
        seen = surf[:, 5] >= 3
        out.append((c, surf.shape[0], int(seen.sum()), float(np.sqrt(np.mean(dist[seen] ** 2))) if seen.any() else float("nan")))
    return out, rms_first


def test_a_moving_sphere_gets_denser_and_less_noisy_at_the_defaults():
    run, rms_first = sphere_run()
    for k, (c, count, seen3, rms3) in enumerate(run):
        print("frame %d: pixels %d candidates %d merged %d added %d conflict %d count %d seen>=3 %d rms(seen>=3) %.3f mm"
              % (k + 1, c["n_pixels"], c["n_candidates"], c["n_merged"], c["n_added"], c["n_conflict"], count, seen3, rms3 * 1e3))
    print("rms of the first frame's surfels %.3f mm" % (rms_first * 1e3))
    first, second = run[0][0], run[1][0]
    assert 1000 < first["n_added"] < first["n_candidates"] and first["n_merged"] == 0  # several pixels share a voxel; nothing to merge into yet
    assert second["n_added"] < first["n_added"]
    assert run[-1][2] > 100 and run[-1][3] < rms_first
    assert all(c["n_out"] == count and c["n_merged"] + c["n_added"] + c["n_conflict"] <= c["n_candidates"] <= c["n_pixels"] for c, count, _, _ in run)


def test_fusing_twice_and_the_order_of_the_append():
    rows, cols = 12, 14
    p = pr.params()
    detail = {}
    z, lab, cam = pc.plane(rows, cols), pc.labels_mixed(rows, cols), pc.cam(rows, cols)
    surf, c = pr.fuse(np.zeros((0, 12), F), 1, z, lab, cam, 2, None, pc.colours(rows, cols), p, detail)
    assert c["n_added"] == c["n_out"] == surf.shape[0] > 50 and c["n_voxels"] == 0 and c["n_merged"] == 0
    order = [v + u * rows for v, u in detail["added"]]
    assert order == sorted(order)
    assert np.all(surf[:, 5] == 1) and np.all(surf[:, 6] == 1) and np.all(surf[:, 7] == 1) and np.all(surf[:, 3] == F(0.1))
    again, c2 = pr.fuse(surf, 2, z, lab, cam, 2, None, pc.colours(rows, cols), p)
    assert c2["n_added"] == 0 and c2["n_merged"] == c["n_added"] and c2["n_voxels"] == c["n_added"]
    assert again[:, 0:3].tobytes() == surf[:, 0:3].tobytes()  # ((w x) + x) / (w + 1) with w = 1 is x
    assert np.all(again[:, 5] == 2) and np.all(again[:, 3] > surf[:, 3]) and np.all(again[:, 7] == 2) and np.all(again[:, 6] == 1)
    assert again[:, 4].tobytes() == surf[:, 4].tobytes()
