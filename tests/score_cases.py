"""Shared set-up of the score tests (test_score_reference_cpu.py, test_gpu_score.py): the ranking fixture -- a frame, the
surfels made from it, the true pose and twelve displaced ones -- with its reference scores computed once per process."""
import functools
import types

import numpy as np

import score_ref
import view_cases as vc
import view_ref
from staticfusion_amd import score, view
from staticfusion_amd.synth import se3_exp
from test_model_prediction import surfels_from_frame  # (imported, not edited)

RANK_ROWS, RANK_COLS = 60, 80
RANK_INTRINSICS = dict(cx=39.5, cy=29.5, fx=72.0, fy=72.0)
RANK_STEP = 0.05  # the displacement along one twist axis, metres or radians


def ranking_case(cx, cy, fx, fy, step=RANK_STEP):
    """frame (depth, grey), surfels made from it at identity, and thirteen views: the true pose first, then the poses
    displaced by +step and -step along each of the six twist axes"""
    depth, rgb = vc.small_frame(RANK_ROWS, RANK_COLS)
    cam = types.SimpleNamespace(cx=cx, cy=cy, fx=fx, fy=fy)
    surf = surfels_from_frame(depth, rgb, np.eye(4), cam, seed=3)
    poses = [np.eye(4, dtype=np.float32)]
    for axis in range(6):
        for sign in (1.0, -1.0):
            xi = np.zeros(6)
            xi[axis] = sign * step
            poses.append(se3_exp(xi).astype(np.float32))
    views = [view.View(p, cx, cy, fx, fy, RANK_ROWS, RANK_COLS, min_confidence=0.0, max_depth=20.0) for p in poses]
    return depth, view_ref.grey(rgb), surf, views


def ranking_params():
    return score.Params(tol_abs=0.02, tol_rel=0.01, use_b=False)


@functools.lru_cache(maxsize=None)
def ranking_reference(cx, cy, fx, fy, step=RANK_STEP):
    """the thirteen reference records of ranking_case (about 0.4 s each)"""
    depth, grey, surf, views = ranking_case(cx, cy, fx, fy, step)
    return [score_ref.score(surf, v, depth, grey, None, ranking_params(), tick=1)[0] for v in views]
