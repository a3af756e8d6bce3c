"""Shared set-up of the free-view tests (test_view_reference_cpu.py, test_gpu_view.py): small synthetic surfel buffers, the
poses, and a stream primed so that a prediction (the oracle's, or the library's) is a pure render of the model."""
import types

import numpy as np

from staticfusion_amd import view as sfview
from staticfusion_amd.synth import se3_exp
from test_model_prediction import surfels_from_frame  # (imported, not edited)

SIZES = [(60, 80), (30, 40)]  # handles of 80 x 60 and 40 x 30


def small_frame(rows, cols, seed=3):
    """a depth frame with a wavy wall, a nearer box (an occlusion edge) and a hole, and colours with every channel >= 1"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    depth = 2.0 + 0.3 * np.sin(xx * 8.0 / cols) + 0.2 * np.cos(yy * 6.0 / rows)
    depth[rows // 3: rows // 2, cols // 4: cols // 2] = 1.2
    depth[rows - rows // 5:, : cols // 6] = 0.0
    rgb = rng.integers(1, 256, (rows, cols, 3)).astype(np.uint8)
    return depth.astype(np.float32), rgb


def frame_surfels(rows, cols, mp, seed=3, step=1):
    depth, rgb = small_frame(rows, cols, seed)
    cam = types.SimpleNamespace(cx=mp.cx, cy=mp.cy, fx=mp.fx, fy=mp.fy)
    return surfels_from_frame(depth, rgb, np.eye(4), cam, step=step, seed=seed)


def poses():
    """identity, a rotated and translated camera, and one that looks away from the model"""
    moved = se3_exp(np.array([0.08, -0.05, 0.12, 0.04, -0.07, 0.03])).astype(np.float32)
    away = np.diag([-1.0, 1.0, -1.0, 1.0]).astype(np.float32)  # half a turn about y
    return [("identity", np.eye(4, dtype=np.float32)), ("moved", moved), ("away", away)]


def other_intrinsics(mp):
    return dict(cx=mp.cx + 1.75, cy=mp.cy - 2.25, fx=mp.fx * 0.9, fy=mp.fy * 1.1)


def prime_pure_render(s, rows, cols):
    """a previous frame that cannot fill anything in: an all-black colour frame and b = 0.1 (< 0.6: no depth fill-in)"""
    s.load_frame(0, np.zeros((2 * rows, 2 * cols, 3), np.uint8), np.full((2 * rows, 2 * cols), 1500, np.uint16), 2)
    s.filter_depth()
    s.set_segm_state(0, np.zeros((rows, cols), np.int32), np.full(24, 0.1, np.float32), np.ones(24, np.float32))
    s.build_segm_image()


def pure_render_params(s, intr, threshold, max_depth, time):
    """model parameters under which sf_predict_from_model draws one target and clips nothing"""
    mp = s.default_model_params()
    mp.cx, mp.cy, mp.fx, mp.fy = intr["cx"], intr["cy"], intr["fx"], intr["fy"]
    mp.conf_low = mp.conf_high = threshold
    mp.max_depth = mp.extract_max_depth = max_depth
    mp.time = mp.max_time = time
    return mp


def view_of(mp, pose, rows, cols, **over):
    kw = dict(pose=pose, cx=mp.cx, cy=mp.cy, fx=mp.fx, fy=mp.fy, rows=rows, cols=cols, min_confidence=mp.conf_high, max_depth=mp.max_depth)
    kw.update(over)
    return sfview.View(**kw)
