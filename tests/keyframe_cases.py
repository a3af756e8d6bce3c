"""Shared set-up of the keyframe tests (test_keyframes_reference_cpu.py, test_gpu_keyframes.py): the retrieval fixture --
twelve keyframe views of one room and a displaced query view beside each -- with its reference codes computed once per
process, and frames that hold every special value of the header."""
import functools

import numpy as np

import keyframe_ref as kr
from staticfusion_amd.synth import Scene, quantise_and_decimate, se3_exp

RET_ROWS, RET_COLS, RET_CELL, RET_FERNS, RET_SEED = 48, 64, 4, 128, 20261020
RET_MIN_DISTANCE = 20  # of the add test: below the smallest distance between two of the twelve keyframes (asserted on the CPU)


def _frame(scene, pose):
    depth, inten = scene.render(pose, 2 * RET_COLS, 2 * RET_ROWS, stride=2)
    return quantise_and_decimate(depth, inten, max_depth=4.5, decimate=False)


@functools.lru_cache(maxsize=None)
def retrieval_case():
    """dict: ferns, poses (12, 4, 4), keyframes and queries (lists of (depth, grey)), key_codes and query_codes (reference)"""
    scene = Scene(seed=1234)
    poses = [se3_exp([0.05 * k - 0.3, 0, 0.02 * k, 0, -0.44 + 0.08 * k, 0]) for k in range(12)]
    shift = se3_exp([0.02, -0.01, 0.015, 0.01, -0.012, 0.008])
    ferns = kr.default_ferns(RET_FERNS, RET_SEED, (RET_ROWS // RET_CELL) * (RET_COLS // RET_CELL))
    keyframes = [_frame(scene, p) for p in poses]
    queries = [_frame(scene, p @ shift) for p in poses]
    return dict(ferns=ferns, poses=np.array(poses, np.float32), keyframes=keyframes, queries=queries,
                key_codes=[kr.encode(d, g, ferns, RET_CELL) for d, g in keyframes], query_codes=[kr.encode(d, g, ferns, RET_CELL) for d, g in queries])


def special_frame(rows, cols, seed):
    """depth and grey with, by position, 0 / NaN / +inf / -inf / negative / > 32 m depths and NaN / < 0 / > 1 / +inf / -inf greys"""
    rng = np.random.default_rng(seed)
    depth = rng.uniform(0.3, 8.0, (rows, cols)).astype(np.float32)
    grey = rng.random((rows, cols)).astype(np.float32)
    flat = np.arange(rows * cols).reshape(rows, cols)
    for mod, rem, val in ((5, 1, 0.0), (7, 2, np.nan), (11, 3, np.inf), (13, 4, -np.inf), (17, 5, -1.5), (19, 6, 40.0)):
        depth[flat % mod == rem] = val
    for mod, rem, val in ((6, 1, np.nan), (7, 3, -0.25), (11, 5, 1.5), (13, 7, np.inf), (17, 9, -np.inf)):
        grey[flat % mod == rem] = val
    return depth, grey


def spread_ferns(n_ferns, n_cells, seed):
    """ferns over every cell with thresholds over the whole legal range, the bounds included"""
    rng = np.random.default_rng(seed)
    f = np.zeros(n_ferns, kr.FERN_DTYPE)
    f["cell"] = rng.integers(0, n_cells, n_ferns)
    f["t_grey"] = rng.choice(np.array([0, 410, 1500, 2048, 2600, 3686, 4096]), n_ferns)
    f["t_depth"] = rng.choice(np.array([0, 512, 2000, 4096, 7168, 32768]), n_ferns)
    f["cell"][0] = n_cells - 1
    return f
