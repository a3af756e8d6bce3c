"""Shared set-up of the align tests (test_align_reference_cpu.py, test_gpu_align.py): one flat surfel that fills a view,
frames with every special value, and the convergence fixture -- the ranking case of score_cases.py with its twelve displaced
poses refined by the reference, computed once per process. It does not import the align binding: parameters are plain
namespaces with the members of sfa_params, which tests/align_ref.py reads."""
import functools
import types

import numpy as np

import align_ref
import score_cases as sc
import view_ref
from staticfusion_amd import view

TICK = 5


def params(dist_max=0.15, z_max=8.0, b_min=0.5, damping=0.0, iterations=10, stride=1, min_pairs=64, use_b=True):
    """the members of sfa_params with the header's defaults, float members rounded to float32 as the struct holds them"""
    f = lambda v: float(np.float32(v))  # noqa: E731
    return types.SimpleNamespace(dist_max=f(dist_max), z_max=f(z_max), b_min=f(b_min), damping=f(damping), iterations=int(iterations),
                                 stride=int(stride), min_pairs=int(min_pairs), use_b=int(use_b))


def as_kwargs(p):
    return dict(vars(p))


def flat_surfel(x, y, z, r, conf=0.5, normal=(0.0, 0.0, -1.0)):
    s = np.zeros(12, np.float32)
    s[:4] = (x, y, z, conf)
    s[4] = (10 << 16) + (20 << 8) + 30
    s[7] = TICK
    s[8:11] = normal
    s[11] = r
    return s


def plane_view(rows=16, cols=16, f=20.0, **kw):
    """a view at identity whose principal point is the centre of the pixel grid (pixel centres at integers)"""
    kw.setdefault("min_confidence", 0.0)
    return view.View(np.eye(4), (cols - 1) / 2.0, (rows - 1) / 2.0, f, f, rows, cols, **kw)


def special_frame(surf, v, seed, tick=TICK, noise=0.02):
    """depth and b images for view v: the map's own depth plus noise, and by position 0, NaN, inf, negative and 9 m depths, NaN
    b and b equal to the default b_min"""
    rng = np.random.default_rng(seed)
    rows, cols = v.rows, v.cols
    zm = view_ref.render(surf, v, tick=tick)["depth"]
    depth = np.where(zm > 0, zm + rng.normal(0, noise, zm.shape), rng.uniform(0.5, 4.0, zm.shape)).astype(np.float32)
    flat = np.arange(rows * cols).reshape(rows, cols)
    for mod, rem, val in ((17, 5, 0.0), (19, 6, np.nan), (23, 7, np.inf), (29, 8, -1.5), (31, 9, 9.0)):
        depth[flat % mod == rem] = val
    b = rng.random((rows, cols)).astype(np.float32)
    b[flat % 37 == 10] = np.nan
    b[flat % 41 == 11] = 0.5
    return depth, b


def pose_error(pose16):
    """(translation in metres, rotation angle in radians) of a column-major pose against identity"""
    T = np.asarray(pose16, np.float64).reshape(4, 4).T
    c = min(1.0, max(-1.0, (np.trace(T[:3, :3]) - 1.0) / 2.0))
    return float(np.linalg.norm(T[:3, 3])), float(np.arccos(c))


def convergence_case(step=sc.RANK_STEP):
    """depth, surfels and the twelve displaced views of score_cases.ranking_case (the true pose, its first view, left out)"""
    depth, _, surf, views = sc.ranking_case(step=step, **sc.RANK_INTRINSICS)
    return depth, surf, views[1:]


@functools.lru_cache(maxsize=None)
def convergence_reference(step=sc.RANK_STEP, dist_max=0.15, iterations=10):
    """[(result, systems)] of the twelve displaced poses refined by the reference (about 0.5 s each)"""
    depth, surf, views = convergence_case(step)
    p = params(dist_max=dist_max, iterations=iterations, stride=1, use_b=False)
    return [align_ref.refine(surf, v, depth, None, p, tick=1) for v in views]
