"""Shared cases of the register tests (test_register_*_cpu.py, test_gpu_register.py): the corner scene of three planes with its
known motion, its variants (a single plane, another grid), surfel sets on the boundaries of the rule PAIR of
include/sf_register.h, a destination whose keys collide in their first slot, and the entries of the batch test. NumPy and the
restatements only."""
import numpy as np

import align_ref
import join_cases as jc
import join_ref
import register_ref as rr

CORNER = np.array([0.3, -0.2, 1.0])
SPACING, JITTER = 0.02, 0.004
W = (0.03, -0.021, 0.015)        # Cayley parameters of the motion's rotation
T = (0.02, -0.01, 0.016)         # ... and its translation


def motion(scale=1.0, t_scale=None):
    """(R, t) of the scene's motion in float64, its parameters scaled"""
    t_scale = scale if t_scale is None else t_scale
    R = np.array(align_ref.cayley(*[scale * w for w in W]), np.float64)
    return R, t_scale * np.array(T, np.float64)


def as_matrix(R, t):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    return M.astype(np.float32)


def planes(side=23, axes=(0, 1, 2), seed=11):
    """len(axes) planes through CORNER, plane k perpendicular to axis axes[k]: side x side surfels at SPACING, jittered in-plane
    by +-JITTER, normals along the axis, distinct confidences, unit colours and times"""
    rng = np.random.default_rng(seed)
    out = []
    for ax in axes:
        u, v = [a for a in (0, 1, 2) if a != ax]
        gi, gj = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
        p = np.tile(CORNER, (side * side, 1))
        p[:, u] += (gi.ravel() + 0.5) * SPACING + rng.uniform(-JITTER, JITTER, side * side)
        p[:, v] += (gj.ravel() + 0.5) * SPACING + rng.uniform(-JITTER, JITTER, side * side)
        s = np.zeros((side * side, 12), np.float32)
        s[:, 0:3] = p
        s[:, 8 + ax] = 1.0
        out.append(s)
    s = np.concatenate(out)
    n = s.shape[0]
    s[:, 3] = (0.25 + 0.5 * rng.permutation(n) / n).astype(np.float32)  # distinct
    s[:, 4] = 0x808080
    s[:, 6] = s[:, 7] = 1
    s[:, 11] = 0.01
    assert len(set(s[:, 3].tolist())) == n
    return s


def moved_by_inverse(surfels, R, t):
    """the surfels in a frame from which (R, t) leads back: p' = R^T (p - t), n' = R^T n"""
    s = np.array(surfels, np.float32)
    s[:, 0:3] = ((s[:, 0:3].astype(np.float64) - t) @ R).astype(np.float32)
    s[:, 8:11] = (s[:, 8:11].astype(np.float64) @ R).astype(np.float32)
    return s


def corner(side=23, axes=(0, 1, 2)):
    """(destination, source, R, t): the source is every third surfel of the reversed destination, moved by the inverse of
    the motion, so that E = [R t] puts it back"""
    dst = planes(side, axes)
    R, t = motion()
    src = moved_by_inverse(dst[::-1][::3], R, t)
    return dst, src, R, t


def estimate_error(E, R, t):
    return float(np.max(np.abs(np.array(E, np.float64).reshape(3, 4) - np.concatenate([R, t[:, None]], axis=1))))


def as_product(p):
    from staticfusion_amd import register

    return register.Params(**{k: getattr(p, k) for k in rr.DEFAULTS})


def random_pair(n=500, seed=3, cell=0.1):
    """n destination surfels in a box of a few cells, and as many sources near them: most within reach of a partner"""
    dst = jc.plain_surfels(n, seed, box=2.5 * cell)
    rng = np.random.default_rng(seed + 1)
    src = jc.plain_surfels(n, seed + 2, box=2.5 * cell)
    take = rng.permutation(n)
    src[:, 0:3] = dst[take, 0:3] + rng.normal(scale=0.15 * cell, size=(n, 3)).astype(np.float32)
    src[:, 8:11] = dst[take, 8:11]
    flip = rng.uniform(size=n) < 0.2
    src[flip, 8:11] = -src[flip, 8:11]
    return dst, src


def boundary_pair(cell=0.1):
    """one representative per voxel of a 4 x 4 x 4 block around the origin (negative coordinates among them), and sources on
    voxel faces (sc - f == 0), voxel centres (sc - f == 0.5), just beside both, and one equidistant from two representatives"""
    c = np.float32(cell)
    dst = []
    for qx in range(-2, 2):
        for qy in range(-2, 2):
            for qz in range(-2, 2):
                s = np.zeros(12, np.float32)
                s[0:3] = jc.centre_of((qx, qy, qz), cell)
                s[3] = 0.5
                s[8:11] = (0.0, 0.0, 1.0)
                dst.append(s)
    dst = np.array(dst, np.float32)
    src = []
    for x in (-1.0, -0.5, 0.0, 0.5, 1.0):
        for y in (-0.5, 0.0, 0.5):
            for z in (-1.0, -0.5, 0.0, 0.5):
                for nudge in (0.0, 1.0, -1.0):
                    s = np.zeros(12, np.float32)
                    p = np.array([x, y, z], np.float32) * c
                    if nudge:
                        p = np.nextafter(p, np.float32(nudge * 10), dtype=np.float32)
                    s[0:3] = p
                    s[3] = 0.5
                    s[8:11] = (0.0, 0.0, 1.0)
                    src.append(s)
    src = np.array(src, np.float32)
    # two more representatives, in the voxels (-1, 5, 5) and (0, 5, 5), and a source on the face between them, equally far from
    # both: the written order visits Q's own voxel (0, 5, 5) first, and the other must not replace it. The one that must win has
    # the higher index and the lower confidence.
    tie = np.zeros((3, 12), np.float32)
    tie[:, 0:3] = ((-0.02, 0.55, 0.55), (0.02, 0.55, 0.55), (0.0, 0.55, 0.55))
    tie[:, 3] = (0.5, 0.4, 0.5)
    tie[:, 8:11] = (0.0, 0.0, 1.0)
    return np.concatenate([dst, tie[:2]]), np.concatenate([src, tie[2:]])


def special_pair(cell=0.1):
    """the random pair with NaN, inf and 1e9 positions on both sides, zero and non-finite normals, special confidences"""
    dst, src = random_pair(200, 9, cell)
    for j, v in enumerate((np.nan, np.inf, -np.inf, 1e9, -1e9, 3e38)):
        dst[3 + 5 * j, j % 3] = v
        src[4 + 7 * j, (j + 1) % 3] = v
    for j, v in enumerate(((0, 0, 0), (np.nan, 0, 1), (np.inf, 0, 0), (1e-30, 0, 0), (1e25, 1e25, 0), (0, 0, -0.0))):
        dst[60 + 3 * j, 8:11] = v
        src[90 + 3 * j, 8:11] = v
    for j, v in enumerate((np.nan, -0.0, 0.0, -1.0, np.inf)):
        dst[120 + j, 3] = v
        src[130 + j, 3] = v
    return dst, src


def colliding_pair(n_cells=12, cell=0.1):
    """a destination of n_cells surfels whose keys all fall on slot 5 of the 64 slots their table has, with a second surfel in
    every third voxel, and sources beside each of them"""
    slots = join_ref.table_slots(n_cells + n_cells // 3 + (1 if n_cells % 3 else 0))
    assert slots == 64
    cells = jc.cells_on_slot(slots, 5, n_cells)
    dst = []
    for j, q in enumerate(cells):
        for k in range(2 if j % 3 == 0 else 1):
            s = np.zeros(12, np.float32)
            s[0:3] = jc.centre_of(q, cell) + np.float32(0.01 * k)
            s[3] = 0.3 + 0.1 * k
            s[8:11] = (1.0, 0.0, 0.0) if j % 2 else (0.0, 1.0, 0.0)
            dst.append(s)
    dst = np.array(dst, np.float32)
    assert join_ref.table_slots(dst.shape[0]) == 64
    src = np.ascontiguousarray(dst[::-1])
    src[:, 0:3] += np.float32(0.004)
    return dst, src
