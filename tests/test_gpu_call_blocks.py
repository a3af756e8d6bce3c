"""The per-call blocks of the companion interfaces (staticfusion_amd/csrc/sf_call_block.h) on the GPU: a block reused at another
size. For join.thin, body_maps.fuse, regions.label_images, bodies.estimate_images and score.score_images, on one handle: a small
call (one entry, a 24 x 32 frame, a map of 257 surfels), then a call large enough to grow the block and to move every offset
behind the first (three entries, 66 x 130 frames, maps of 1025 surfels), then the small call again. The first and the third
result are equal byte for byte, and equal to the same call as the first call of a fresh handle; the large result is that of a
handle whose second call it is. The sizes cross the 64, 256 and 1024 boundaries of the ballots, the workgroups and the scan.
What each call computes is held to its reference in the part's own test file; nothing here asserts a time."""
import functools
import types

import numpy as np
import pytest

import body_cases as bc
import body_map_cases as pc
import join_cases as jc
import region_cases as rc
import view_cases as vc
import view_ref
from staticfusion_amd import bodies, body_maps, join, regions, score, tracks, view
from test_gpu_view import small_solver, uploaded

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = {"small": (1, 24, 32, 257), "large": (3, 66, 130, 1025)}  # entries, rows, cols, surfels per map


def surfels_of_count(first, k, seed):
    """k surfels: spread over `first` as far as it reaches, then random ones"""
    step = max(first.shape[0] // k, 1)
    out = np.concatenate([first[::step][:k], jc.plain_surfels(k, seed)])[:k]
    assert out.shape == (k, 12)
    return np.ascontiguousarray(out, F)


# ---- the five calls: size name -> bytes of everything the call returns or writes ----------------------------------------------
def thin(s, size):
    n, _, _, k = SIZES[size]
    maps = [uploaded(s, jc.special_surfels(k, seed=40 + q, box=jc.box_for(k))) for q in range(n)]
    counts = join.thin(maps, join.Params(cell=jc.CELL))
    out = repr(counts).encode() + b"".join(m.download().tobytes() for m in maps)
    assert all(0 < c["n_out"] < k for c in counts)
    for m in maps:
        m.close()
    return out


@functools.lru_cache(maxsize=None)
def fuse_inputs(size):
    n, rows, cols, k = SIZES[size]
    first, _ = pc.first_map(rows, cols)
    surf = [surfels_of_count(first, k, seed=60 + q) for q in range(n)]
    z = [pc.plane(rows, cols, shift=0.002 * q) for q in range(n)]
    return surf, z, pc.labels_mixed(rows, cols), pc.cam(rows, cols), pc.colours(rows, cols)


def fuse(s, size):
    n, rows, cols, k = SIZES[size]
    surf, z, lab, cam, rgb = fuse_inputs(size)
    maps = [uploaded(s, a, tick=5, capacity=max(k + rows * cols, s.rows * s.cols)) for a in surf]
    camera = body_maps.Camera(cam["pose"], cam["cx"], cam["cy"], cam["fx"], cam["fy"])
    counts = body_maps.fuse(maps, z, [lab] * n, [camera] * n, [2] * n, None, [rgb] * n)
    out = repr(counts).encode() + b"".join(m.download().tobytes() for m in maps)
    assert all(c["n_added"] > 0 and c["n_voxels"] > 0 for c in counts)
    for m in maps:
        m.close()
    return out


def label(s, size):
    n, rows, cols, _ = SIZES[size]
    frames = [rc.random_levels(rows, cols, seed=rc.RANDOM_SEED + q) for q in range(n)]
    summ, per, labs = regions.label_images(s, [f[0] for f in frames], [f[1] for f in frames], regions.Params(b_max=rc.RANDOM_B_MAX, min_pixels=2),
                                           max_regions=64 * n, labels=True)
    assert all(len(r) > 0 for r in per) and all(a.max() > 0 for a in labs)
    return summ.tobytes() + b"".join(r.tobytes() for r in per) + b"".join(a.tobytes() for a in labs)


@functools.lru_cache(maxsize=None)
def pairs_of_frames(size):
    n, rows, cols, _ = SIZES[size]
    pair = bc.pyramid_pair(rows, cols)
    return [pair, bc.with_wall_patch(rows, cols, pair), bc.plane_pair(rows, cols)][:n]


def estimate(s, size):
    n, rows, cols, _ = SIZES[size]
    entries = pairs_of_frames(size)
    to_cam = lambda c: tracks.Camera(c["pose"], c["cx"], c["cy"], c["fx"], c["fy"])
    m = 2 * n  # (the large call: more region slots per entry, and a pair table)
    k = [int(e[1].max()) for e in entries]
    pairs = None if size == "small" else np.array([[t + 1 if t < k[q] else 0 for t in range(m)] for q in range(n)], np.int32)
    mot, sysm = bodies.estimate_images(s, [e[0] for e in entries], [e[1] for e in entries], [e[2] for e in entries], [e[3] for e in entries],
                                       [to_cam(e[4]) for e in entries], [to_cam(e[5]) for e in entries], k, pairs, bodies.Params(iterations=3, damping=1e-3),
                                       max_regions=m, systems=True)
    assert all(int(mot[q, 0]["n_first"]) > 0 for q in range(n))  # (pairs were found: the kernels had work)
    return mot.tobytes() + sysm.tobytes()


@functools.lru_cache(maxsize=None)
def score_inputs(size):
    n, rows, cols, k = SIZES[size]
    intr = types.SimpleNamespace(cx=(cols - 1) / 2.0, cy=(rows - 1) / 2.0, fx=0.9 * cols, fy=0.9 * cols)
    surf = [surfels_of_count(vc.frame_surfels(rows, cols, intr, seed=3 + q), k, seed=80 + q) for q in range(n)]
    frames = [vc.small_frame(rows, cols, seed=3 + q) for q in range(n)]
    depth = [np.asarray(f[0], F) for f in frames]
    grey = [np.asarray(view_ref.grey(f[1]), F) for f in frames]
    b = [rc.random_levels(rows, cols, seed=q)[1] for q in range(n)]
    views = [view.View(np.eye(4, dtype=F), intr.cx, intr.cy, intr.fx, intr.fy, rows, cols, min_confidence=0.0, max_depth=20.0) for _ in range(n)]
    return surf, depth, grey, b, views


def score_images(s, size):
    surf, depth, grey, b, views = score_inputs(size)
    maps = [uploaded(s, a) for a in surf]
    rec, cls = score.score_images(maps, views, depth, grey, b, score.Params(), classes=True)
    assert all(int(r["n_both"]) > 0 for r in rec)
    for m in maps:
        m.close()
    return rec.tobytes() + b"".join(a.tobytes() for a in cls)


@pytest.mark.parametrize("call", [thin, fuse, label, estimate, score_images], ids=lambda f: f.__name__)
def test_a_block_reused_at_another_size_gives_the_same_bytes(hip_auto, call):
    used, fresh = small_solver(hip_auto, 60, 80), small_solver(hip_auto, 60, 80)
    try:
        first = call(used, "small")
        large = call(used, "large")
        third = call(used, "small")
        assert len(large) > 3 * len(first)
        assert third == first
        assert call(fresh, "small") == first  # the first call of a handle: its block is made at exactly this size
        assert call(fresh, "large") == large  # ... and grown by its second
    finally:
        used.close()
        fresh.close()
