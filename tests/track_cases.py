"""The frames of the track tests (tests/test_gpu_tracks.py, tests/test_tracks_reference_cpu.py), each a function of its size
alone: rectangles of constant depth in front of nothing (depth 0, outside the mask), and the cameras that look at them. A CASE
is a list of steps (depth, b, camera, region parameters, track parameters) that update one slot in turn; cameras and parameters
are those of tests/track_ref.py. Imports neither the product nor the oracle."""
import numpy as np

import region_ref as rr
import track_ref as tr

F = np.float32
RP = dict(use_b=0, min_pixels=1, connectivity=8)  # depth alone decides the mask; b is a plane of 0.25 that nothing reads


def intrinsics(rows, cols):
    return dict(cx=(cols - 1) / 2.0, cy=(rows - 1) / 2.0, fx=float(max(rows, cols)), fy=float(max(rows, cols)))


def cam(rows, cols, pose=None):
    return tr.camera(pose, **intrinsics(rows, cols))


def rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    T = np.eye(4)
    T[i, i], T[i, j], T[j, i], T[j, j] = c, -s, s, c
    return T


def shift(x=0.0, y=0.0, z=0.0):
    T = np.eye(4)
    T[:3, 3] = (x, y, z)
    return T


def rects(rows, cols, items):
    """items: (v0, v1, u0, u1, z) in fractions of the image (v1, u1 exclusive), or in pixels when integers"""
    d = np.zeros((rows, cols), F)
    for v0, v1, u0, u1, z in items:
        px = [int(np.floor(a * n)) if isinstance(a, float) else a for a, n in ((v0, rows), (v1, rows), (u0, cols), (u1, cols))]
        d[max(px[0], 0):max(px[1], 0), max(px[2], 0):max(px[3], 0)] = F(z)
    return d


def step(depth, camera, rp=None, tp=None):
    return (depth, np.full(depth.shape, 0.25, F), camera, rr.params(**dict(RP, **(rp or {}))), tr.params(**(tp or {})))


def two(rows, cols):
    return rects(rows, cols, [(0.1, 0.9, 0.05, 0.4, 2.0), (0.2, 0.8, 0.6, 0.95, 3.0)])


def moved(rows, cols, s, z=2.0):
    """one rectangle, s columns to the right of where `moved(rows, cols, 0)` has it"""
    u0, u1 = int(np.floor(0.25 * cols)) + s, max(int(np.floor(0.7 * cols)), int(np.floor(0.25 * cols)) + 1) + s
    return rects(rows, cols, [(0.2, 0.8, u0, u1, z)])


def checkerboard(rows, cols):
    v, u = np.indices((rows, cols))
    return np.where((v + u) % 2 == 0, F(1.0), F(0.0)).astype(F)


def five(rows, cols):
    return rects(rows, cols, [(0.0, 1.0, k / 5.0, k / 5.0 + 0.12, 1.5 + 0.5 * k) for k in range(5)])


def cases_of(rows, cols):
    """name -> list of steps"""
    c0 = cam(rows, cols)
    fx = intrinsics(rows, cols)["fx"]
    out = {}
    out["identical"] = [step(two(rows, cols), c0), step(two(rows, cols), c0)]
    for s in (0, 1, 7):
        out["shift%d" % s] = [step(moved(rows, cols, 0), c0), step(moved(rows, cols, s), c0)]
    # the camera moves 3 pixels' worth to the right at z = 2: the rectangle appears 3 columns further left
    out["translation"] = [step(moved(rows, cols, 3), c0), step(moved(rows, cols, 0), cam(rows, cols, shift(x=3 * 2.0 / fx)))]
    out["roll"] = [step(two(rows, cols), c0), step(two(rows, cols), cam(rows, cols, rot(2, 0.3)))]
    whole = rects(rows, cols, [(0.1, 0.9, 0.1, 0.9, 2.0)])
    parts = rects(rows, cols, [(0.1, 0.9, 0.1, 0.55, 2.0), (0.1, 0.9, 0.65, 0.9, 2.0)])
    out["split"] = [step(whole, c0), step(parts, c0)]
    out["merge"] = [step(parts, c0), step(whole, c0)]
    left_right = rects(rows, cols, [(0.1, 0.9, 0.05, 0.4, 2.0), (0.1, 0.9, 0.6, 0.95, 3.0)])
    right_left = rects(rows, cols, [(0.1, 0.9, 0.05, 0.4, 3.0), (0.1, 0.9, 0.6, 0.95, 2.0)])
    out["swap_gated"] = [step(left_right, c0), step(right_left, c0)]
    out["swap_ungated"] = [step(left_right, c0), step(right_left, c0, tp=dict(use_depth_gate=0))]
    out["leaves"] = [step(two(rows, cols), c0), step(two(rows, cols), cam(rows, cols, shift(x=1000.0)))]
    out["behind"] = [step(two(rows, cols), c0), step(two(rows, cols), cam(rows, cols, rot(1, np.pi)))]
    # the camera moves 6 m backwards: what was at 2 m is at 8 m and a quarter of the size, so several sources share a target
    out["backwards"] = [step(rects(rows, cols, [(0.1, 0.9, 0.1, 0.9, 2.0)]), c0), step(rects(rows, cols, [(0.4, 0.6, 0.4, 0.6, 8.0)]), cam(rows, cols, shift(z=-6.0)))]
    # the gate: 0.25 + 0 * min is exact, 2.25 - 2 meets it, the next float above 2.25 is one ulp beyond
    edge = rects(rows, cols, [(0.1, 0.9, 0.05, 0.4, 2.25), (0.1, 0.9, 0.6, 0.95, float(np.nextafter(F(2.25), F(3))))])
    flat = rects(rows, cols, [(0.1, 0.9, 0.05, 0.4, 2.0), (0.1, 0.9, 0.6, 0.95, 2.0)])
    out["gate_edge"] = [step(flat, c0), step(edge, c0, tp=dict(dz_abs=0.25, dz_rel=0.0))]
    out["gate_off"] = [step(flat, c0), step(edge, c0, tp=dict(dz_abs=0.25, dz_rel=0.0, use_depth_gate=0))]
    holes = two(rows, cols)
    holes[rows // 2, cols // 4] = np.nan
    holes[rows // 3, (3 * cols) // 4] = np.inf
    holes[0, 0] = np.nan
    out["special"] = [step(holes, c0), step(two(rows, cols), c0)]
    out["five"] = [step(five(rows, cols), c0), step(five(rows, cols), c0)]
    return out


def long_case(rows, cols):
    """five updates of one slot: a rectangle walks right; a second one is there in frames 0 and 1, gone in 2 and 3, and one
    stands in the same place again in frame 4"""
    c0 = cam(rows, cols)
    out = []
    for f in range(5):
        items = [(0.1, 0.45, int(0.1 * cols) + 2 * f, int(0.1 * cols) + 2 * f + max(cols // 4, 1), 2.0)]
        if f in (0, 1, 4):
            items.append((0.6, 0.95, 0.5, 0.9, 3.0))
        out.append(step(rects(rows, cols, items), c0))
    return out
