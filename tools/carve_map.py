"""A box that was fused into a map and then carried away, carved out of the map again (include/sf_carve.h), at QVGA.

The scene of tests/carve_cases.py: a wall at z = 3, a floor at y = 1 seen at a grazing angle, a box face at z = 1.6. A static
camera (view A) fuses four frames with the box present through the whole pipeline (load, solve, fuse). Then the box is gone:
frames from A and from two displaced views B and E vote. Printed: the score's n_behind of a box-gone frame against the map
before and after the carve ("the frame sees through the map"), and the counts. Written: the map from view B before and after,
as PGM depth images (sfv_render_maps).

The fuse of this library stores normals that point AWAY from the camera that saw them (the cross product of data.vert), and
OBSERVE judges a surfel only when it faces the camera (d < 0): the first carve, of the map as fused, therefore judges nothing.
The tool prints that, turns the normals round (download, negate, upload) and carves again.

usage: python tools/carve_map.py [--out DIR]
"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import staticfusion_amd as sf
from staticfusion_amd import SurfelMap, carve, score, view

ROWS, COLS = 240, 320
BOX = (-0.4, 0.4, 0.0, 0.24)  # x0, x1, y0, y1 of the face at z = 1.6


def pose_of(name):
    T = np.eye(4, dtype=np.float32)
    t, a = dict(A=((0, 0, 0), 0.0), B=((0.25, -0.05, 0.0), -0.06), E=((-0.3, -0.1, 0.1), 0.08))[name]
    c, s = np.cos(a), np.sin(a)
    T[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)
    T[:3, 3] = t
    return T


def cast(T, cx, cy, fx, fy, rows, cols, box):
    """camera z of the nearest of wall, floor and box face along the ray of every pixel (pixel centres at integers)"""
    T = np.asarray(T, np.float64)
    R, t = T[:3, :3], T[:3, 3]
    u, w = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    ray = np.stack([(u - cx) / fx, (w - cy) / fy, np.ones_like(u)], -1) @ R.T
    with np.errstate(all="ignore"):
        best = np.full(u.shape, np.inf)
        lam = (3.0 - t[2]) / ray[..., 2]
        best = np.where(lam > 0, np.minimum(best, lam), best)
        lam = (1.0 - t[1]) / ray[..., 1]
        best = np.where((lam > 0) & (t[2] + lam * ray[..., 2] <= 3.0), np.minimum(best, lam), best)
        if box:
            lam = (1.6 - t[2]) / ray[..., 2]
            x, y = t[0] + lam * ray[..., 0], t[1] + lam * ray[..., 1]
            best = np.where((lam > 0) & (x >= BOX[0]) & (x <= BOX[1]) & (y >= BOX[2]) & (y <= BOX[3]), np.minimum(best, lam), best)
    return np.where(np.isfinite(best), best, 0.0).astype(np.float32)


def write_pgm(path, depth, z_far=4.0):
    img = np.clip(np.rint(depth / z_far * 255.0), 0, 255).astype(np.uint8)
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img).tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="directory for the two PGM files (default: a fresh temporary directory)")
    a = ap.parse_args()
    if a.out is None:
        a.out = tempfile.mkdtemp(prefix="carve_map_")
    os.makedirs(a.out, exist_ok=True)
    print("writing before_B.pgm and after_B.pgm to %s" % a.out)
    api = sf.load()
    s = sf.Solver(api, ROWS, COLS, 1, api.default_params_struct())
    m = SurfelMap(s, 8 * ROWS * COLS)
    mp = s.default_model_params()

    def sensor(box):
        """what the loader takes: the frame of view A at twice the size, rows flipped, depth in millimetres"""
        d = cast(pose_of("A"), 2 * mp.cx, 2 * mp.cy, 2 * mp.fx, 2 * mp.fy, 2 * ROWS, 2 * COLS, box)
        grey = np.clip(np.rint(60 + 40 * d), 1, 255).astype(np.uint8)
        return np.ascontiguousarray(np.repeat(grey[::-1, :, None], 3, axis=2)), np.ascontiguousarray(np.clip(np.rint(d[::-1] * 1000), 0, 65535).astype(np.uint16))

    # ---- fuse the box in: four frames from a camera that stands still
    there = sensor(True)
    s.load_frame(0, *there, 2)
    s.current_to_prediction()
    s.push_history(0)
    s.set_kb(1.05)
    s.load_frame(0, *there, 2)
    s.process_frame(1)
    s.filter_depth()
    SurfelMap.fuse_frames(s, [0], [m], list(s.batch_results()[0]), 1.0, mp)
    for k in range(2, 5):
        SurfelMap.predict_frames(s, [0], [m], mp)
        s.load_frame(0, *there, 2)
        s.filter_depth()
        s.process_frame(k)
        SurfelMap.fuse_frames(s, [0], [m], list(s.batch_results()[0]), 1.0, mp)
    info = m.info()
    print("fused: %d surfels, tick %d" % (info["count"], info["tick"]))
    # ---- take it away: three frames without the box
    views = {k: view.View(pose_of(k), mp.cx, mp.cy, mp.fx, mp.fy, ROWS, COLS, min_confidence=0.0) for k in "ABE"}
    gone = {k: cast(pose_of(k), mp.cx, mp.cy, mp.fx, mp.fy, ROWS, COLS, False) for k in "ABE"}
    sp = score.Params(use_grey=False, use_b=False)
    behind = lambda: int(score.score_images([m], [views["B"]], [gone["B"]], params=sp)["n_behind"][0])  # noqa: E731
    crv = carve.Carver(s)
    entries = [(0, views[k], gone[k]) for k in "ABE"]
    before = behind()
    write_pgm(os.path.join(a.out, "before_B.pgm"), view.render([m], [views["B"]], rgb=False, index=False)[0]["depth"])
    (c,) = crv.carve([m], carve.Params(), entries)
    print("the map as fused (normals point away from the camera): n_behind %d, counts %r" % (before, c))
    surf = m.download()
    surf[:, 8:11] *= -1
    m.upload(surf, info["pose"], info["tick"])
    (c,) = crv.carve([m], carve.Params(), entries)
    after = behind()
    write_pgm(os.path.join(a.out, "after_B.pgm"), view.render([m], [views["B"]], rgb=False, index=False)[0]["depth"])
    print("normals turned to the camera: n_behind %d -> %d, counts %r" % (before, after, c))
    box_left = int(((np.abs(m.download()[:, 2] - 1.6) < 0.05)).sum())
    print("surfels within 5 cm of the box face's plane: %d before, %d after" % (int((np.abs(surf[:, 2] - 1.6) < 0.05).sum()), box_left))
    crv.close()
    m.close()
    s.close()


if __name__ == "__main__":
    main()
