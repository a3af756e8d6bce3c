"""Look at a surfel map: a short synthetic sequence through predict -> input -> solve -> fuse (the loop of
tools/full_pipeline_bench.py, one stream), then an orbit of N free views of the map (include/sf_view.h), written as binary PPM
(colour, normals) and 16-bit PGM (depth in millimetres). No dependency beyond NumPy.

usage: python tools/render_map.py [--frames 10] [--views 8] [--rows 480] [--cols 640] [--out render_out] [--normals]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import staticfusion_amd as sf
from staticfusion_amd import view
from staticfusion_amd.synth import Scene, se3_exp


def write_ppm(path, rgb):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]))
        f.write(np.ascontiguousarray(rgb, np.uint8).tobytes())


def write_pgm16(path, depth_m):
    mm = np.clip(np.rint(depth_m * 1000.0), 0, 65535).astype(">u2")  # PGM with maxval > 255 is big-endian
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n65535\n" % (mm.shape[1], mm.shape[0]))
        f.write(mm.tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--rows", type=int, default=480)
    ap.add_argument("--cols", type=int, default=640)
    ap.add_argument("--out", default="render_out")
    ap.add_argument("--normals", action="store_true", help="shade with the camera-frame normal instead of the colour")
    a = ap.parse_args()
    api = sf.load()
    rows, cols = 240, 320
    s = sf.Solver(api, rows, cols, 1, api.default_params_struct())
    m = sf.SurfelMap(s, 4 * rows * cols)
    mp = s.default_model_params()
    scene = Scene(seed=77, sphere=False)
    xi = np.array([0.010, 0.004, 0.006, 0.002, -0.004, 0.003]) * 0.6
    T = np.eye(4)
    for k in range(a.frames):
        depth, inten = scene.render(T, 640, 480)
        g = np.clip(np.rint(inten * 255), 1, 255).astype(np.uint8)
        if k >= 2:  # the prediction fills in from the PREVIOUS frame: before the load
            s.set_kb(1.05 if k == 2 else 1.5)
            m.predict(0, mp)
        s.load_frame(0, np.ascontiguousarray(np.repeat(g[::-1, :, None], 3, axis=2)), np.ascontiguousarray(np.clip(np.rint(depth[::-1] * 1000), 0, 65535).astype(np.uint16)), 2)
        if k == 0:  # bootstrap (StaticFusion-imagesequenceassoc.cpp:102-137)
            s.current_to_prediction()
            s.push_history(0)
            s.set_kb(1.05)
        else:
            if k >= 2:
                s.filter_depth()
            s.process_frame(k)
            Tq = s.batch_results()[0]
            if k == 1:
                s.filter_depth()
            sf.SurfelMap.fuse_frames(s, [0], [m], list(Tq), 1.0, mp)
        T = T @ se3_exp(xi)
    info = m.info()
    surf = m.download()
    centre = np.median(surf[:, :3], axis=0).astype(np.float64)
    f = 0.9 * a.cols
    views = []
    for q in range(a.views):
        ang = 2 * np.pi * q / max(a.views, 1)
        eye = centre + np.array([1.2 * np.sin(ang), -0.3, -1.8 + 0.6 * (1 - np.cos(ang))])
        views.append(view.View(view.look_at(eye, centre), a.cols / 2, a.rows / 2, f, f, a.rows, a.cols, min_confidence=0.0,
                               shade=view.SHADE_NORMAL if a.normals else view.SHADE_COLOUR))
    images = view.render([m] * a.views, views)
    os.makedirs(a.out, exist_ok=True)
    for q, im in enumerate(images):
        write_ppm(os.path.join(a.out, "view_%02d.ppm" % q), im["rgb"])
        write_pgm16(os.path.join(a.out, "view_%02d_depth.pgm" % q), im["depth"])
    drawn = [float((im["index"] >= 0).mean()) for im in images]
    print("map of %d surfels at tick %d; %d views %dx%d written to %s/ (drawn share %.2f .. %.2f, large sprites %s)"
          % (info["count"], info["tick"], a.views, a.cols, a.rows, a.out, min(drawn), max(drawn), view.last_large_sprites(s, a.views)))


if __name__ == "__main__":
    main()
