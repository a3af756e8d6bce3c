"""Free-view rendering (include/sf_view.h) on one MI355X: what a render costs beside the prediction of the same maps.

The maps are what tools/full_pipeline_bench.py leaves: N sequences through predict -> input -> solve -> fuse for 10 QVGA frames
of a synthetic walk (about 75 k surfels each). Every figure is the median of 5 calls, each bracketed by a synchronisation of
the handle's stream, in one process with sf_microbench_copy (the streaming ceiling of the box at that moment).

  (a) N maps, one 320 x 240 view each from the map's own pose, into device memory and into host memory; the yardstick is
      sf_map_predict_frames on the same maps (two targets and a fill-in, into the streams' prediction slots)
  (b) one map, 64 orbit views at 640 x 480
  (c) the same orbit at 1280 x 960 with a near pass: the large-sprite path; reports the lengths of the large-sprite lists
  and the route a user had before: sf_map_download + the NumPy renderer of tests/view_ref.py, on one map, as a multiple.

usage: python tools/view_bench.py [--streams 256] [--frames 10] [--skip-numpy] [--json FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import staticfusion_amd as sf
from staticfusion_amd import view
from staticfusion_amd.synth import Scene, se3_exp


def build_maps(api, n, n_frames):
    """the loop of tools/full_pipeline_bench.py, untimed"""
    rows, cols, res = 240, 320, 2
    s = sf.Solver(api, rows, cols, n, api.default_params_struct())
    maps = [sf.SurfelMap(s, 4 * rows * cols) for _ in range(n)]
    mp = s.default_model_params()
    streams = list(range(n))
    scene = Scene(seed=77, sphere=False)
    xi = np.array([0.010, 0.004, 0.006, 0.002, -0.004, 0.003]) * 0.6
    T = np.eye(4)
    for k in range(n_frames):
        depth, inten = scene.render(T, 640, 480)
        g = np.clip(np.rint(inten * 255), 0, 255).astype(np.uint8)
        col = np.ascontiguousarray(np.repeat(g[::-1, :, None], 3, axis=2))
        dep = np.ascontiguousarray(np.clip(np.rint(depth[::-1] * 1000), 0, 65535).astype(np.uint16))
        if k >= 2:  # the prediction fills in from the PREVIOUS frame: before the load
            s.set_kb(1.05 if k == 2 else 1.5)
            sf.SurfelMap.predict_frames(s, streams, maps, mp)
        for b in range(n):
            s.load_frame(b, col, dep, res)
        if k == 0:
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
            sf.SurfelMap.fuse_frames(s, streams, maps, list(Tq), 1.0, mp)
        T = T @ se3_exp(xi)
    return s, maps, mp


def median_ms(s, fn, calls=5):
    fn()  # warm-up: scratch growth, code objects
    s.synchronize()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        s.synchronize()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


class DeviceImages:
    """depth / rgb / index buffers for a list of views, in plain device memory of the library's HIP runtime"""

    def __init__(self, views):
        self.rt = C.CDLL(sf.LIB)
        self.ptrs = []
        for v in views:
            px = v.rows * v.cols
            row = []
            for nbytes in (px * 4, px * 3, px * 4):
                p = C.c_void_p()
                assert self.rt.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
                row.append(p)
            self.ptrs.append(row)

    def lists(self):
        return [[r[k].value for r in self.ptrs] for k in range(3)]

    def free(self):
        for r in self.ptrs:
            for p in r:
                self.rt.hipFree(p)


def orbit(n_views, rows, cols, centre, radius, near=None):
    """n_views cameras on a circle around `centre` looking at it; with `near`, every fourth stands that close to the surface"""
    f = 0.9 * cols
    out = []
    for q in range(n_views):
        ang = 2 * np.pi * q / n_views
        r = near if (near is not None and q % 4 == 0) else radius
        eye = centre + np.array([r * np.sin(ang) * 0.6, -0.2 * r * np.cos(ang), -r * (0.6 + 0.4 * np.cos(ang))])
        out.append(view.View(view.look_at(eye, centre), cols / 2, rows / 2, f, f, rows, cols, min_confidence=0.0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--skip-numpy", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    api = sf.load()
    s, maps, mp = build_maps(api, a.streams, a.frames)
    n = len(maps)
    counts = [m.info()["count"] for m in maps]
    res = dict(streams=n, frames=a.frames, surfels_per_map=int(np.median(counts)), copy_gbs=round(s.microbench_copy(256 << 20, 10), 1))
    print("%d maps, median %d surfels; device copy %.0f GB/s" % (n, res["surfels_per_map"], res["copy_gbs"]))
    streams = list(range(n))

    # (a)
    res["a_predict_ms"] = median_ms(s, lambda: sf.SurfelMap.predict_frames(s, streams, maps, mp))
    own = [view.default_view(s, m) for m in maps]
    dev = DeviceImages(own)
    res["a_render_device_ms"] = median_ms(s, lambda: view.render_device(maps, own, *dev.lists()))
    res["a_large_sprites"] = int(sum(view.last_large_sprites(s, n)))
    res["a_render_device_depth_only_ms"] = median_ms(s, lambda: view.render_device(maps, own, dev.lists()[0], None, None))
    dev.free()
    res["a_render_host_ms"] = median_ms(s, lambda: view.render(maps, own))
    px = n * 240 * 320
    model = sum(counts) * 48 + px * (8 + 8 + 19)
    res["a_model_bytes"] = int(model)
    res["a_model_gbs"] = round(model / (res["a_render_device_ms"] * 1e-3) / 1e9, 1)
    print("(a) %d views 320x240: predict_frames %.3f ms | render to device %.3f ms (depth only %.3f) | to host %.3f ms | byte model %.1f MB -> %.0f GB/s"
          % (n, res["a_predict_ms"], res["a_render_device_ms"], res["a_render_device_depth_only_ms"], res["a_render_host_ms"], model / 1e6, res["a_model_gbs"]))

    # (b), (c)
    surf = maps[0].download()
    centre = np.median(surf[:, :3], axis=0).astype(np.float64)
    for tag, rows, cols, near in (("b", 480, 640, None), ("c", 960, 1280, 0.45)):
        views = orbit(64, rows, cols, centre, 1.6, near)
        dev = DeviceImages(views)
        ms = median_ms(s, lambda: view.render_device([maps[0]] * 64, views, *dev.lists()))
        large = view.last_large_sprites(s, 64)
        dev.free()
        res[tag + "_render_device_ms"] = ms
        res[tag + "_large_sprites_total"] = int(sum(large))
        res[tag + "_large_sprites_max"] = int(max(large))
        print("(%s) 1 map x 64 orbit views %dx%d: %.3f ms (%.3f ms per view); large-sprite lists: %d in all, longest %d"
              % (tag, cols, rows, ms, ms / 64, sum(large), max(large)))

    # the route without the renderer
    if not a.skip_numpy:
        import view_ref

        t0 = time.perf_counter()
        d = maps[0].download()
        ref = view_ref.render(d, own[0], tick=maps[0].info()["tick"])
        res["numpy_route_ms"] = 1e3 * (time.perf_counter() - t0)
        one = median_ms(s, lambda: view.render([maps[0]], [own[0]]))
        got = view.render([maps[0]], [own[0]])[0]
        res["one_view_host_ms"] = one
        res["numpy_equal"] = bool(np.array_equal(got["index"], ref["index"]) and np.array_equal(got["depth"].view(np.uint32), ref["depth"].view(np.uint32)))
        print("download + NumPy renderer, one map one view: %.0f ms = %.0f x sfv_render_maps (%.3f ms); images equal: %s"
              % (res["numpy_route_ms"], res["numpy_route_ms"] / one, one, res["numpy_equal"]))
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
