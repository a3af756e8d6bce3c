"""Region motion (include/sf_bodies.h) on one MI355X: what the rigid motions of the moving regions of B QVGA frame pairs cost in
one call.

The frames are those of tools/region_bench.py: eight views of a room with a sphere, with the generator's camera poses. The eight
views are labelled once (sfr_label_images_device; the label images stay on the device); pair q aligns the regions of view
q % 8 with view (q + 1) % 8, unpaired (any pixel of the later frame may be a target). The call is the asynchronous device-pointer
form, sfb_estimate_images_device, on plain device memory, with systems_out NULL and the parameters of sfb_default_params but
--damping (a sphere leaves three degrees unobservable). The figure is the median of 5 calls, each bracketed by a
synchronisation of the handle's stream, in one process with sf_microbench_copy (the streaming ceiling of the box at that moment)
before and after. No result is copied to the host inside a bracket.

Byte model per pixel of a pair: the model kernel reads depth and label of the later frame (8 bytes) and writes the 32-byte
model; each of the iterations + 1 linearisations reads label and depth of the earlier frame (8 bytes). The 32-byte gathers at
the warp targets (region pixels only), the systems and the records are not in the model, and a workgroup whose tile holds no
running region reads only its labels (4 bytes): the model is an upper figure for the streamed bytes.

NOT measured here: the host form (it adds copies to and from host memory), sizes other than QVGA, batches other than --pairs,
max_regions other than --max-regions, pairs given, systems_out given, and the time of each kernel (a run under a kernel-tracing
profiler gives it).

usage: python tools/body_bench.py [--pairs 4096] [--max-regions 8] [--damping 1e-4] [--json FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

import staticfusion_amd as sf
from region_bench import frames_with_a_sphere
from staticfusion_amd import bodies, regions, tracks
from staticfusion_amd.synth import FOVH, sequence_trajectory
from view_bench import median_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--max-regions", type=int, default=8)
    ap.add_argument("--damping", type=float, default=1e-4)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    api = sf.load()
    rt = C.CDLL(sf.LIB)  # the HIP runtime the library is bound to
    rows, cols, n, m = 240, 320, a.pairs, a.max_regions
    px = rows * cols
    s = sf.Solver(api, rows, cols, 1, api.default_params_struct())  # (the handle only owns the stream and the scratch here)
    frames = frames_with_a_sphere(rows, cols, 8)
    assert frames[0][0].shape == (rows, cols)
    poses = sequence_trajectory(1000, 32)[0]
    f = cols / (2.0 * np.tan(0.5 * FOVH))
    cam_of = [tracks.Camera(poses[4 * k], (cols - 1) / 2.0, (rows - 1) / 2.0, f, f) for k in range(8)]
    blocks = []

    def dev(nbytes):
        p = C.c_void_p()
        assert rt.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0, "hipMalloc of %d bytes" % nbytes
        blocks.append(p)
        return p.value

    d_img = [dev(8 * px * 4), dev(8 * px * 4)]  # the eight views once: depth, b
    for k in range(2):
        tile = np.concatenate([np.ascontiguousarray(fr[k].T).ravel() for fr in frames])
        assert rt.hipMemcpy(C.c_void_p(d_img[k]), tile.ctypes.data_as(C.c_void_p), C.c_size_t(tile.nbytes), 1) == 0
    d_lab = dev(8 * px * 4)
    d_rsum, d_rreg = dev(8 * regions.SUMMARY_DTYPE.itemsize), dev(8 * m * regions.REGION_DTYPE.itemsize)
    regions.label_images_device(s, rows, cols, [d_img[0] + v * px * 4 for v in range(8)], [d_img[1] + v * px * 4 for v in range(8)], [regions.Params()] * 8, m, d_rsum,
                                d_rreg, [d_lab + v * px * 4 for v in range(8)])
    s.synchronize()
    rsum = np.zeros(8, regions.SUMMARY_DTYPE)
    assert rt.hipMemcpy(rsum.ctypes.data_as(C.c_void_p), C.c_void_p(d_rsum), C.c_size_t(rsum.nbytes), 2) == 0
    k_of = [int(x) for x in rsum["n_written"]]
    d_mot = dev(n * m * bodies.MOTION_DTYPE.itemsize)
    # the argument arrays are made once: a bracket then holds the call and not the making of ctypes arrays
    b = bodies._bind(api)
    v0, v1 = [q % 8 for q in range(n)], [(q + 1) % 8 for q in range(n)]
    ptrs = lambda base, views: (C.c_void_p * n)(*[base + v * px * 4 for v in views])
    z0, l0, z1, l1 = ptrs(d_img[0], v0), ptrs(d_lab, v0), ptrs(d_img[0], v1), ptrs(d_lab, v1)
    c0, c1 = (bodies.SfbCamera * n)(*[cam_of[v] for v in v0]), (bodies.SfbCamera * n)(*[cam_of[v] for v in v1])
    ks = (C.c_int32 * n)(*[k_of[v] for v in v0])
    par = bodies.Params(damping=a.damping)
    ps = (bodies.SfbParams * n)(*[par] * n)

    def estimate():
        b.check(b.estimate_images_device(s.h, rows, cols, n, z0, l0, z1, l1, c0, c1, ks, None, ps, m, C.c_void_p(d_mot), None), "estimate_images_device")

    copy = [s.microbench_copy(256 << 20, 10)]
    ms = median_ms(s, estimate)
    copy.append(s.microbench_copy(256 << 20, 10))
    mot = np.zeros((n, m), bodies.MOTION_DTYPE)
    assert rt.hipMemcpy(mot.ctypes.data_as(C.c_void_p), C.c_void_p(d_mot), C.c_size_t(mot.nbytes), 2) == 0
    assert all(mot[q].tobytes() == mot[q % 8].tobytes() for q in range(n))  # a motion is a function of its pair alone
    its = int(par.iterations)
    model_bytes = int(n * px * (40 + (its + 1) * 8))
    mid = float(np.median(copy))
    live = [(q, t) for q in range(8) for t in range(k_of[q])]
    res = dict(pairs=n, rows=rows, cols=cols, max_regions=m, damping=a.damping, iterations=its, calls=5, ms=round(ms, 3), model_bytes=model_bytes,
               model_gbs=round(model_bytes / ms / 1e6, 1), copy_gbs=[round(c, 1) for c in copy], fraction_of_copy=round(model_bytes / ms / 1e6 / mid, 3),
               regions_per_pair=round(float(np.mean(k_of)), 2), dynamic_pixels_per_pair=round(float(np.mean(rsum["n_mask"])), 1),
               status_counts={str(c): int(sum(int(mot[q, t]["status"]) == c for q, t in live)) for c in (0, 1, 2)},
               iterations_done=[int(mot[q, t]["iterations_done"]) for q, t in live], n_first=[int(mot[q, t]["n_first"]) for q, t in live])
    print("%d pairs %dx%d, max_regions %d, %d iterations, damping %g; %.2f regions per pair; device copy %s GB/s" % (n, cols, rows, m, its, a.damping, res["regions_per_pair"], res["copy_gbs"]))
    print("sfb_estimate_images_device   %8.3f ms = %.1f us per pair; byte model %.2f GB = %.0f GB/s = %.3f of the copy rate" % (ms, 1e3 * ms / n, model_bytes / 1e9, res["model_gbs"], res["fraction_of_copy"]))
    print("of the eight distinct pairs: status counts %s, steps taken %s, pairs of the first linearisation %s" % (res["status_counts"], res["iterations_done"], res["n_first"]))
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    for p in blocks:
        rt.hipFree(p)
    s.close()


if __name__ == "__main__":
    main()
