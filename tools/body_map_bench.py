"""Body maps (include/sf_body_maps.h) on one MI355X: what fusing the moving regions of B QVGA frames into B maps costs in one call.

The frames are those of tools/region_bench.py: eight views of a room with a sphere, with the generator's camera poses. The eight
views are labelled once (sfr_label_images_device; the label images stay on the device); entry q fuses the largest region of view
q % 8 into a map of its own, with W = NULL and the parameters of sfp_default_params. The call is the device-pointer form,
sfp_fuse_images_device, on plain device memory; it returns after the counts are back on the host, so every bracket holds one
host synchronisation by construction. The warm-up call is the FIRST SIGHTING (every winner is added); the figure is the median of
the 5 calls that follow, which see the same frame again (winners are merged), in one process with sf_microbench_copy (the
streaming ceiling of the box at that moment) before and after.

Byte model per entry, from the counts of the call: both pixel passes read every label (8 bytes per pixel); a pixel of the
region costs its depth once (the four neighbours are its neighbours' own loads), the write and the read of its slot and, for the
colour, nothing (no colour image is given): 12 bytes; the tables are cleared at 20 bytes per slot; a surfel is read by the insert
(16 bytes) and read and written by the move (96 bytes). The probes and atomics on the tables, the block counts and the entry
tables are not in the model.

NOT measured here: the host form (it adds the uploads), sizes other than QVGA, colour images, motions other than the identity,
a first sighting in the timed calls, and the time of each kernel (a run under a kernel-tracing profiler gives it).

usage: python tools/body_map_bench.py [--entries 256] [--max-regions 8] [--json FILE]
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
from staticfusion_amd import body_maps, join, regions, tracks
from staticfusion_amd.synth import FOVH, sequence_trajectory
from view_bench import median_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=256)
    ap.add_argument("--max-regions", type=int, default=8)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    api = sf.load()
    rt = C.CDLL(sf.LIB)  # the HIP runtime the library is bound to
    rows, cols, n, m = 240, 320, a.entries, a.max_regions
    px = rows * cols
    s = sf.Solver(api, rows, cols, 1, api.default_params_struct())  # (the handle only owns the stream and the scratch here)
    frames = frames_with_a_sphere(rows, cols, 8)
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
    rsum, rreg = np.zeros(8, regions.SUMMARY_DTYPE), np.zeros((8, m), regions.REGION_DTYPE)
    assert rt.hipMemcpy(rsum.ctypes.data_as(C.c_void_p), C.c_void_p(d_rsum), C.c_size_t(rsum.nbytes), 2) == 0
    assert rt.hipMemcpy(rreg.ctypes.data_as(C.c_void_p), C.c_void_p(d_rreg), C.c_size_t(rreg.nbytes), 2) == 0
    label_of = [int(np.argmax(rreg[v]["n"])) + 1 for v in range(8)]  # the largest region of the view
    maps = [sf.SurfelMap(s, px) for _ in range(n)]
    # the argument arrays are made once: a bracket then holds the call and not the making of ctypes arrays
    b = body_maps._bind(api)
    views = [q % 8 for q in range(n)]
    z = (C.c_void_p * n)(*[d_img[0] + v * px * 4 for v in views])
    lab = (C.c_void_p * n)(*[d_lab + v * px * 4 for v in views])
    cams = (body_maps.SfpCamera * n)(*[cam_of[v] for v in views])
    ts = (C.c_int32 * n)(*[label_of[v] for v in views])
    mptr = (C.c_void_p * n)(*[mm.m.value for mm in maps])
    ps = (body_maps.SfpParams * n)(*[body_maps.Params()] * n)
    out = (body_maps.SfpCounts * n)()
    history = []

    def fuse():
        b.check(b.fuse_images_device(s.h, rows, cols, n, z, lab, None, cams, ts, mptr, None, ps, out), "fuse_images_device")
        history.append([out[q].as_dict() for q in range(8)])

    copy = [s.microbench_copy(256 << 20, 10)]
    ms = median_ms(s, fuse)
    copy.append(s.microbench_copy(256 << 20, 10))
    assert all(out[q].as_dict() == out[q % 8].as_dict() for q in range(n))  # the counts are a function of the entry alone
    first, again = history[0], history[-1]
    per_view = []
    for v in range(8):
        c = again[v]
        count_in = c["n_out"] - c["n_added"]
        slots = join.table_slots(count_in + (rows - 2) * (cols - 2))
        per_view.append(px * 8 + c["n_pixels"] * 12 + slots * 20 + count_in * 112)
    model_bytes = int(sum(per_view[q % 8] for q in range(n)))
    mid = float(np.median(copy))
    res = dict(entries=n, rows=rows, cols=cols, max_regions=m, calls=5, ms=round(ms, 3), us_per_entry=round(1e3 * ms / n, 2), model_bytes=model_bytes,
               model_gbs=round(model_bytes / ms / 1e6, 1), copy_gbs=[round(c, 1) for c in copy], fraction_of_copy=round(model_bytes / ms / 1e6 / mid, 3),
               region_label=label_of, first_sighting=first, last_call=again)
    print("%d entries %dx%d; device copy %s GB/s" % (n, cols, rows, res["copy_gbs"]))
    print("sfp_fuse_images_device (a frame seen again)   %8.3f ms = %.1f us per entry; byte model %.2f GB = %.0f GB/s = %.3f of the copy rate"
          % (ms, 1e3 * ms / n, model_bytes / 1e9, res["model_gbs"], res["fraction_of_copy"]))
    print("of the eight distinct entries, first sighting: pixels %s added %s; last call: surfels %s merged %s added %s conflict %s"
          % ([c["n_pixels"] for c in first], [c["n_added"] for c in first], [c["n_out"] for c in again], [c["n_merged"] for c in again], [c["n_added"] for c in again],
             [c["n_conflict"] for c in again]))
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    for mm in maps:
        mm.close()
    for p in blocks:
        rt.hipFree(p)
    s.close()


if __name__ == "__main__":
    main()
