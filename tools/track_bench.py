"""Region tracks (include/sf_tracks.h) on one MI355X: what following the regions of B QVGA frames in one call costs, beside
what labelling the same frames costs alone.

The frames are those of tools/region_bench.py: eight views of a room with a sphere, with the generator's camera poses. Slot q
sees view q % 8 and view (q + 1) % 8 in turn, so every timed update warps a previous frame into a consecutive view. Every figure
is the median of 5 calls, each bracketed by a synchronisation of the handle's stream, in one process with sf_microbench_copy
(the streaming ceiling of the box at that moment) before, between and after. The calls are the asynchronous device-pointer
forms on plain device memory: sft_update_images_device (which labels, counts overlaps, assigns and commits), and
sfr_label_images_device with label images alone on the same frames, so that what tracking adds to labelling is read off
directly. No result is copied to the host inside a bracket.

Byte model of what tracking adds per pixel: the overlap kernel reads the previous label and depth (8 bytes), the commit kernel
reads label and depth of the new frame (8) and writes the slot's label and depth (8), and an id image is 4 more. The gathers
at the warp targets and the records are not in the model.

NOT measured here: the stream form and the host form (they add copies to host memory), sizes other than QVGA, batches other
than --streams, max_tracks other than --max-tracks (the overlap table of an entry has max_tracks^2 words and the global-atomic
path begins past 4096 pairs), and the time of each kernel (a run under a kernel-tracing profiler gives it).

usage: python tools/track_bench.py [--streams 4096] [--max-tracks 16] [--json FILE]
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
from staticfusion_amd import regions, tracks
from staticfusion_amd.synth import FOVH, sequence_trajectory
from view_bench import median_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--max-tracks", type=int, default=16)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    api = sf.load()
    rt = C.CDLL(sf.LIB)  # the HIP runtime the library is bound to
    rows, cols, n, m = 240, 320, a.streams, a.max_tracks
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
    d_ids, d_lab = dev(n * px * 4), dev(n * px * 4)
    d_sum, d_trk = dev(n * tracks.SUMMARY_DTYPE.itemsize), dev(n * m * tracks.TRACK_DTYPE.itemsize)
    d_rsum, d_rreg = dev(n * regions.SUMMARY_DTYPE.itemsize), dev(n * m * regions.REGION_DTYPE.itemsize)
    # the argument arrays are made once: a bracket then holds the call and not the making of ctypes arrays
    tb, rb = tracks._bind(api), regions._bind(api)
    slots = (C.c_int32 * n)(*range(n))
    views = [[(q + step) % 8 for q in range(n)] for step in range(2)]
    depth_ptrs = [(C.c_void_p * n)(*[d_img[0] + v * px * 4 for v in views[step]]) for step in range(2)]
    b_ptrs = [(C.c_void_p * n)(*[d_img[1] + v * px * 4 for v in views[step]]) for step in range(2)]
    cams = [(tracks.SftCamera * n)(*[cam_of[v] for v in views[step]]) for step in range(2)]
    id_ptrs = (C.c_void_p * n)(*[d_ids + q * px * 4 for q in range(n)])
    lab_ptrs = (C.c_void_p * n)(*[d_lab + q * px * 4 for q in range(n)])
    rp = (regions.SfrParams * n)(*[regions.Params()] * n)
    tp = (tracks.SftParams * n)(*[tracks.Params()] * n)
    tracker = tracks.Tracker(s, n, m)
    turn = [0]

    def update(with_ids):
        step = turn[0] & 1
        turn[0] += 1
        tb.check(tb.update_images_device(tracker.t, rows, cols, n, slots, depth_ptrs[step], b_ptrs[step], cams[step], rp, tp, d_sum, d_trk, id_ptrs if with_ids else None),
                 "update_images_device")

    def label():
        rb.check(rb.label_images_device(s.h, rows, cols, n, depth_ptrs[1], b_ptrs[1], rp, m, d_rsum, d_rreg, lab_ptrs), "label_images_device")

    res = dict(streams=n, rows=rows, cols=cols, max_tracks=m, calls=5)
    copy = [s.microbench_copy(256 << 20, 10)]
    cases = {}
    update(False)  # every slot holds a previous frame from here on
    for name, fn, extra in (("label_alone", label, 0), ("update", lambda: update(False), 24), ("update_id_images", lambda: update(True), 28)):
        ms = median_ms(s, fn)
        copy.append(s.microbench_copy(256 << 20, 10))
        cases[name] = dict(ms=round(ms, 3), added_model_bytes=int(n * px * extra))
    summ = np.zeros(n, tracks.SUMMARY_DTYPE)
    assert rt.hipMemcpy(summ.ctypes.data_as(C.c_void_p), C.c_void_p(d_sum), C.c_size_t(summ.nbytes), 2) == 0
    assert all(summ[q][k] == summ[q % 8][k] for q in range(n) for k in ("n_regions", "n_tracked", "n_matched", "n_warped"))  # ids differ by history only
    mid = float(np.median(copy))
    res["copy_gbs"] = [round(c, 1) for c in copy]
    for k in ("update", "update_id_images"):
        c = cases[k]
        c["added_ms"] = round(c["ms"] - cases["label_alone"]["ms"], 3)
        c["added_model_gbs"] = round(c["added_model_bytes"] / max(c["added_ms"], 1e-6) / 1e6, 1)
        c["fraction_of_copy"] = round(c["added_model_gbs"] / mid, 3)
    res["cases"] = cases
    res["per_frame"] = {k: round(float(summ[k][:8].mean()), 1) for k in ("n_regions", "n_tracked", "n_matched", "n_warped")}
    print("%d frames %dx%d, max_tracks %d; device copy %s GB/s; per frame %s" % (n, cols, rows, m, res["copy_gbs"], res["per_frame"]))
    print("sfr_label_images_device alone (labels)   %8.3f ms" % cases["label_alone"]["ms"])
    for k in ("update", "update_id_images"):
        c = cases[k]
        print("sft_update_images_device %-16s %8.3f ms = labelling + %.3f ms; added byte model %.2f GB = %.0f GB/s = %.3f of the copy rate"
              % (k, c["ms"], c["added_ms"], c["added_model_bytes"] / 1e9, c["added_model_gbs"], c["fraction_of_copy"]))
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    tracker.close()
    for p in blocks:
        rt.hipFree(p)
    s.close()


if __name__ == "__main__":
    main()
