"""Moving regions (include/sf_regions.h) on one MI355X: what labelling B QVGA frames in one call costs, with and without
label images, under connectivity 4 and 8.

Every figure is the median of 5 calls of sfr_label_images_device, each bracketed by a synchronisation of the handle's
stream, in one process with sf_microbench_copy (the streaming ceiling of the box at that moment) before, between and after.
The call is the asynchronous device-pointer form on plain device memory, so a figure holds the upload of the entry table and
the seven launches and nothing else: no result is copied to the host inside the bracket.

Byte model: 8 bytes per pixel read (depth and b, once each) and 4 bytes per pixel written when labels are asked for. That
is what a labelling that kept everything on chip would move. The rate is set beside the copy rate (bytes read + bytes written
per second of a plain 16-byte copy): the fraction says how much of a streaming kernel's bandwidth the call reaches. The
traffic on the provisional labels and counts in the call's scratch is counted separately (scratch_bytes_model): per pixel,
pass 1 writes 8 bytes, pass 3 reads 4 and writes up to 4, passes 4 and 6 read 8 each, and pass 7 reads 4 and reads depth
and b of the masked pixels a second time.

The frames are eight views of a room with a sphere; b is low on the sphere and on 3 % of the other pixels (salt noise, so
that there are many small components beside the large one).

NOT measured here: the stream form and the host form (they add copies to host memory), sizes other than QVGA, batches other
than --streams, and frames with other mask shares. The time of each pass is not measured here either: a run of this tool
under a kernel-tracing profiler gives it (profiles/r16a_region_kernel_times.txt).

usage: python tools/region_bench.py [--streams 4096] [--max-regions 16] [--json FILE]
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
from staticfusion_amd import regions
from staticfusion_amd.synth import _render_sequence_frame, sequence_trajectory
from view_bench import median_ms


def frames_with_a_sphere(rows, cols, count):
    poses, offsets = sequence_trajectory(1000, count * 4)
    rng = np.random.default_rng(3)
    out = []
    for k in range(count):
        job = (1000, poses[4 * k], offsets[4 * k], True, 2 * cols, 2 * rows)
        depth = _render_sequence_frame(job)[0]
        behind = _render_sequence_frame(job[:3] + (False,) + job[4:])[0]
        b = np.where(depth != behind, 0.1, 0.9).astype(np.float32)
        b[rng.random(b.shape) < 0.03] = 0.2
        out.append((np.asarray(depth, np.float32), b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--max-regions", type=int, default=16)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    api = sf.load()
    rt = C.CDLL(sf.LIB)  # the HIP runtime the library is bound to
    rows, cols, n, m = 240, 320, a.streams, a.max_regions
    px = rows * cols
    s = sf.Solver(api, rows, cols, 1, api.default_params_struct())  # (the handle only owns the stream and the scratch here)
    frames = frames_with_a_sphere(rows, cols, 8)
    blocks = []

    def dev(nbytes):
        p = C.c_void_p()
        assert rt.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0, "hipMalloc of %d bytes" % nbytes
        blocks.append(p)
        return p.value

    d_depth, d_b, d_lab = dev(n * px * 4), dev(n * px * 4), dev(n * px * 4)
    d_sum, d_reg = dev(n * regions.SUMMARY_DTYPE.itemsize), dev(n * m * regions.REGION_DTYPE.itemsize)
    for k in range(2):
        tile = np.concatenate([np.ascontiguousarray(f[k].T).ravel() for f in frames])  # eight column-major images
        for q0 in range(0, n, 8):
            cnt = min(8, n - q0)
            assert rt.hipMemcpy(C.c_void_p((d_depth, d_b)[k] + q0 * px * 4), tile.ctypes.data_as(C.c_void_p), C.c_size_t(cnt * px * 4), 1) == 0
    # the argument arrays are made once: a bracket then holds the call and not the making of three ctypes arrays
    bind = regions._bind(api)
    depth_ptrs = (C.c_void_p * n)(*[d_depth + q * px * 4 for q in range(n)])
    b_ptrs = (C.c_void_p * n)(*[d_b + q * px * 4 for q in range(n)])
    lab_ptrs = (C.c_void_p * n)(*[d_lab + q * px * 4 for q in range(n)])
    res = dict(streams=n, rows=rows, cols=cols, max_regions=m, calls=5)
    copy = [s.microbench_copy(256 << 20, 10)]
    cases = {}
    for conn in (4, 8):
        for with_labels in (False, True):
            params = (regions.SfrParams * n)(*[regions.Params(connectivity=conn)] * n)

            def call():
                bind.check(bind.label_images_device(s.h, rows, cols, n, depth_ptrs, b_ptrs, params, m, d_sum, d_reg, lab_ptrs if with_labels else None),
                           "label_images_device")

            ms = median_ms(s, call)
            copy.append(s.microbench_copy(256 << 20, 10))
            model = n * px * (8 + (4 if with_labels else 0))
            cases["conn%d_%s" % (conn, "labels" if with_labels else "records")] = dict(ms=round(ms, 3), model_bytes=int(model), model_gbs=round(model / (ms * 1e-3) / 1e9, 1))
    # what the last call (connectivity 8, labels) found, against NumPy's count of the mask
    summ = np.zeros(n, regions.SUMMARY_DTYPE)
    assert rt.hipMemcpy(summ.ctypes.data_as(C.c_void_p), C.c_void_p(d_sum), C.c_size_t(summ.nbytes), 2) == 0
    masks = [int(((f[0] > 0) & (f[0] <= 8.0) & (f[1] < 0.5)).sum()) for f in frames]
    assert all(int(summ["n_mask"][q]) == masks[q % 8] for q in range(n)) and all(summ[q].tobytes() == summ[q % 8].tobytes() for q in range(n))
    mid = float(np.median(copy))
    res["copy_gbs"] = [round(c, 1) for c in copy]
    for k, c in cases.items():
        c["fraction_of_copy"] = round(c["model_gbs"] / mid, 3)
    res["cases"] = cases
    res["mask_share"] = round(float(np.mean(masks)) / px, 4)
    res["components_per_frame"] = round(float(summ["n_components"][:8].mean()), 1)
    res["regions_per_frame"] = round(float(summ["n_regions"][:8].mean()), 1)
    # per pixel: pass 1 writes labels + counts (8), pass 3 reads labels (4), passes 4 and 6 read both (16), pass 7 reads labels (4)
    # and depth + b of the masked pixels again (8 x mask share)
    res["scratch_bytes_model"] = int(n * px * (8 + 4 + 16 + 4 + 8 * res["mask_share"]))
    print("%d frames %dx%d, max_regions %d; device copy %s GB/s; mask share %.3f, %.0f components and %.1f regions per frame"
          % (n, cols, rows, m, res["copy_gbs"], res["mask_share"], res["components_per_frame"], res["regions_per_frame"]))
    for k, c in cases.items():
        print("sfr_label_images_device %-14s %8.3f ms, byte model %.2f GB = %.0f GB/s = %.3f of the copy rate"
              % (k, c["ms"], c["model_bytes"] / 1e9, c["model_gbs"], c["fraction_of_copy"]))
    print("scratch traffic by its own model: %.2f GB per call (not in the figures above)" % (res["scratch_bytes_model"] / 1e9))
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    for p in blocks:
        rt.hipFree(p)
    s.close()


if __name__ == "__main__":
    main()
