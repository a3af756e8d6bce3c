"""How did it move (include/sf_bodies.h): the moving-sphere sequences of tools/moving_regions.py go through predict -> load ->
solve -> fuse, and after every solve the moving regions of every stream are labelled (sfr_label_streams), followed
(sft_update_streams) and, from the second labelled frame on, aligned with the frame before (sfb_estimate_images, paired by the
tracks: region t of the earlier frame must land on the region its track went to), all with the ground-truth camera poses the
generator gives. Per stream and frame the tool prints, for the largest track that has a previous frame, the world motion W
applied to the track's previous centroid as a displacement beside the generator's true displacement of the sphere, and the
misfit of the "did not move" hypothesis (ss_first / n_first) beside the misfit after the steps (ss_last / n_last), as rms in mm.

A sphere's rotation about its centre is not observable by point-to-plane: the run uses a small non-zero damping, which keeps
the unobservable directions at zero, and reports TRANSLATION ONLY. The figures are what they are on these synthetic walks;
nothing is tuned on them.

usage: python tools/body_motion.py [--sequences 4] [--frames 10] [--min-pixels 16] [--damping 1e-4] [--json FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

import staticfusion_amd as sf
from moving_regions import as_sensor_frame
from staticfusion_amd import bodies, regions, tracks
from staticfusion_amd.synth import FOVH, make_sequence, sequence_trajectory


def rms_mm(n, ss):
    return 1000.0 * float(np.sqrt(float(ss) / n)) / 65536.0 if n > 0 else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=4)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--min-pixels", type=int, default=16)
    ap.add_argument("--damping", type=float, default=1e-4)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    api = sf.load()
    rows, cols, n, M = 240, 320, a.sequences, 8
    s = sf.Solver(api, rows, cols, n, api.default_params_struct())
    maps = [sf.SurfelMap(s, 4 * rows * cols) for _ in range(n)]
    mp = s.default_model_params()
    streams = list(range(n))
    seqs = [make_sequence(1000 + q, a.frames, sphere=True, out_rows=rows, out_cols=cols) for q in range(n)]
    walks = [sequence_trajectory(1000 + q, a.frames) for q in range(n)]  # (camera-to-world poses, sphere offsets)
    f = cols / (2.0 * np.tan(0.5 * FOVH))  # the generator's camera at the solver's resolution
    cx, cy = (cols - 1) / 2.0, (rows - 1) / 2.0
    tracker = tracks.Tracker(s, n, M)
    rp, tp, bp = regions.Params(min_pixels=a.min_pixels), tracks.Params(), bodies.Params(damping=a.damping)
    out, before = [], None  # before: (depths, labels, cameras, track records) of the last labelled frame

    def report(k):
        nonlocal before
        cams = [tracks.Camera(walks[q][0][k], cx, cy, f, f) for q in range(n)]
        depth = [s.current(q)[0] for q in range(n)]
        labels = regions.label_streams(s, streams, rp, M, labels=True)[2]
        summ, recs = tracker.update_streams(streams, streams, cams, rp, tp)
        if before is not None:
            z0, l0, c0, r0 = before
            pairs = np.array([bodies.pairs_from_tracks(recs[q], M) for q in range(n)])
            mot = bodies.estimate_images(s, z0, l0, depth, labels, c0, cams, [len(r0[q]) for q in range(n)], pairs, bp, M)
            for q in range(n):
                kept = [r for r in recs[q] if int(r["prev_region"]) > 0]
                truth = np.asarray(walks[q][1][k], np.float64) - np.asarray(walks[q][1][k - 1], np.float64)
                rec = dict(frame=k, stream=q, true_displacement=[round(float(x), 4) for x in truth])
                if kept:
                    big = max(kept, key=lambda r: int(r["n"]))
                    t = int(big["prev_region"])
                    m = mot[q, t - 1]
                    was = tracks.centroids(r0[q])[t - 1]
                    moved = bodies.apply(m["w"], was) - was
                    rec.update(id=int(big["id"]), status=int(m["status"]), iterations_done=int(m["iterations_done"]), n_first=int(m["n_first"]), n_last=int(m["n_last"]),
                               rms_first_mm=round(rms_mm(int(m["n_first"]), int(m["ss_first"])), 3), rms_last_mm=round(rms_mm(int(m["n_last"]), int(m["ss_last"])), 3),
                               displacement=[round(float(x), 4) for x in moved], error_m=round(float(np.linalg.norm(moved - truth)), 4))
                    print("%5d %6d | id %d status %d after %2d steps | W on the centroid (%s) true (%s): off by %.4f m | did-not-move rms %7.3f mm on %5d px, after %7.3f mm on %5d px"
                          % (k, q, rec["id"], rec["status"], rec["iterations_done"], ", ".join("%+.4f" % x for x in moved), ", ".join("%+.4f" % x for x in truth),
                             rec["error_m"], rec["rms_first_mm"], rec["n_first"], rec["rms_last_mm"], rec["n_last"]))
                else:
                    print("%5d %6d | no track with a previous frame" % (k, q))
                out.append(rec)
        before = (depth, labels, cams, recs)

    print("frame stream | sfb_estimate_images on the largest followed region (damping %g, other parameters the defaults of sfb_default_params); translation only" % a.damping)
    for q in range(n):
        s.load_frame(q, *as_sensor_frame(*seqs[q]["frames"][0]), 1)
    s.current_to_prediction()
    s.push_history(0)
    s.set_kb(1.05)
    for q in range(n):
        s.load_frame(q, *as_sensor_frame(*seqs[q]["frames"][1]), 1)
    s.process_frame(1)
    Tq = s.batch_results()[0]
    report(1)
    s.filter_depth()
    sf.SurfelMap.fuse_frames(s, streams, maps, list(Tq), 1.0, mp)
    for k in range(2, a.frames):
        s.set_kb(1.05 if k == 2 else 1.5)
        sf.SurfelMap.predict_frames(s, streams, maps, mp)
        for q in range(n):
            s.load_frame(q, *as_sensor_frame(*seqs[q]["frames"][k]), 1)
        s.filter_depth()
        s.process_frame(k)
        Tq = s.batch_results()[0]
        report(k)
        sf.SurfelMap.fuse_frames(s, streams, maps, list(Tq), 1.0, mp)
    errs = [r["error_m"] for r in out if "error_m" in r]
    if errs:
        print("%d motions: the displacement of W is off by a median of %.4f m, at most %.4f m; the true displacements are %.4f m long in the median"
              % (len(errs), float(np.median(errs)), max(errs), float(np.median([np.linalg.norm(r["true_displacement"]) for r in out if "error_m" in r]))))
    res = dict(sequences=n, frames=a.frames, min_pixels=a.min_pixels, damping=a.damping, rows=rows, cols=cols, records=out)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    tracker.close()
    for m in maps:
        m.close()
    s.close()


if __name__ == "__main__":
    main()
