"""Is it the same thing that moved a frame ago, and where is it in the room (include/sf_tracks.h): the moving-sphere sequences
of tools/moving_regions.py go through predict -> load -> solve -> fuse, and after every solve ONE sft_update_streams call
follows the moving regions of every stream, with the ground-truth camera poses the generator gives. Per stream and frame the
tool prints the ids, ages and overlaps of the tracks, the world centroid of the largest track against the sphere's true centre
(the centroid is of the visible cap, so it lies up to a radius, 0.25 m, nearer the camera), and at the end whether the sphere
kept one id over the frames.

The figures are what they are on these synthetic walks; nothing is tuned on them.

usage: python tools/track_regions.py [--sequences 4] [--frames 10] [--min-pixels 16] [--json FILE]
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
from staticfusion_amd import regions, tracks
from staticfusion_amd.synth import FOVH, Scene, make_sequence, sequence_trajectory


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=4)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--min-pixels", type=int, default=16)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    api = sf.load()
    rows, cols, n = 240, 320, a.sequences
    s = sf.Solver(api, rows, cols, n, api.default_params_struct())
    maps = [sf.SurfelMap(s, 4 * rows * cols) for _ in range(n)]
    mp = s.default_model_params()
    streams = list(range(n))
    seqs = [make_sequence(1000 + q, a.frames, sphere=True, out_rows=rows, out_cols=cols) for q in range(n)]
    walks = [sequence_trajectory(1000 + q, a.frames) for q in range(n)]  # (camera-to-world poses, sphere offsets)
    centre0 = Scene(sphere=True).sphere_c0
    f = cols / (2.0 * np.tan(0.5 * FOVH))  # the generator's camera at the solver's resolution
    cx, cy = (cols - 1) / 2.0, (rows - 1) / 2.0
    tracker = tracks.Tracker(s, n, 8)
    rp, tp = regions.Params(min_pixels=a.min_pixels), tracks.Params()
    out, ids_seen = [], [[] for _ in range(n)]

    def report(k):
        cams = [tracks.Camera(walks[q][0][k], cx, cy, f, f) for q in range(n)]
        summ, recs = tracker.update_streams(streams, streams, cams, rp, tp)
        for q in range(n):
            truth = centre0 + np.asarray(walks[q][1][k], np.float64)
            cen = tracks.centroids(recs[q])
            big = int(np.argmax(recs[q]["n"])) if len(recs[q]) else -1
            ids_seen[q].append(int(recs[q]["id"][big]) if big >= 0 else 0)
            err = float(np.linalg.norm(cen[big] - truth)) if big >= 0 else float("nan")
            rec = dict(frame=k, stream=q, summary={key: int(summ[key][q]) for key in tracks.SUMMARY_FIELDS},
                       tracks=[dict(id=int(r["id"]), age=int(r["age"]), overlap=int(r["overlap"]), n=int(r["n"]), centroid=[round(float(x), 3) for x in cen[j]])
                               for j, r in enumerate(recs[q])], sphere=[round(float(x), 3) for x in truth], largest_to_sphere_m=round(err, 3))
            out.append(rec)
            print("%5d %6d | %s | largest at (%s) sphere at (%s): %.3f m | matched %d born %d ended %d warped %d"
                  % (k, q, "; ".join("id %d age %d overlap %d of %d px" % (t["id"], t["age"], t["overlap"], t["n"]) for t in rec["tracks"]) or "-",
                     ", ".join("%.2f" % x for x in (cen[big] if big >= 0 else [np.nan] * 3)), ", ".join("%.2f" % x for x in truth), err, summ["n_matched"][q],
                     summ["n_born"][q], summ["n_ended"][q], summ["n_warped"][q]))

    print("frame stream | tracks of sft_update_streams (b < %.2f, >= %d px; defaults of sft_default_params) | world centroid against the sphere's centre" % (rp.b_max, rp.min_pixels))
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
    kept = []
    for q in range(n):
        one = len(set(ids_seen[q])) == 1 and ids_seen[q][0] > 0
        kept.append(one)
        print("stream %d: the largest track had the ids %s over %d frames: %s" % (q, ids_seen[q], len(ids_seen[q]), "one id" if one else "NOT one id"))
    res = dict(sequences=n, frames=a.frames, min_pixels=a.min_pixels, b_max=rp.b_max, rows=rows, cols=cols, ids_of_largest=ids_seen, kept_one_id=kept, records=out)
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
