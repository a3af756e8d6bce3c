"""Tracking health from pose scores (include/sf_score.h): the loop of tools/full_pipeline_bench.py on N synthetic sequences
(host frames, one scene per sequence), with every stream's current frame scored against its own map twice per frame, each time
in one sfs_score_streams call for all streams: BEFORE the fuse at the pose the solver returned (does the pose explain the frame?
the map does not hold the frame yet) and AFTER the fuse at the map's pose (the last two columns: by then the map has taken the
frame in, and agrees with it). At a chosen frame one stream is handed another sequence's frame ("kidnapped"); the table shows
what the counts do. For that stream the tool then ranks a grid of candidate poses around its
last good pose against the kidnapped frame's successor -- one call with the same map and the same stream repeated.

The figures are what they are on this synthetic walk: the parameter defaults of sfs_default_params are not acceptance
thresholds, and no threshold is applied here.

usage: python tools/track_health.py [--streams 4] [--frames 12] [--kidnap-frame 7] [--kidnap-stream 1] [--grid 5]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import staticfusion_amd as sf
from staticfusion_amd import score, view
from staticfusion_amd.synth import Scene, pose_delta, se3_exp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--kidnap-frame", type=int, default=7)
    ap.add_argument("--kidnap-stream", type=int, default=1)
    ap.add_argument("--grid", type=int, default=5, help="candidates per axis of the translation grid (x, y, z)")
    a = ap.parse_args()
    api = sf.load()
    rows, cols, res = 240, 320, 2
    n = a.streams
    s = sf.Solver(api, rows, cols, n, api.default_params_struct())
    maps = [sf.SurfelMap(s, 4 * rows * cols) for _ in range(n)]
    mp = s.default_model_params()
    streams = list(range(n))
    # a room of its own per sequence (the seed alone only changes the texture): another back wall, tilt and floor
    scenes = [Scene(seed=77 + 5 * q, sphere=False, wall_z=3.0 - 0.3 * (q % 4), tilt_deg=10.0 + 5.0 * (q % 4), floor_y=1.0 - 0.08 * (q % 4)) for q in range(n)]
    xi = np.array([0.010, 0.004, 0.006, 0.002, -0.004, 0.003]) * 0.6
    T, frames, gts = np.eye(4), [], []
    for k in range(a.frames):
        per = []
        for q in range(n):
            depth, inten = scenes[q].render(T, 640, 480)
            g = np.clip(np.rint(inten * 255), 0, 255).astype(np.uint8)
            per.append((np.ascontiguousarray(np.repeat(g[::-1, :, None], 3, axis=2)), np.ascontiguousarray(np.clip(np.rint(depth[::-1] * 1000), 0, 65535).astype(np.uint16))))
        frames.append(per)
        gts.append(T.copy())
        T = T @ se3_exp(xi)
    victim, donor = a.kidnap_stream % n, (a.kidnap_stream + 1) % n

    def load(k):
        for q in range(n):
            src = donor if (k == a.kidnap_frame and q == victim) else q
            s.load_frame(q, *frames[k][src], res)

    def before_fuse(Tq):
        """every stream's frame against its map as it is, seen from the pose the solver returned"""
        vs = [view.default_view(s, m) for m in maps]
        for q, v in enumerate(vs):
            v.pose[:] = [float(x) for x in np.asarray(Tq[q], np.float32).T.ravel()]
        return score.score_streams(maps, vs, streams)

    def health(k, rec):
        after = score.score_streams(maps, [view.default_view(s, m) for m in maps], streams)
        d, da = score.derived(rec), score.derived(after)
        for q in range(n):
            mark = " <- kidnapped" if (k == a.kidnap_frame and q == victim) else ""
            print("%5d %6d %8d %8d %8d %7d %7d %8.3f %8.3f %9.4f | %8d %8.3f%s"
                  % (k, q, rec["n_frame"][q], rec["n_masked"][q], rec["n_both"][q], rec["n_front"][q], rec["n_behind"][q], d["inlier_ratio"][q], d["overlap"][q],
                     d["mean_abs"][q], after["n_both"][q], da["inlier_ratio"][q], mark))

    def relocalise(k, last_good, rec, Tq):
        """the victim's own frame again: which pose near its last good one explains it? A translation grid of two frames' reach."""
        step = np.linspace(-0.03, 0.03, a.grid)
        cand, offs = [], []
        for dx in step:
            for dy in step:
                for dz in step:
                    v = view.default_view(s, maps[victim])
                    Tc = np.array(last_good, np.float64).reshape(4, 4).copy()
                    Tc[:3, 3] += Tc[:3, :3] @ np.array([dx, dy, dz])
                    v.pose[:] = [float(x) for x in Tc.astype(np.float32).T.ravel()]
                    cand.append(v)
                    offs.append((dx, dy, dz))
        got = score.score_streams([maps[victim]] * len(cand), cand, [victim] * len(cand))
        order = np.argsort(-got["n_inlier"], kind="stable")[:5]
        rel = np.linalg.inv(gts[a.kidnap_frame - 1]) @ gts[k]
        print("  relocalisation of stream %d: %d candidate poses around its last good pose in one call; true offset in that frame %s m"
              % (victim, len(cand), np.round(rel[:3, 3], 4).tolist()))
        for o in order:
            print("    offset %s: n_inlier %d of n_both %d" % (np.round(offs[o], 4).tolist(), got["n_inlier"][o], got["n_both"][o]))
        err = pose_delta(np.asarray(Tq[victim], np.float64), gts[k])
        print("    the pose the solver carried on with: n_inlier %d of n_both %d; its error vs ground truth %.2e rad %.2e m"
              % (rec["n_inlier"][victim], rec["n_both"][victim], err[0], err[1]))

    print("%5s %6s %8s %8s %8s %7s %7s %8s %8s %9s | %8s %8s" % ("frame", "stream", "n_frame", "n_masked", "n_both", "n_front", "n_behind", "inliers", "overlap",
                                                          "mean|r| m", "n_both'", "inliers'"))
    load(0)
    s.current_to_prediction()
    s.push_history(0)
    s.set_kb(1.05)
    load(1)
    s.process_frame(1)
    Tq = s.batch_results()[0]
    s.filter_depth()
    rec = before_fuse(Tq)  # (the maps are still empty)
    sf.SurfelMap.fuse_frames(s, streams, maps, list(Tq), 1.0, mp)
    health(1, rec)
    last_good = None
    for k in range(2, a.frames):
        s.set_kb(1.05 if k == 2 else 1.5)
        if k == a.kidnap_frame:
            last_good = maps[victim].info()["pose"].copy()
        sf.SurfelMap.predict_frames(s, streams, maps, mp)
        load(k)
        s.filter_depth()
        s.process_frame(k)
        Tq = s.batch_results()[0]
        rec = before_fuse(Tq)
        if k == a.kidnap_frame + 1 and last_good is not None:
            relocalise(k, last_good, rec, Tq)  # before the fuse: the map does not hold this frame yet
        sf.SurfelMap.fuse_frames(s, streams, maps, list(Tq), 1.0, mp)
        health(k, rec)


if __name__ == "__main__":
    main()
