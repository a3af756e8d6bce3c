"""Relocalisation from keyframes (include/sf_keyframes.h + include/sf_score.h): the scenario of tools/track_health.py taken one
step further. Four sequences walk through four rooms (host frames, predict -> load -> solve -> fuse); after every frame ONE
sfk_add_streams call offers every stream's frame, under its map's tag and with the pose its map has after the fuse, to one keyframe
database, which keeps the frames that differ from what it holds by at least --min-distance ferns. Then one stream is handed a
frame from earlier in its own walk with its pose withheld: ONE sfk_query_streams call (m = 4) proposes stored poses, ONE
sfs_score_streams call scores the frame against the stream's map from each of them, and the tool reports which candidate wins
and how far its pose lies from the true one.

The figures are what they are on this synthetic walk; no threshold is drawn from them.

usage: python tools/relocalise.py [--frames 14] [--lost-stream 1] [--earlier-frame 4] [--min-distance 8] [--cell 8] [--ferns 256] [--json FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import staticfusion_amd as sf
from staticfusion_amd import keyframes, score, view
from staticfusion_amd.synth import Scene, pose_delta, se3_exp


def arguments(doc=None):
    ap = argparse.ArgumentParser(description=doc)
    ap.add_argument("--frames", type=int, default=14)
    ap.add_argument("--lost-stream", type=int, default=1)
    ap.add_argument("--earlier-frame", type=int, default=4)
    ap.add_argument("--min-distance", type=int, default=8)
    ap.add_argument("--cell", type=int, default=8)
    ap.add_argument("--ferns", type=int, default=256)
    ap.add_argument("--step-scale", type=float, default=2.0, help="the walk's step as a multiple of the one of tools/track_health.py")
    ap.add_argument("--json", default=None)
    return ap


def lost_in_the_rooms(a):
    """the walk, the keyframe database and the lost stream (also the scene of tools/refine_pose.py): solver, maps, what the
    database holds, the lost stream and the frame it was handed, the true poses, the candidates of ONE query and their views"""
    api = sf.load()
    rows, cols, res, n = 240, 320, 2, 4
    s = sf.Solver(api, rows, cols, n, api.default_params_struct())
    maps = [sf.SurfelMap(s, 4 * rows * cols) for _ in range(n)]
    mp = s.default_model_params()
    streams = list(range(n))
    db = keyframes.KeyframeDb(s, a.cell, n_ferns=a.ferns, capacity=n * a.frames)
    scenes = [Scene(seed=77 + 5 * q, sphere=False, wall_z=3.0 - 0.3 * (q % 4), tilt_deg=10.0 + 5.0 * (q % 4), floor_y=1.0 - 0.08 * (q % 4)) for q in range(n)]
    xi = np.array([0.010, 0.004, 0.006, 0.002, -0.004, 0.003]) * 0.6 * a.step_scale
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

    def offer(k):
        poses = np.stack([m.info()["pose"] for m in maps])  # after the fuse: where each map now says its camera is
        slots, near = db.add_streams(streams, poses, streams, [k] * n, min_distance=a.min_distance, nearest=True)
        print("%5d   %s" % (k, "   ".join("%4s (nearest %3d)" % ("-" if slots[q] < 0 else str(slots[q]), near["distance"][q]) for q in range(n))))

    print("frame   new slot per stream, or - (the distance to the nearest keyframe of the stream's map before the call; -1: none)")
    for q in range(n):
        s.load_frame(q, *frames[0][q], res)
    s.current_to_prediction()
    s.push_history(0)
    s.set_kb(1.05)
    for q in range(n):
        s.load_frame(q, *frames[1][q], res)
    s.process_frame(1)
    Tq = s.batch_results()[0]
    s.filter_depth()
    sf.SurfelMap.fuse_frames(s, streams, maps, list(Tq), 1.0, mp)
    offer(1)
    for k in range(2, a.frames):
        s.set_kb(1.05 if k == 2 else 1.5)
        sf.SurfelMap.predict_frames(s, streams, maps, mp)
        for q in range(n):
            s.load_frame(q, *frames[k][q], res)
        s.filter_depth()
        s.process_frame(k)
        Tq = s.batch_results()[0]
        sf.SurfelMap.fuse_frames(s, streams, maps, list(Tq), 1.0, mp)
        offer(k)
    info = db.info()
    stored = db.get()
    print("the database holds %d keyframes of %d offered; per map: %s" % (info["count"], n * (a.frames - 1), np.bincount(stored["tags"], minlength=n).tolist()))
    # ---- the lost stream: a frame from earlier in its own walk, pose withheld
    lost, k0 = a.lost_stream % n, a.earlier_frame
    s.load_frame(lost, *frames[k0][lost], res)
    s.filter_depth()
    got = db.query_streams([lost], [lost], 4)
    cand = db.candidates(got)
    vs = []
    for pose in cand["pose"]:
        v = view.default_view(s, maps[lost])
        v.pose[:] = [float(x) for x in pose.T.ravel()]
        vs.append(v)
    return s, maps, info, stored, lost, k0, gts, cand, vs


def main():
    a = arguments().parse_args()
    s, maps, info, stored, lost, k0, gts, cand, vs = lost_in_the_rooms(a)
    rec = score.score_streams([maps[lost]] * len(vs), vs, [lost] * len(vs), score.Params(use_b=False))  # (the b image belongs to another frame)
    d = score.derived(rec)
    winner = int(np.argmax(rec["n_inlier"]))
    print("stream %d is handed its frame %d again. One query (m = 4), one score call over %d candidates:" % (lost, k0, len(vs)))
    out = []
    for c in range(len(vs)):
        err = pose_delta(cand["pose"][c].astype(np.float64), gts[k0])
        out.append(dict(slot=int(cand["slot"][c]), stamp=int(stored["stamps"][cand["slot"][c]]), distance=int(cand["distance"][c]), n_inlier=int(rec["n_inlier"][c]),
                        n_both=int(rec["n_both"][c]), inlier_ratio=float(d["inlier_ratio"][c]), rot_err_rad=err[0], trans_err_m=err[1]))
        print("  %s slot %3d (frame %2d) fern distance %3d | n_inlier %6d of n_both %6d (%.3f) | its pose vs the true one: %.2e rad %.2e m"
              % ("*" if c == winner else " ", out[-1]["slot"], out[-1]["stamp"], out[-1]["distance"], out[-1]["n_inlier"], out[-1]["n_both"], out[-1]["inlier_ratio"],
                 err[0], err[1]))
    res_json = dict(frames=a.frames, cell=a.cell, ferns=a.ferns, min_distance=a.min_distance, step_scale=a.step_scale, keyframes=info["count"], lost_stream=lost,
                    earlier_frame=k0, winner=winner, candidates=out)
    print(json.dumps(res_json))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res_json, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
