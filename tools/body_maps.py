"""A map of the moving thing (include/sf_body_maps.h): the moving-sphere sequences of tools/moving_regions.py go through predict
-> load -> solve -> fuse, and after every solve the moving regions of every stream are labelled (sfr_label_streams), followed
(sft_update_streams) and aligned with the frame before (sfb_estimate_images, paired by the tracks), as tools/body_motion.py does,
all with the ground-truth camera poses the generator gives. The largest followed region of every stream is then fused into two
body maps of its own (sfp_fuse_images): one carried along with the W of its motion record where the status is SFB_OK (the
identity otherwise, marked `-`), and one carried along with the generator's true motion of the sphere. A map starts again when
its track was not the largest followed region of the frame before.

Per stream and frame the tool prints, for both maps, the count, how many surfels have been seen at least three times
(s[5] >= 3) and the rms distance of those to the true sphere. One orbit of the first stream's estimated-motion map is written
with the calls of tools/render_map.py. The figures are what they are on these synthetic walks; nothing is tuned on them.

usage: python tools/body_maps.py [--sequences 4] [--frames 10] [--min-pixels 16] [--damping 1e-4] [--views 8] [--out DIR] [--json FILE]
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
from render_map import write_pgm16, write_ppm
from staticfusion_amd import bodies, body_maps, regions, tracks, view
from staticfusion_amd.synth import FOVH, Scene, make_sequence, sequence_trajectory


def sphere_stats(surf, centre, radius):
    """(count, seen at least three times, rms distance in mm of those to the sphere)"""
    seen = surf[:, 5] >= 3
    if not seen.any():
        return surf.shape[0], 0, float("nan")
    d = np.linalg.norm(surf[seen, 0:3].astype(np.float64) - centre, axis=1) - radius
    return surf.shape[0], int(seen.sum()), 1000.0 * float(np.sqrt(np.mean(d * d)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=4)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--min-pixels", type=int, default=16)
    ap.add_argument("--damping", type=float, default=1e-4)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--out", default=None)
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
    scene = Scene(sphere=True)
    centre0, radius = scene.sphere_c0.astype(np.float64), float(scene.sphere_r)
    f = cols / (2.0 * np.tan(0.5 * FOVH))  # the generator's camera at the solver's resolution
    cx, cy = (cols - 1) / 2.0, (rows - 1) / 2.0
    tracker = tracks.Tracker(s, n, M)
    rp, tp, bp, pp = regions.Params(min_pixels=a.min_pixels), tracks.Params(), bodies.Params(damping=a.damping), body_maps.Params()
    body = [None] * n  # per stream: dict(id, frame, est, true) of the region its two maps follow
    out, before = [], None

    def report(k):
        nonlocal before
        cams = [tracks.Camera(walks[q][0][k], cx, cy, f, f) for q in range(n)]
        depth = [s.current(q)[0] for q in range(n)]
        labels = regions.label_streams(s, streams, rp, M, labels=True)[2]
        summ, recs = tracker.update_streams(streams, streams, cams, rp, tp)
        mot = None
        if before is not None:
            z0, l0, c0, r0 = before
            pairs = np.array([bodies.pairs_from_tracks(recs[q], M) for q in range(n)])
            mot = bodies.estimate_images(s, z0, l0, depth, labels, c0, cams, [len(r0[q]) for q in range(n)], pairs, bp, M)
        for q in range(n):
            live = [r for r in recs[q] if int(r["id"]) > 0]
            if not live:
                print("%5d %6d | no followed region" % (k, q))
                continue
            big = max(live, key=lambda r: int(r["n"]))
            t, ident, prev = int(big["region"]), int(big["id"]), int(big["prev_region"])
            centre = centre0 + np.asarray(walks[q][1][k], np.float64)
            b = body[q]
            if b is None or b["id"] != ident or b["frame"] != k - 1 or prev <= 0 or mot is None:
                if b is not None:
                    b["est"].close()
                    b["true"].close()
                b = body[q] = dict(id=ident, est=sf.SurfelMap(s, rows * cols), true=sf.SurfelMap(s, rows * cols))
                W_est, W_true, mark = np.eye(4), np.eye(4), "new"
            else:
                m = mot[q, prev - 1]
                ok = int(m["status"]) == bodies.OK
                W_est = bodies.matrix(m["w"]) if ok else np.eye(4)
                W_true = np.eye(4)
                W_true[:3, 3] = np.asarray(walks[q][1][k], np.float64) - np.asarray(walks[q][1][k - 1], np.float64)
                mark = "W" if ok else "-"
            b["frame"] = k
            ce, ct = body_maps.fuse([b["est"], b["true"]], [depth[q]] * 2, [labels[q]] * 2, [cams[q]] * 2, [t, t], [W_est, W_true], None, pp)
            se, st = sphere_stats(b["est"].download(), centre, radius), sphere_stats(b["true"].download(), centre, radius)
            rec = dict(frame=k, stream=q, id=ident, motion=mark, counts_estimated=ce, counts_true=ct, estimated=dict(count=se[0], seen3=se[1], rms_mm=round(se[2], 3)),
                       true=dict(count=st[0], seen3=st[1], rms_mm=round(st[2], 3)))
            out.append(rec)
            print("%5d %6d | id %d %3s | estimated motion: %5d surfels (+%4d, merged %4d, conflict %3d), %5d seen >= 3 at rms %7.3f mm | true motion: %5d surfels (+%4d, merged %4d), %5d seen >= 3 at rms %7.3f mm"
                  % (k, q, ident, mark, se[0], ce["n_added"], ce["n_merged"], ce["n_conflict"], se[1], se[2], st[0], ct["n_added"], ct["n_merged"], st[1], st[2]))
        before = (depth, labels, cams, recs)

    print("frame stream | the largest followed region fused into two body maps (parameters the defaults of sfp_default_params; region motion with damping %g)" % a.damping)
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
    last = [r for r in out if r["frame"] == a.frames - 1]
    if last:
        print("last frame, median over %d streams: estimated motion %d surfels, %d seen >= 3, rms %.3f mm; true motion %d surfels, %d seen >= 3, rms %.3f mm"
              % (len(last), np.median([r["estimated"]["count"] for r in last]), np.median([r["estimated"]["seen3"] for r in last]),
                 np.nanmedian([r["estimated"]["rms_mm"] for r in last]), np.median([r["true"]["count"] for r in last]), np.median([r["true"]["seen3"] for r in last]),
                 np.nanmedian([r["true"]["rms_mm"] for r in last])))
    if a.out and body[0] is not None and body[0]["est"].info()["count"] > 0:
        m = body[0]["est"]
        surf = m.download()
        centre = np.median(surf[:, :3], axis=0).astype(np.float64)
        fv = 0.9 * cols
        views = []
        for q in range(a.views):
            ang = 2 * np.pi * q / max(a.views, 1)
            eye = centre + np.array([0.6 * np.sin(ang), -0.15, -0.9 + 0.3 * (1 - np.cos(ang))])
            views.append(view.View(view.look_at(eye, centre), cols / 2, rows / 2, fv, fv, rows, cols, min_confidence=0.0))
        images = view.render([m] * a.views, views)
        os.makedirs(a.out, exist_ok=True)
        for q, im in enumerate(images):
            write_ppm(os.path.join(a.out, "body_%02d.ppm" % q), im["rgb"])
            write_pgm16(os.path.join(a.out, "body_%02d_depth.pgm" % q), im["depth"])
        drawn = [float((im["index"] >= 0).mean()) for im in images]
        print("body map of stream 0 (estimated motion): %d surfels; %d views %dx%d written to %s/ (drawn share %.3f .. %.3f)"
              % (surf.shape[0], a.views, cols, rows, a.out, min(drawn), max(drawn)))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(dict(sequences=n, frames=a.frames, min_pixels=a.min_pixels, damping=a.damping, rows=rows, cols=cols, records=out), fh, indent=1)
            fh.write("\n")
    tracker.close()
    for b in body:
        if b is not None:
            b["est"].close()
            b["true"].close()
    for m in maps:
        m.close()
    s.close()


if __name__ == "__main__":
    main()
