"""What moved, where, and how large it was (include/sf_regions.h): the moving-sphere sequences of
synth.make_sequence(sphere=True) go through predict -> load -> solve -> fuse, and after every solve ONE sfr_label_streams call
labels the moving pixels of every stream (b < b_max of the solver's static weight, split where depth jumps). Per frame and
stream the tool prints the regions found next to where the generator put the sphere: the sphere's pixels are those whose depth
differs from a rendering of the same frame without it.

The figures are what they are on these synthetic walks; no threshold is drawn from them.

usage: python tools/moving_regions.py [--sequences 4] [--frames 10] [--min-pixels 16] [--json FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import staticfusion_amd as sf
from staticfusion_amd import regions
from staticfusion_amd.synth import _render_sequence_frame, make_sequence, sequence_trajectory


def as_sensor_frame(depth, inten):
    """a rendered (depth in metres, intensity in 0..1) pair as the loader takes it: RGB bytes and millimetres, decoder order"""
    g = np.clip(np.rint(inten * 255), 1, 255).astype(np.uint8)
    return (np.ascontiguousarray(np.repeat(g[::-1, :, None], 3, axis=2)), np.ascontiguousarray(np.clip(np.rint(depth[::-1] * 1000), 0, 65535).astype(np.uint16)))


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
    truth = []  # per sequence and frame: (pixels, mean v, mean u, mean depth) of the sphere
    for q in range(n):
        poses, offsets = sequence_trajectory(1000 + q, a.frames)
        per = []
        for k in range(a.frames):
            behind = _render_sequence_frame((1000 + q, poses[k], offsets[k], False, 2 * cols, 2 * rows))[0]
            d = seqs[q]["frames"][k][0]
            on = d != behind
            v, u = np.nonzero(on)
            per.append((int(on.sum()), float(v.mean()) if on.any() else -1.0, float(u.mean()) if on.any() else -1.0, float(d[on].mean()) if on.any() else 0.0))
        truth.append(per)
    p = regions.Params(min_pixels=a.min_pixels)
    out = []

    def report(k):
        summ, recs = regions.label_streams(s, streams, p, 8)
        for q in range(n):
            v, u, z, w = regions.means(recs[q])
            t = truth[q][k]
            found = [dict(n=int(r["n"]), v=round(float(v[j]), 1), u=round(float(u[j]), 1), z=round(float(z[j]), 3), b=round(float(w[j]), 3),
                          box=[int(r["v_min"]), int(r["v_max"]), int(r["u_min"]), int(r["u_max"])]) for j, r in enumerate(recs[q])]
            out.append(dict(frame=k, stream=q, n_mask=int(summ["n_mask"][q]), n_components=int(summ["n_components"][q]), n_regions=int(summ["n_regions"][q]),
                            sphere=dict(n=t[0], v=round(t[1], 1), u=round(t[2], 1), z=round(t[3], 3)), regions=found))
            print("%5d %6d | sphere %5d px at (%5.1f, %5.1f) %.2f m | mask %5d, %3d components, %2d regions: %s"
                  % (k, q, t[0], t[1], t[2], t[3], summ["n_mask"][q], summ["n_components"][q], summ["n_regions"][q],
                     "; ".join("%d px at (%.1f, %.1f) %.2f m" % (f["n"], f["v"], f["u"], f["z"]) for f in found) or "-"))

    print("frame stream | where the generator put the sphere (rows down, columns right) | what sfr_label_streams found (b < %.2f, >= %d px)" % (p.b_max, p.min_pixels))
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
    res = dict(sequences=n, frames=a.frames, min_pixels=a.min_pixels, b_max=p.b_max, rows=rows, cols=cols, records=out)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    for m in maps:
        m.close()
    s.close()


if __name__ == "__main__":
    main()
