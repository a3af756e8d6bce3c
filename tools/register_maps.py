"""Two maps of one room registered against each other (include/sf_register.h): the scene of tools/join_maps.py -- four walks
through four rooms, a keyframe database, one stream handed an earlier frame with its pose withheld, which it fuses into a fresh
second map whose world frame is its own camera; a query, a score and one sfa_refine_streams call against that single frame give
the refined pose, the transform tools/join_maps.py merges with. Here that pose is then PERTURBED by a small motion, and ONE
sfg_register_maps call registers the second map against the first from the perturbed start: map against map, no frame. For each of
the three transforms -- refined, perturbed, registered -- the tool prints n_shared and n_out of a dry-run merge, and how far the
transform is from the true pose of the frame.

The figures are what they are on this synthetic walk; no threshold is drawn from them.

usage: python tools/register_maps.py [--join-cell 0.02] [--register-cell 0.1] [--register-dist-max 0.05] [--iterations 10] [--perturb 1.0]
                                     [the options of tools/relocalise.py] [--json FILE]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

import staticfusion_amd as sf
from relocalise import arguments, lost_in_the_rooms
from staticfusion_amd import align, join, register, score
from staticfusion_amd.synth import pose_delta


def small_motion(scale):
    """a rotation of about 0.02 rad and a translation of about 0.03 m, times scale, as a 4 x 4 matrix"""
    w = scale * np.array([0.012, -0.014, 0.008])
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    a = 0.5 * K
    M = np.eye(4)
    M[:3, :3] = np.linalg.solve(np.eye(3) - a, np.eye(3) + a)  # the Cayley map of w
    M[:3, 3] = scale * np.array([0.02, -0.015, 0.017])
    return M


def main():
    ap = arguments(__doc__)
    ap.add_argument("--join-cell", type=float, default=0.02)
    ap.add_argument("--register-cell", type=float, default=0.1)
    ap.add_argument("--register-dist-max", type=float, default=0.05)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--perturb", type=float, default=1.0)
    a = ap.parse_args()
    s, maps, info, stored, lost, k0, gts, cand, vs = lost_in_the_rooms(a)
    first = maps[lost]
    n = len(vs)
    second = sf.SurfelMap(s, 4 * s.rows * s.cols)
    second.fuse_frame(lost, None)
    sp = score.Params(use_b=False)  # (the b image belongs to another frame)
    rec = score.score_streams([first] * n, vs, [lost] * n, sp)
    winner = int(np.argmax(rec["n_inlier"]))
    res = align.refine_streams([first], [vs[winner]], [lost], align.Params(iterations=a.iterations, use_b=False))
    refined = align.pose_matrix(res[0])
    perturbed = (small_motion(a.perturb) @ refined.astype(np.float64)).astype(np.float32)
    reg = register.Registrar(s)
    out = reg.register_maps([first], [second], [perturbed], register.Params(cell=a.register_cell, dist_max=a.register_dist_max, iterations=a.iterations))
    registered = register.transform_matrix(out[0])
    dry = join.Params(cell=a.join_cell, dry_run=True)
    rows = {}
    print("stream %d is handed its frame %d again and fuses it into a second map of %d surfels; the first map has %d."
          % (lost, k0, second.info()["count"], first.info()["count"]))
    print("  sfg_register_maps from the perturbed pose, cell %.3f m, dist_max %.3f m: status %d after %d steps, pairs %d -> %d of %d sampled, rms residual %.2e -> %.2e m"
          % (a.register_cell, a.register_dist_max, int(out["status"][0]), int(out["iterations_done"][0]), int(out["n_first"][0]), int(out["n_last"][0]), int(out["n_sampled"][0]),
             np.sqrt(out["ss_first"][0] / max(int(out["n_first"][0]), 1)) / 65536, np.sqrt(out["ss_last"][0] / max(int(out["n_last"][0]), 1)) / 65536))
    for name, T in (("refined against one frame", refined), ("perturbed", perturbed), ("registered map against map", registered)):
        c = join.merge([first], [second], [T], dry)[0]
        err = pose_delta(T.astype(np.float64), gts[k0])
        rows[name] = dict(n_shared=c["n_shared"], n_out=c["n_out"], n_in=c["n_in"], rot_err_rad=err[0], trans_err_m=err[1])
        print("  %-28s dry-run merge at %.3f m: n_shared %6d, n_out %6d of %d; %.2e rad %.2e m from the true pose" % (name, a.join_cell, c["n_shared"], c["n_out"], c["n_in"], err[0], err[1]))
    res_json = dict(frames=a.frames, lost_stream=lost, earlier_frame=k0, join_cell=a.join_cell, register_cell=a.register_cell, register_dist_max=a.register_dist_max, perturb=a.perturb,
                    status=int(out["status"][0]), iterations_done=int(out["iterations_done"][0]), n_first=int(out["n_first"][0]), n_last=int(out["n_last"][0]),
                    n_sampled=int(out["n_sampled"][0]), n_outside=int(out["n_outside"][0]), transforms=rows)
    print(json.dumps(res_json))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res_json, f, indent=1)
            f.write("\n")
    reg.close()


if __name__ == "__main__":
    main()
