"""Relocalisation, the last link (include/sf_align.h): the scene of tools/relocalise.py -- four walks through four rooms, a
keyframe database, one stream handed an earlier frame with its pose withheld, ONE query that proposes stored poses -- and then
ONE sfa_refine_streams call that refines every candidate against the stream's map with the frame where it lies on the device.
Per candidate the tool reports the pose error against the true pose and the sfs inlier count (ONE sfs_score_streams call each)
before and after the refinement.

The figures are what they are on this synthetic walk; no threshold is drawn from them.

usage: python tools/refine_pose.py [--iterations 10] [--dist-max 0.15] [--stride 1] [the options of tools/relocalise.py] [--json FILE]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

from relocalise import arguments, lost_in_the_rooms
from staticfusion_amd import align, score, view
from staticfusion_amd.synth import pose_delta


def main():
    ap = arguments(__doc__)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--dist-max", type=float, default=0.15)
    ap.add_argument("--stride", type=int, default=1)
    a = ap.parse_args()
    s, maps, info, stored, lost, k0, gts, cand, vs = lost_in_the_rooms(a)
    n = len(vs)
    sp = score.Params(use_b=False)  # (the b image belongs to another frame)
    p = align.Params(iterations=a.iterations, dist_max=a.dist_max, stride=a.stride, use_b=False)
    before = score.score_streams([maps[lost]] * n, vs, [lost] * n, sp)
    res = align.refine_streams([maps[lost]] * n, vs, [lost] * n, p)
    refined = []
    for q in range(n):
        v = view.default_view(s, maps[lost])
        v.pose[:] = [float(x) for x in res["pose"][q]]
        refined.append(v)
    after = score.score_streams([maps[lost]] * n, refined, [lost] * n, sp)
    print("stream %d is handed its frame %d again. One query, one refine call over %d candidates (%d iterations, dist_max %.2f, stride %d):"
          % (lost, k0, n, a.iterations, a.dist_max, a.stride))
    out = []
    for q in range(n):
        e0 = pose_delta(cand["pose"][q].astype(np.float64), gts[k0])
        e1 = pose_delta(align.pose_matrix(res[q]).astype(np.float64), gts[k0])
        rms = [float(np.sqrt(res[k][q] / max(int(res[m][q]), 1)) / 65536.0) for k, m in (("ss_first", "n_first"), ("ss_last", "n_last"))]
        out.append(dict(slot=int(cand["slot"][q]), status=int(res["status"][q]), iterations_done=int(res["iterations_done"][q]), rot_err_before_rad=e0[0],
                        trans_err_before_m=e0[1], rot_err_after_rad=e1[0], trans_err_after_m=e1[1], n_inlier_before=int(before["n_inlier"][q]),
                        n_inlier_after=int(after["n_inlier"][q]), n_both_after=int(after["n_both"][q]), pairs_first=int(res["n_first"][q]),
                        pairs_last=int(res["n_last"][q]), rms_first_m=rms[0], rms_last_m=rms[1]))
        print("  slot %3d status %d after %2d steps | pose vs the true one: %.2e rad %.2e m -> %.2e rad %.2e m | n_inlier %6d -> %6d | pairs %6d -> %6d, "
              "point-to-plane rms %.4f -> %.4f m" % (out[-1]["slot"], out[-1]["status"], out[-1]["iterations_done"], e0[0], e0[1], e1[0], e1[1],
                                                       out[-1]["n_inlier_before"], out[-1]["n_inlier_after"], out[-1]["pairs_first"], out[-1]["pairs_last"], rms[0], rms[1]))
    res_json = dict(frames=a.frames, lost_stream=lost, earlier_frame=k0, keyframes=info["count"], iterations=a.iterations, dist_max=a.dist_max, stride=a.stride,
                    candidates=out)
    print(json.dumps(res_json))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res_json, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
