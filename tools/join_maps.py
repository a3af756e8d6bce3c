"""Two maps of one room put together (include/sf_join.h): the scene of tools/relocalise.py -- four walks through four rooms, a
keyframe database, one stream handed an earlier frame with its pose withheld. The lost stream does what a lost stream does: it
fuses the frame into a fresh second map, whose world frame is its own camera. Then it is relocalised against its first map: ONE
query proposes stored poses, ONE sfs_score_streams call ranks them, ONE sfa_refine_streams call refines the winner. With the
refined pose as the transform, ONE sfj_merge_maps call joins the second map into the first. The tool prints the counts beside what
a blind append would have stored, and the agreement of the frame with the first map alone and with the joined map.

The figures are what they are on this synthetic walk; no threshold is drawn from them.

usage: python tools/join_maps.py [--join-cell 0.02] [--iterations 10] [the options of tools/relocalise.py] [--json FILE]
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
from staticfusion_amd import align, join, score, view
from staticfusion_amd.synth import pose_delta


def main():
    ap = arguments(__doc__)
    ap.add_argument("--join-cell", type=float, default=0.02)
    ap.add_argument("--iterations", type=int, default=10)
    a = ap.parse_args()
    s, maps, info, stored, lost, k0, gts, cand, vs = lost_in_the_rooms(a)
    first = maps[lost]
    n = len(vs)
    # the lost stream maps on: its frame into a fresh map, camera at the identity
    second = sf.SurfelMap(s, 4 * s.rows * s.cols)
    second.fuse_frame(lost, None)
    # relocalise: rank the candidates, refine the winner
    sp = score.Params(use_b=False)  # (the b image belongs to another frame)
    rec = score.score_streams([first] * n, vs, [lost] * n, sp)
    winner = int(np.argmax(rec["n_inlier"]))
    res = align.refine_streams([first], [vs[winner]], [lost], align.Params(iterations=a.iterations, use_b=False))
    pose = align.pose_matrix(res[0])
    err = pose_delta(pose.astype(np.float64), gts[k0])
    at = view.default_view(s, first)
    at.pose[:] = [float(x) for x in res["pose"][0]]
    alone = score.score_streams([first], [at], [lost], sp)
    # join: the second map's world frame is the camera of the frame, so the refined pose is the transform
    p = join.Params(cell=a.join_cell, stamp=first.info()["tick"])
    before = first.info()["count"]
    dry = join.merge([first], [second], [pose], join.Params(cell=a.join_cell, stamp=p.stamp, dry_run=True))[0]
    c = join.merge([first], [second], [pose], p)[0]
    joined = score.score_streams([first], [at], [lost], sp)
    thinned = join.thin_extract(first, join.Params(cell=a.join_cell))[1]
    print("stream %d is handed its frame %d again and fuses it into a second map of %d surfels." % (lost, k0, c["n_in"]))
    print("  relocalised: candidate %d of %d wins (n_inlier %d), refined in %d steps to %.2e rad %.2e m from the true pose"
          % (winner, n, int(rec["n_inlier"][winner]), int(res["iterations_done"][0]), err[0], err[1]))
    print("  sfj_merge_maps, cell %.3f m: first map %d surfels in %d voxels; of the second map's %d, %d share a voxel with the first and stay out, %d lie "
          "outside the grid, %d are added -> %d surfels (a blind append: %d)" % (a.join_cell, before, c["n_voxels"], c["n_in"], c["n_shared"], c["n_outside"], c["n_out"],
                                                                                first.info()["count"], before + c["n_in"]))
    print("  the frame against the first map alone: n_inlier %d of n_both %d; against the joined map: n_inlier %d of n_both %d"
          % (int(alone["n_inlier"][0]), int(alone["n_both"][0]), int(joined["n_inlier"][0]), int(joined["n_both"][0])))
    print("  a thin of the joined map at the same cell would keep %d of %d surfels" % (thinned["n_out"], thinned["n_in"]))
    res_json = dict(frames=a.frames, lost_stream=lost, earlier_frame=k0, join_cell=a.join_cell, winner=winner, rot_err_rad=err[0], trans_err_m=err[1],
                    first_map=before, dry_run_equals_merge=bool(dry == c), counts=c, joined_map=first.info()["count"], blind_append=before + c["n_in"],
                    n_inlier_alone=int(alone["n_inlier"][0]), n_both_alone=int(alone["n_both"][0]), n_inlier_joined=int(joined["n_inlier"][0]),
                    n_both_joined=int(joined["n_both"][0]), thin_of_joined=thinned)
    print(json.dumps(res_json))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res_json, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
