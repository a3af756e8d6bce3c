"""A loop closed with constraints the library builds (include/sf_closure.h): the walk of tools/bend_map.py -- a camera looks into
the corner of a room, turns away along the side wall and comes back, every frame put into the map under a pose that drifts a
little more, so the wall is in the map twice at the end -- with step 2 of that tool, its NumPy constraints, replaced by
closure.Builder.build.

  1 the whole walk is ONE map; its old part (what the last frames - 2 ticks did not see) is taken out with map_window.extract
    (a filter with max_age and invert) and appended into a second map, the inactive model of a loop closure;
  2 the drifted pose of the last frame is refined against the old part (align.refine_images);
  3 closure.Builder.build draws the active part of the map (max_age 1: the last frame) from the drifted pose and the old part
    from the refined pose and returns the constraints: a link wherever both are drawn at the same depth, a pin wherever the old
    part is drawn;
  4 nodes are sampled from the old part and from the rest (deform.sample_nodes), deform.solve finds the transforms with a time
    window, deform.apply_maps bends the whole map;
  5 the figures of tools/bend_map.py are printed: the agreement counts of the last frame against the map from the refined pose
    before and after, and how far the surfels lie from where the true poses would have put them.

The figures are what they are on this synthetic walk; no threshold is drawn from them.

usage: python tools/close_loop.py [--frames 12] [--spacing 0.5] [--window 3] [--stride 6] [--json FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

from bend_map import COLS, ROWS, intrinsics, position_error, walk  # the walk itself: one statement of it
from staticfusion_amd.synth import pose_delta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--spacing", type=float, default=0.5)
    ap.add_argument("--window", type=float, default=3.0)
    ap.add_argument("--stride", type=int, default=6)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import staticfusion_amd as sf
    from staticfusion_amd import align, closure, deform, map_window, score, view

    fr = walk(a.frames)
    api = sf.load()
    s = sf.Solver(api, ROWS, COLS, 1, api.default_params_struct())
    all_s = np.concatenate([f["surfels"] for f in fr])
    truth = np.concatenate([f["truth"] for f in fr])
    tick = a.frames + 1
    eye = np.eye(4, dtype=np.float32)
    m_all = sf.SurfelMap(s, all_s.shape[0])
    m_all.upload(all_s, eye, tick)
    # 1 the old part: what the last frames - 2 ticks did not see (the first two frames), as a map of its own; and the rest
    recent = map_window.Filter(max_age=a.frames - 2)
    old_s = map_window.extract(m_all, map_window.Filter(max_age=a.frames - 2, invert=True))
    rest_s = map_window.extract(m_all, recent)
    parts = {}
    for name, arr in (("old", old_s), ("rest", rest_s)):
        parts[name] = sf.SurfelMap(s, max(arr.shape[0], ROWS * COLS))
        parts[name].upload(arr[:0], eye, tick)
        map_window.append(parts[name], arr)
    last = fr[-1]
    cx, cy, f = intrinsics()
    to_view = lambda pose, **kw: view.View(pose, cx, cy, f, f, ROWS, COLS, min_confidence=0.0, **kw)  # noqa: E731
    # 2 the drifted pose refined against the old part
    res = align.refine_images([parts["old"]], [to_view(last["drifted"])], [last["depth"]], None, align.Params(iterations=15, use_b=False))
    refined = align.pose_matrix(res[0]).astype(np.float64)
    e0, e1 = pose_delta(last["drifted"], last["true"]), pose_delta(refined, last["true"])
    print("last frame: drifted pose off by %.3f rad %.3f m; refined against the old part (status %d, %d steps): %.4f rad %.4f m"
          % (e0[0], e0[1], int(res["status"][0]), int(res["iterations_done"][0]), e1[0], e1[1]))
    # 3 the constraints, built on the device
    bld = closure.Builder(s)
    cp = closure.Params(stride=a.stride, pins=2, min_time_gap=2.0 * a.window)
    recs, (cc,) = bld.build([m_all], [parts["old"]], [to_view(last["drifted"], max_age=1)], [to_view(refined)], cp)
    print("closure: %r" % (cc,))
    c_src, c_dst, c_time, c_w = closure.as_solve_arrays(recs)
    # 4 nodes from the old part and from the rest; solve; apply
    nodes = [deform.sample_nodes(parts[k], a.spacing, deform.SOLVE_MAX_NODES // 2) for k in ("old", "rest")]
    pos, times = np.concatenate([p[0] for p in nodes]), np.concatenate([p[1] for p in nodes])
    M, rep = deform.solve(pos, times, c_src, c_dst, c_time, c_w, params=deform.SolveParams(time_window=a.window, w_reg=10.0, iterations=8))
    print("%d nodes (%d old, %d recent), %d constraints (%d links, %d pins), %d bound; status %d after %d iterations; energy %.4e -> %.4e"
          % (pos.shape[0], nodes[0][0].shape[0], nodes[1][0].shape[0], recs.shape[0], cc["n_links"], cc["n_pins"], rep["n_bound"], rep["status"],
             rep["iterations_done"], rep["energy"][0], rep["energy"][-1]))
    sp = score.Params(use_b=False)
    before = score.score_images([m_all], [to_view(refined)], [last["depth"]], [last["inten"]], None, sp)
    late = all_s[:, 6] >= a.frames - 1  # the surfels of the last two frames: the second sighting of the wall
    wall_before = position_error(all_s[late], truth[late])
    g = deform.Graph(s)
    g.set(pos, times, M)
    counts = deform.apply_maps([m_all], g, deform.Params(time_window=a.window))[0]
    bent = m_all.download()
    after = score.score_images([m_all], [to_view(refined)], [last["depth"]], [last["inten"]], None, sp)
    wall_after = position_error(bent[late], truth[late])
    all_before, all_after = position_error(all_s, truth), position_error(bent, truth)
    is_old = all_s[:, 6] <= 2
    old_moved = float(np.abs(bent[is_old, 0:3] - all_s[is_old, 0:3]).max())
    fields = [k for k in before.dtype.names if k.startswith("n_")]
    print("apply: %r" % (counts,))
    print("score of the last frame against the map from the refined pose, before -> after:")
    for k in fields:
        print("  %-12s %8d -> %8d" % (k, int(before[k][0]), int(after[k][0])))
    print("mean distance of a surfel from where the true poses put it: last two frames %.4f m -> %.4f m, whole map %.4f m -> %.4f m; the old part moved by at most "
          "%.2e m" % (wall_before, wall_after, all_before, all_after, old_moved))
    out = dict(frames=a.frames, spacing=a.spacing, window=a.window, stride=a.stride, nodes=int(pos.shape[0]), constraints=int(recs.shape[0]), closure=cc,
               solve=dict(status=rep["status"], iterations_done=rep["iterations_done"], n_bound=rep["n_bound"], energy=[float(x) for x in rep["energy"]]),
               pose_error_drifted=list(e0), pose_error_refined=list(e1), apply=counts, score_before={k: int(before[k][0]) for k in fields},
               score_after={k: int(after[k][0]) for k in fields}, recent_error_before_m=wall_before, recent_error_after_m=wall_after, map_error_before_m=all_before,
               map_error_after_m=all_after, old_part_moved_m=old_moved)
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    g.close()
    bld.close()
    for m in [m_all] + list(parts.values()):
        m.close()
    s.close()


if __name__ == "__main__":
    main()
