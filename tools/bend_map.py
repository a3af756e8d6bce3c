"""A loop closure applied to a map (include/sf_deform.h), on a synthetic walk: a camera looks into the corner of a room (back wall, side wall, floor),
turns away along the side wall and comes back. Every frame is put into the map under a pose that drifts a little more with every
frame, so the wall is in the map twice at the end: where the first frames saw it, and where the last frames -- 8 cm and 0.02 rad
off by then -- put it.

The tool then does what a caller of the library does:
  1 refines the drifted pose of the last frame against the OLD part of the map (align.refine_images on a map of the first
    frames' surfels: the inactive model of a loop closure);
  2 makes constraints from that: pixels of the last frame under the drifted pose go to the same pixels under the refined pose,
    with the last frame's time, and pins (dst == src) are sampled from the old part;
  3 samples nodes from the old part and from the rest (deform.sample_nodes), solves (deform.solve) with a time window, so that a
    constraint takes the nodes of its own time, and applies the graph to the whole map (deform.apply_maps);
  4 prints the agreement counts of the last frame against the map (score.score_images, seen from the refined pose) before and
    after, and how far the surfels lie from where the true poses would have put them, before and after.
The map is built in NumPy from the rendered frames (one surfel per pixel), not by the fusion: the tool is about the bend.

The figures are what they are on this synthetic walk; no threshold is drawn from them.

usage: python tools/bend_map.py [--frames 12] [--spacing 0.5] [--window 3] [--json FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from staticfusion_amd.synth import FOVH, Scene, pose_delta, se3_exp

ROWS, COLS = 120, 160
DRIFT = np.array([0.06, 0.0, 0.05, 0.0, 0.02, 0.0])  # the twist the pose error has reached at the last frame


def yaw(a):
    T = np.eye(4)
    T[0, 0], T[0, 2], T[2, 0], T[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    return T


def intrinsics():
    f = COLS / (2.0 * np.tan(0.5 * FOVH))
    return COLS / 2.0 - 1.0, ROWS / 2.0 - 1.0, f


def camera_points(depth):
    cx, cy, f = intrinsics()
    u, v = np.meshgrid(np.arange(COLS, dtype=np.float64), np.arange(ROWS, dtype=np.float64))
    return np.stack([(u - cx) * depth / f, (v - cy) * depth / f, depth], axis=-1)


def frame_surfels(depth, inten, pose, time):
    """one surfel per interior pixel with a depth: position and normal under `pose`, grey colour, confidence 1, both times `time`"""
    cx, cy, f = intrinsics()
    P = camera_points(depth)
    a, b = P[1:-1, 2:] - P[1:-1, :-2], P[2:, 1:-1] - P[:-2, 1:-1]
    n = np.cross(a, b)
    ok = (depth[1:-1, 1:-1] > 0) & (depth[1:-1, 2:] > 0) & (depth[1:-1, :-2] > 0) & (depth[2:, 1:-1] > 0) & (depth[:-2, 1:-1] > 0) & (np.linalg.norm(n, axis=-1) > 0)
    p, n, g, z = P[1:-1, 1:-1][ok], n[ok], inten[1:-1, 1:-1][ok], depth[1:-1, 1:-1][ok]
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    s = np.zeros((p.shape[0], 12), np.float32)
    s[:, 0:3] = p @ pose[:3, :3].T + pose[:3, 3]
    s[:, 3] = 1.0
    byte = np.clip(np.rint(g * 255), 0, 255).astype(np.int64)
    s[:, 4] = (byte << 16) + (byte << 8) + byte
    s[:, 5] = 1.0
    s[:, 6] = s[:, 7] = time
    s[:, 8:11] = n @ pose[:3, :3].T
    s[:, 11] = np.minimum(2.0, 1.0 / np.maximum(np.abs(n[:, 2]), 1e-3)) * (z / f) * np.sqrt(2.0)
    return s


def walk(frames):
    """per frame: the true pose, the drifted pose, depth and intensity as the true pose sees them, and its surfels under the
    drifted pose (time k + 1)"""
    scene = Scene(seed=77, sphere=False)
    out = []
    for k in range(frames):
        x = k / (frames - 1.0)
        true = yaw(-0.35 - 0.7 * np.sin(np.pi * x))  # (the first and the last frames see the back wall, the side wall and the floor)
        true[:3, 3] = [0.1 * np.sin(np.pi * x), 0.0, 0.05 * x]
        drifted = se3_exp(DRIFT * x) @ true
        depth, inten = scene.render(true, COLS, ROWS)
        out.append(dict(true=true, drifted=drifted, depth=depth.astype(np.float32), inten=inten.astype(np.float32), surfels=frame_surfels(depth, inten, drifted, k + 1.0),
                        truth=frame_surfels(depth, inten, true, k + 1.0)))
    return out


def position_error(surfels, truth):
    """mean distance of surfels from where the true poses would have put them"""
    return float(np.mean(np.linalg.norm(surfels[:, 0:3].astype(np.float64) - truth[:, 0:3], axis=1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--spacing", type=float, default=0.5)
    ap.add_argument("--window", type=float, default=3.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import staticfusion_amd as sf
    from staticfusion_amd import align, deform, score, view

    fr = walk(a.frames)
    api = sf.load()
    s = sf.Solver(api, ROWS, COLS, 1, api.default_params_struct())
    n_old = 2
    old_s = np.concatenate([f["surfels"] for f in fr[:n_old]])
    rest_s = np.concatenate([f["surfels"] for f in fr[n_old:]])
    all_s = np.concatenate([old_s, rest_s])
    truth = np.concatenate([f["truth"] for f in fr])
    eye = np.eye(4, dtype=np.float32)
    maps = {}
    for name, arr in (("old", old_s), ("rest", rest_s), ("all", all_s)):
        maps[name] = sf.SurfelMap(s, arr.shape[0])
        maps[name].upload(arr, eye, a.frames + 1)
    last = fr[-1]
    cx, cy, f = intrinsics()
    to_view = lambda pose: view.View(pose, cx, cy, f, f, ROWS, COLS, min_confidence=0.0)  # noqa: E731
    # 1 the drifted pose refined against the old part
    res = align.refine_images([maps["old"]], [to_view(last["drifted"])], [last["depth"]], None, align.Params(iterations=15, use_b=False))
    refined = align.pose_matrix(res[0]).astype(np.float64)
    e0, e1 = pose_delta(last["drifted"], last["true"]), pose_delta(refined, last["true"])
    print("last frame: drifted pose off by %.3f rad %.3f m; refined against the old part (status %d, %d steps): %.4f rad %.4f m"
          % (e0[0], e0[1], int(res["status"][0]), int(res["iterations_done"][0]), e1[0], e1[1]))
    # 2 constraints: the last frame's pixels from the drifted pose to the refined one; pins from the old part
    P = camera_points(last["depth"].astype(np.float64))[::6, ::6].reshape(-1, 3)
    P = P[P[:, 2] > 0]
    src = P @ last["drifted"][:3, :3].T + last["drifted"][:3, 3]
    dst = P @ refined[:3, :3].T + refined[:3, 3]
    pins = old_s[::40]
    c_src = np.concatenate([src, pins[:, 0:3]])
    c_dst = np.concatenate([dst, pins[:, 0:3]])
    c_time = np.concatenate([np.full(src.shape[0], float(a.frames)), pins[:, 6]])
    # 3 nodes from the old part and from the rest; solve; apply
    parts = [deform.sample_nodes(maps[k], a.spacing, deform.SOLVE_MAX_NODES // 2) for k in ("old", "rest")]
    pos, times = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    M, rep = deform.solve(pos, times, c_src, c_dst, c_time, 1.0, params=deform.SolveParams(time_window=a.window, w_reg=10.0, iterations=8))
    print("%d nodes (%d old, %d recent), %d constraints (%d pins), %d bound; status %d after %d iterations; energy %.4e -> %.4e"
          % (pos.shape[0], parts[0][0].shape[0], parts[1][0].shape[0], c_src.shape[0], pins.shape[0], rep["n_bound"], rep["status"], rep["iterations_done"],
             rep["energy"][0], rep["energy"][-1]))
    sp = score.Params(use_b=False)
    before = score.score_images([maps["all"]], [to_view(refined)], [last["depth"]], [last["inten"]], None, sp)
    recent = all_s[:, 6] >= a.frames - 1  # the surfels of the last two frames: the second sighting of the wall
    wall_before = position_error(all_s[recent], truth[recent])
    g = deform.Graph(s)
    g.set(pos, times, M)
    counts = deform.apply_maps([maps["all"]], g, deform.Params(time_window=a.window))[0]
    bent = maps["all"].download()
    after = score.score_images([maps["all"]], [to_view(refined)], [last["depth"]], [last["inten"]], None, sp)
    wall_after = position_error(bent[recent], truth[recent])
    all_before, all_after = position_error(all_s, truth), position_error(bent, truth)
    old_moved = float(np.abs(bent[:old_s.shape[0], 0:3] - old_s[:, 0:3]).max())
    fields = [k for k in before.dtype.names if k.startswith("n_")]
    print("apply: %r" % (counts,))
    print("score of the last frame against the map from the refined pose, before -> after:")
    for k in fields:
        print("  %-12s %8d -> %8d" % (k, int(before[k][0]), int(after[k][0])))
    print("mean distance of a surfel from where the true poses put it: last two frames %.4f m -> %.4f m, whole map %.4f m -> %.4f m; the old part moved by at most "
          "%.2e m" % (wall_before, wall_after, all_before, all_after, old_moved))
    out = dict(frames=a.frames, spacing=a.spacing, window=a.window, nodes=int(pos.shape[0]), constraints=int(c_src.shape[0]), pins=int(pins.shape[0]),
               solve=dict(status=rep["status"], iterations_done=rep["iterations_done"], n_bound=rep["n_bound"], energy=[float(x) for x in rep["energy"]]),
               pose_error_drifted=list(e0), pose_error_refined=list(e1), apply=counts, score_before={k: int(before[k][0]) for k in fields},
               score_after={k: int(after[k][0]) for k in fields}, recent_error_before_m=wall_before, recent_error_after_m=wall_after, map_error_before_m=all_before, map_error_after_m=all_after, old_part_moved_m=old_moved)
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    g.close()
    for m in maps.values():
        m.close()
    s.close()


if __name__ == "__main__":
    main()
