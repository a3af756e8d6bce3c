"""Pose scoring (include/sf_score.h) on one MI355X: what a score call costs beside the route a caller had without it.

The maps are what tools/full_pipeline_bench.py leaves (tools/view_bench.py build_maps): N sequences through predict -> input ->
solve -> fuse for 10 QVGA frames of a synthetic walk. Every figure is the median of 5 calls, each bracketed by a synchronisation
of the handle's stream, in one process with sf_microbench_copy (the streaming ceiling of the box at that moment).

  (a) N maps, one 320 x 240 view each from the map's own pose, every stream's current frame against its own map
      (sfs_score_streams)
  (b) one map and one frame at 512 candidate poses around the map's pose (the same map and stream 512 times)
Beside each, in the same process, the route without the feature: sfv_render_maps_device of depth + rgb into torch tensors,
then a torch reduction to the same ten numbers, read back. The tool asserts that the numbers are equal.

usage: python tools/score_bench.py [--streams 256] [--frames 10] [--candidates 512] [--json FILE]
"""
import argparse
import json
import os
import sys
import time

import torch  # first, as bench.py does: the process then holds the HIP runtime torch brought

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

import staticfusion_amd as sf
from staticfusion_amd import score, view
from staticfusion_amd.synth import se3_exp
from view_bench import build_maps, median_ms


def torch_scores(depth, rgb, zf, gf, b, p):
    """the ten numbers of include/sf_score.h from rendered images: depth (n, rows, cols) float32, rgb (n, rows, cols, 3) uint8,
    frames zf / gf / b (n or 1, rows, cols); one elementwise kernel per operation, so no contraction. `drawn` is depth > 0:
    the depth image holds 0 where nothing was drawn and a drawn surfel lies beyond 0.4 m."""
    drawn = depth > 0
    f = rgb.to(torch.float32) * (1.0 / 255.0)
    gm = (0.299 * f[..., 0] + 0.587 * f[..., 1]) + 0.114 * f[..., 2]
    fv = zf > 0
    w = (b > p.b_min) if p.use_b else torch.ones_like(fv)
    fr, masked = fv & w, fv & ~w
    both = fr & drawn
    r = zf - depth
    tol = p.tol_abs + p.tol_rel * depth
    inlier, front, behind = both & (r.abs() <= tol), both & (r < -tol), both & (r > tol)
    q = torch.round(torch.fmin(r.abs(), torch.tensor(p.max_residual, device=r.device)) * 16384.0).to(torch.int64)
    q = torch.where(both, q, torch.zeros_like(q))
    g = torch.round(torch.fmin((gf - gm).abs(), torch.tensor(1.0, device=r.device)) * 65536.0).to(torch.int64)
    g = torch.where(inlier, g, torch.zeros_like(g)) if p.use_grey else torch.zeros_like(q)
    cols = [x.expand_as(drawn).sum((1, 2)) for x in (fr, masked, drawn, both, inlier, front, behind)] + [q.sum((1, 2)), (q * q).sum((1, 2)), g.sum((1, 2))]
    return torch.stack(cols, 1).cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--candidates", type=int, default=512)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    api = sf.load()
    s, maps, mp = build_maps(api, a.streams, a.frames)
    n = len(maps)
    rows, cols = s.rows, s.cols
    counts = [m.info()["count"] for m in maps]
    res = dict(streams=n, frames=a.frames, candidates=a.candidates, surfels_per_map=int(np.median(counts)), copy_gbs=round(s.microbench_copy(256 << 20, 10), 1))
    print("%d maps, median %d surfels; device copy %.0f GB/s" % (n, res["surfels_per_map"], res["copy_gbs"]))
    p = score.Params()
    # the frames as torch tensors (row-major, like the rendered images) for the route without the feature: set-up, untimed
    cur = [s.current(q) for q in range(n)]
    zf = torch.from_numpy(np.stack([c[0] for c in cur])).cuda()
    gf = torch.from_numpy(np.stack([c[1] for c in cur])).cuda()
    bf = torch.from_numpy(np.stack([s.b_image(q) for q in range(n)])).cuda()

    def case(tag, ms, vs, st, fz, fg, fb):
        k = len(ms)
        depth = torch.zeros((k, rows, cols), dtype=torch.float32, device="cuda")
        rgb = torch.zeros((k, rows, cols, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        dp = [depth[q].data_ptr() for q in range(k)]
        cp = [rgb[q].data_ptr() for q in range(k)]
        out = {}

        def with_feature():
            out["score"] = score.score_streams(ms, vs, st, p)

        def without():
            view.render_device(ms, vs, dp, cp, None)
            s.synchronize()  # the reduction runs on torch's stream
            out["torch"] = torch_scores(depth, rgb, fz, fg, fb, p)

        res[tag + "_score_ms"] = median_ms(s, with_feature)
        res[tag + "_render_torch_ms"] = median_ms(s, without)
        got = np.stack([out["score"][f] for f in score.FIELDS], 1)
        res[tag + "_equal"] = bool(np.array_equal(got, out["torch"]))
        assert res[tag + "_equal"], "the two routes disagree:\n%s\n%s" % (got[:3], out["torch"][:3])
        d = score.derived(out["score"])
        res[tag + "_inlier_ratio_max"] = float(d["inlier_ratio"].max())
        px = k * rows * cols
        res[tag + "_model_bytes"] = int(sum(m.info()["count"] for m in ms) * 48 + px * (8 + 8 + 16 + 12))  # keys cleared and read, rays, the frame
        print("(%s) %d entries %dx%d: sfs_score_streams %.3f ms (%.1f us per entry) | render depth + rgb, torch reduction %.3f ms = %.1f x | equal: %s"
              % (tag, k, cols, rows, res[tag + "_score_ms"], 1e3 * res[tag + "_score_ms"] / k, res[tag + "_render_torch_ms"],
                 res[tag + "_render_torch_ms"] / res[tag + "_score_ms"], res[tag + "_equal"]))
        return out["score"]

    own = [view.default_view(s, m) for m in maps]
    case("a", maps, own, list(range(n)), zf, gf, bf)
    # (b) a grid of candidate poses around the pose of map 0: translations and small rotations
    rng = np.random.default_rng(1)
    base = view.view_pose(own[0]).astype(np.float64)
    cand = [own[0]]
    for _ in range(a.candidates - 1):
        xi = np.concatenate([rng.uniform(-0.15, 0.15, 3), rng.uniform(-0.08, 0.08, 3)])
        v = view.default_view(s, maps[0])
        T = (base @ se3_exp(xi)).astype(np.float32)
        v.pose[:] = [float(x) for x in T.T.ravel()]
        cand.append(v)
    sc_b = case("b", [maps[0]] * len(cand), cand, [0] * len(cand), zf[:1], gf[:1], bf[:1])
    res["b_best_is_the_maps_pose"] = bool(int(np.argmax(sc_b["n_inlier"])) == 0)
    print("(b) the map's own pose has the most inliers of the %d candidates: %s" % (len(cand), res["b_best_is_the_maps_pose"]))
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
