"""Pose refinement (include/sf_align.h) on one MI355X: what a refine call costs beside the route a caller had without it.

The maps are what tools/full_pipeline_bench.py leaves (tools/view_bench.py build_maps): N sequences through predict -> input ->
solve -> fuse for 10 QVGA frames of a synthetic walk. Every figure is the median of 5 calls, each bracketed by a synchronisation
of the handle's stream, in one process with sf_microbench_copy (the streaming ceiling of the box at that moment).

  (a) N maps, every stream's current frame against its own map from a pose displaced from the map's own (sfa_refine_streams)
  (b) one map and one frame at 512 candidate poses around the map's pose (the same map and stream 512 times)
each at strides 1 and 4. Beside each, in the same process, the route without the feature: sfv_render_maps_device of depth + index
into torch tensors, then the same steps in torch (model points and normals gathered through the index image, the gates, fp64
sums of the normal equations, a batched solve, the Cayley update), with no host synchronisation between iterations either. The
torch route sums in floating point, so its poses agree with the call's to rounding only; the tool reports the largest difference.
Time per entry and iteration divides a call by its entries and by its iterations + 1 linearisations.

No rate is asserted anywhere; the figures are what they are on the box the tool ran on.

usage: python tools/align_bench.py [--streams 256] [--frames 10] [--candidates 512] [--iterations 10] [--json FILE]
"""
import argparse
import json
import os
import sys

import torch  # first, as bench.py does: the process then holds the HIP runtime torch brought

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

import staticfusion_amd as sf
from staticfusion_amd import align, view
from staticfusion_amd.synth import se3_exp
from view_bench import build_maps, median_ms


def torch_refine(depth, index, normals, t_inv, zf, v, p):
    """the LOOP of include/sf_align.h from rendered images. depth, index (k, rows, cols); normals (k or 1, N, 3) world normals
    of the surfels; t_inv (k, 3, 3) rotation of the inverse view pose; zf (k or 1, rows, cols). Returns D (k, 3, 4) float64."""
    k, rows, cols = depth.shape
    dev = depth.device
    jj, ii = torch.meshgrid(torch.arange(rows, device=dev, dtype=torch.float32), torch.arange(cols, device=dev, dtype=torch.float32), indexing="ij")
    ray = torch.stack([(ii + 0.5 - v.cx) / v.fx, (jj + 0.5 - v.cy) / v.fy, torch.ones_like(ii)], -1)
    ray = (ray / ray.norm(dim=-1, keepdim=True)).view(1, -1, 3)
    idx = index.view(k, -1)
    drawn = idx >= 0
    nw = torch.gather(normals.expand(k, -1, -1), 1, idx.clamp(min=0).long()[..., None].expand(-1, -1, 3))
    nc = torch.einsum("kij,kpj->kpi", t_inv, nw)
    nc = nc / nc.norm(dim=-1, keepdim=True)
    M = ray * (depth.view(k, -1, 1) / ray[..., 2:3])
    st = p.stride
    z = zf[:, ::st, ::st].reshape(zf.shape[0], -1)
    x, y = ii[::st, ::st].reshape(1, -1), jj[::st, ::st].reshape(1, -1)
    P = torch.stack([((x - v.cx) * z) / v.fx, ((y - v.cy) * z) / v.fy, z], -1).expand(k, -1, -1)
    valid = ((z > 0) & (z <= p.z_max)).expand(k, -1)
    D = torch.eye(3, 4, dtype=torch.float64, device=dev).repeat(k, 1, 1)
    eye6 = torch.eye(6, dtype=torch.float64, device=dev)
    for _ in range(p.iterations):
        Df = D.float()
        Q = torch.einsum("kij,kpj->kpi", Df[:, :, :3], P) + Df[:, None, :, 3]
        px, py = (v.fx * Q[..., 0]) / Q[..., 2] + v.cx, (v.fy * Q[..., 1]) / Q[..., 2] + v.cy
        ok = valid & (Q[..., 2] >= 0.4) & (px >= 0) & (px < cols) & (py >= 0) & (py < rows)
        flat = py.floor().clamp(0, rows - 1).long() * cols + px.floor().clamp(0, cols - 1).long()
        Mg = torch.gather(M, 1, flat[..., None].expand(-1, -1, 3))
        ng = torch.gather(nc, 1, flat[..., None].expand(-1, -1, 3))
        d = Q - Mg
        r = (ng * d).sum(-1)
        ok = ok & torch.gather(drawn, 1, flat) & ((d * d).sum(-1) <= p.dist_max * p.dist_max) & ((ng * ng).sum(-1) > 0.5) & (r.abs() <= p.dist_max)
        J = torch.cat([torch.cross(Q, ng, dim=-1), ng], -1).double()
        Jw = J * ok[..., None]
        n = ok.sum(-1).double()
        H = torch.einsum("kpi,kpj->kij", Jw, J) + (p.damping * n + 1e-9)[:, None, None] * eye6
        g = torch.einsum("kpi,kp->ki", Jw, torch.where(ok, r, torch.zeros_like(r)).double())
        xi = torch.linalg.solve(H, -g)
        a = 0.5 * xi[:, :3]
        s = (2.0 / (1.0 + (a * a).sum(-1)))[:, None, None]
        A = torch.zeros((k, 3, 3), dtype=torch.float64, device=dev)
        A[:, 0, 1], A[:, 0, 2], A[:, 1, 0], A[:, 1, 2], A[:, 2, 0], A[:, 2, 1] = -a[:, 2], a[:, 1], a[:, 2], -a[:, 0], -a[:, 1], a[:, 0]
        R = torch.eye(3, dtype=torch.float64, device=dev) + s * (A + A @ A)
        D = torch.cat([R @ D[:, :, :3], R @ D[:, :, 3:] + xi[:, 3:, None]], -1)
    return D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--candidates", type=int, default=512)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    api = sf.load()
    s, maps, mp = build_maps(api, a.streams, a.frames)
    n = len(maps)
    rows, cols = s.rows, s.cols
    counts = [m.info()["count"] for m in maps]
    res = dict(streams=n, frames=a.frames, candidates=a.candidates, iterations=a.iterations, surfels_per_map=int(np.median(counts)),
               copy_gbs=round(s.microbench_copy(256 << 20, 10), 1))
    print("%d maps, median %d surfels; device copy %.0f GB/s" % (n, res["surfels_per_map"], res["copy_gbs"]))
    # what the route without the feature needs beside the rendered images, as torch tensors: set-up, untimed
    zf = torch.from_numpy(np.stack([s.current(q)[0] for q in range(n)])).cuda()
    width = max(counts)
    normals = torch.zeros((n, width, 3), dtype=torch.float32, device="cuda")
    for q, m in enumerate(maps):
        normals[q, :counts[q]] = torch.from_numpy(np.ascontiguousarray(m.download()[:, 8:11])).cuda()
    rng = np.random.default_rng(1)

    def displaced(v0, xi):
        v = view.default_view(s, maps[0])
        T = (view.view_pose(v0).astype(np.float64) @ se3_exp(xi)).astype(np.float32)
        v.pose[:] = [float(x) for x in T.T.ravel()]
        return v

    def case(tag, ms, vs, st, fz, nw, stride):
        k = len(ms)
        p = align.Params(iterations=a.iterations, stride=stride, use_b=False, damping=1e-6)
        depth = torch.zeros((k, rows, cols), dtype=torch.float32, device="cuda")
        index = torch.zeros((k, rows, cols), dtype=torch.int32, device="cuda")
        t_inv = torch.from_numpy(np.stack([np.linalg.inv(view.view_pose(v).astype(np.float64))[:3, :3] for v in vs]).astype(np.float32)).cuda()
        torch.cuda.synchronize()
        dp, ip = [depth[q].data_ptr() for q in range(k)], [index[q].data_ptr() for q in range(k)]
        out = {}

        def with_feature():
            out["align"] = align.refine_streams(ms, vs, st, p)

        def without():
            view.render_device(ms, vs, dp, None, ip)
            s.synchronize()  # the steps run on torch's stream
            out["torch"] = torch_refine(depth, index, nw, t_inv, fz, vs[0], p).cpu().numpy()

        t = tag + "_stride%d" % stride
        res[t + "_refine_ms"] = median_ms(s, with_feature)
        res[t + "_render_torch_ms"] = median_ms(s, without)
        lin = k * (a.iterations + 1)
        res[t + "_us_per_entry_iteration"] = 1e3 * res[t + "_refine_ms"] / lin
        res[t + "_torch_us_per_entry_iteration"] = 1e3 * res[t + "_render_torch_ms"] / lin
        r = out["align"]
        T0 = np.stack([view.view_pose(v).astype(np.float64) for v in vs])
        D4 = np.concatenate([out["torch"], np.tile(np.array([[[0.0, 0.0, 0.0, 1.0]]]), (k, 1, 1))], 1)
        theirs = T0 @ D4
        ours = np.stack([align.pose_matrix(r[q]).astype(np.float64) for q in range(k)])
        ran = r["status"] == align.OK
        res[t + "_ok"] = int(ran.sum())
        res[t + "_max_pose_difference"] = float(np.abs(ours - theirs)[ran].max()) if ran.any() else None
        sub = ((rows + stride - 1) // stride) * ((cols + stride - 1) // stride)
        # per entry: keys cleared and read, rays, the model image written; per linearisation: the frame and up to one 32-byte gather per pixel
        res[t + "_model_bytes"] = int(sum(m.info()["count"] for m in ms) * 48 + k * rows * cols * (8 + 8 + 16 + 32) + lin * sub * (4 + 32))
        res[t + "_median_pairs_last"] = int(np.median(r["n_last"]))
        print("(%s) %d entries %dx%d stride %d, %d iterations: sfa_refine_streams %.3f ms (%.2f us per entry and iteration) | render depth + index, torch "
              "steps %.3f ms (%.2f us) = %.1f x | %d entries OK, median %d pairs, largest pose difference between the routes %s"
              % (tag, k, cols, rows, stride, a.iterations, res[t + "_refine_ms"], res[t + "_us_per_entry_iteration"], res[t + "_render_torch_ms"],
                 res[t + "_torch_us_per_entry_iteration"], res[t + "_render_torch_ms"] / res[t + "_refine_ms"], res[t + "_ok"], res[t + "_median_pairs_last"],
                 res[t + "_max_pose_difference"]))

    own = [view.default_view(s, m) for m in maps]
    shifted = [displaced(v, np.array([0.02, -0.01, 0.02, 0.01, -0.01, 0.01])) for v in own]
    cand = [own[0]] + [displaced(own[0], np.concatenate([rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.03, 0.03, 3)])) for _ in range(a.candidates - 1)]
    for stride in (1, 4):
        case("a", maps, shifted, list(range(n)), zf, normals, stride)
        case("b", [maps[0]] * len(cand), cand, [0] * len(cand), zf[:1], normals[:1], stride)
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
