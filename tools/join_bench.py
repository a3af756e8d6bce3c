"""Joined and thinned maps (include/sf_join.h) on one MI355X: what a thin and a merge cost beside the route a caller had
without them.

The maps are what tools/full_pipeline_bench.py leaves (tools/view_bench.py build_maps): N sequences through predict -> input ->
solve -> fuse for 10 QVGA frames of a synthetic walk. Every figure is the median of 5 calls, each bracketed by a synchronisation
of the handle's stream, in one process with sf_microbench_copy (the streaming ceiling of the box at that moment). A thin and a
merge change their maps, so before every timed call the maps are uploaded again from host copies, outside the timed part.

  (a) sfj_thin_maps of all N maps in one call, at cells of 0.01, 0.02 and 0.05 m
  (b) sfj_merge_maps of N / 2 pairs in one call (map 2 i + 1 into map 2 i, displaced by a small rigid motion), cell 0.02 m
Beside each, in the same process, the route without the feature, map by map in torch on the device: int64 voxel keys,
torch.unique with the inverse, a scatter_reduce("amax") of (rank, index) per voxel, the mask and the compaction (thin);
the keys of both maps, torch.isin and the concatenation (merge). The torch route's keys come from the same fp32 multiply and
floor, so its counts equal the call's; the tool checks that and says so.

No rate is asserted anywhere; the figures are what they are on the box the tool ran on.

usage: python tools/join_bench.py [--streams 256] [--frames 10] [--json FILE]
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
from staticfusion_amd import join
from staticfusion_amd.synth import se3_exp
from view_bench import build_maps

BIAS = 1 << 20


def torch_keys(pos, inv):
    """(int64 keys, inside) of n x 3 float32 positions: include/sf_join.h, VOXEL KEY"""
    q = torch.floor(pos * inv)
    inside = torch.isfinite(pos).all(1) & torch.isfinite(q).all(1) & (q.abs() < float(BIAS)).all(1)
    qi = torch.where(inside[:, None], q, torch.zeros_like(q)).long() + BIAS
    return (qi[:, 0] << 42) | (qi[:, 1] << 21) | qi[:, 2], inside


def torch_thin(surf, inv):
    keys, inside = torch_keys(surf[:, 0:3], inv)
    n = surf.shape[0]
    idx = torch.arange(n, device=surf.device)
    u = surf[:, 3].contiguous().view(torch.int32).long() & 0xFFFFFFFF
    rank = torch.where(u >= 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    rank = torch.where((u & 0x7FFFFFFF) > 0x7F800000, torch.zeros_like(rank), rank)
    bid = (rank << 31) | (0x7FFFFFFF - idx)  # the higher rank, then the lower index
    _, inverse = torch.unique(keys[inside], return_inverse=True)
    best = torch.zeros(int(inverse.max()) + 1 if inverse.numel() else 1, dtype=torch.int64, device=surf.device)
    best.scatter_reduce_(0, inverse, bid[inside], "amax")
    keep = ~inside
    keep[inside] = best[inverse] == bid[inside]
    return surf[keep]


def torch_merge(dst, src, T, inv):
    moved = src.clone()
    moved[:, 0:3] = src[:, 0:3] @ T[:3, :3].T + T[:3, 3]
    moved[:, 8:11] = src[:, 8:11] @ T[:3, :3].T
    dkeys, dinside = torch_keys(dst[:, 0:3], inv)
    skeys, sinside = torch_keys(moved[:, 0:3], inv)
    shared = sinside & torch.isin(skeys, torch.unique(dkeys[dinside]))
    return torch.cat([dst, moved[~shared]])


def timed(s, prepare, fn, calls=5):
    """median ms of fn(), prepare() before every call outside the timed part; the first pair is a warm-up"""
    t = []
    for k in range(calls + 1):
        prepare()
        s.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        s.synchronize()
        torch.cuda.synchronize()
        if k:
            t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    api = sf.load()
    s, maps, mp = build_maps(api, a.streams, a.frames)
    n = len(maps)
    host = [m.download() for m in maps]
    infos = [m.info() for m in maps]
    counts = [h.shape[0] for h in host]
    total = int(sum(counts))
    res = dict(streams=n, frames=a.frames, surfels_per_map=int(np.median(counts)), surfels=total, copy_gbs=round(s.microbench_copy(256 << 20, 10), 1))
    print("%d maps, median %d surfels; device copy %.0f GB/s" % (n, res["surfels_per_map"], res["copy_gbs"]))
    dev = [torch.from_numpy(h).cuda() for h in host]  # the route without the feature works on torch tensors: set-up, untimed

    def restore(which):
        for q in which:
            maps[q].upload(host[q], infos[q]["pose"], infos[q]["tick"])

    out = {}
    for cell in (0.01, 0.02, 0.05):
        p = join.Params(cell=cell)
        inv = float(np.float32(1.0) / np.float32(cell))
        tag = "thin_cell%g" % cell

        def with_feature():
            out["counts"] = join.thin(maps, p)

        def without():
            out["torch"] = [torch_thin(d, inv) for d in dev]

        res[tag + "_ms"] = timed(s, lambda: restore(range(n)), with_feature)
        restore(range(n))
        res[tag + "_dry_run_ms"] = timed(s, lambda: None, lambda: join.thin(maps, join.Params(cell=cell, dry_run=True)))
        res[tag + "_torch_ms"] = timed(s, lambda: None, without)
        kept = sum(c["n_out"] for c in out["counts"])
        res[tag + "_kept"] = int(kept)
        res[tag + "_voxels"] = int(sum(c["n_voxels"] for c in out["counts"]))
        res[tag + "_same_counts"] = bool([c["n_out"] for c in out["counts"]] == [t.shape[0] for t in out["torch"]])
        res[tag + "_msurfels_per_s"] = total / res[tag + "_ms"] / 1e3
        res[tag + "_map_gbs"] = (total + kept) * 48 / res[tag + "_ms"] / 1e6  # the map read once, the kept part written once
        print("(a) thin %d maps, cell %g: sfj_thin_maps %.3f ms (%.0f M surfels/s, map read + kept written = %.0f GB/s; counts only %.3f ms) | torch unique + "
              "scatter_reduce, map by map %.3f ms = %.1f x | kept %d of %d, counts equal: %s"
              % (n, cell, res[tag + "_ms"], res[tag + "_msurfels_per_s"], res[tag + "_map_gbs"], res[tag + "_dry_run_ms"], res[tag + "_torch_ms"],
                 res[tag + "_torch_ms"] / res[tag + "_ms"], kept, total, res[tag + "_same_counts"]))
    # ---- merge of pairs
    pairs = n // 2
    if pairs:
        dst, src = [maps[2 * i] for i in range(pairs)], [maps[2 * i + 1] for i in range(pairs)]
        T = se3_exp(np.array([0.013, -0.008, 0.011, 0.004, -0.006, 0.005])).astype(np.float32)
        Td = torch.from_numpy(T).cuda()
        p = join.Params(cell=0.02)
        inv = float(np.float32(1.0) / np.float32(0.02))

        def with_feature():
            out["counts"] = join.merge(dst, src, [T] * pairs, p)

        def without():
            out["torch"] = [torch_merge(dev[2 * i], dev[2 * i + 1], Td, inv) for i in range(pairs)]

        res["merge_ms"] = timed(s, lambda: restore(range(0, 2 * pairs, 2)), with_feature)
        restore(range(0, 2 * pairs, 2))
        res["merge_torch_ms"] = timed(s, lambda: None, without)
        added = sum(c["n_out"] for c in out["counts"])
        examined = sum(c["n_in"] for c in out["counts"])
        res["merge_pairs"], res["merge_added"], res["merge_shared"] = pairs, int(added), int(sum(c["n_shared"] for c in out["counts"]))
        # the torch route multiplies by T in another order: a surfel next to a cell border may fall on the other side
        res["merge_count_difference"] = int(sum(abs(c["n_out"] - (t.shape[0] - counts[2 * i])) for i, (c, t) in enumerate(zip(out["counts"], out["torch"]))))
        res["merge_msurfels_per_s"] = (examined + sum(counts[0:2 * pairs:2])) / res["merge_ms"] / 1e3
        print("(b) merge %d pairs, cell 0.02: sfj_merge_maps %.3f ms (%.0f M surfels/s inserted or examined) | torch unique + isin + cat, pair by pair %.3f ms "
              "= %.1f x | added %d of %d, shared %d; added counts of the two routes differ by %d in all"
              % (pairs, res["merge_ms"], res["merge_msurfels_per_s"], res["merge_torch_ms"], res["merge_torch_ms"] / res["merge_ms"], added, examined,
                 res["merge_shared"], res["merge_count_difference"]))
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
