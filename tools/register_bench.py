"""The map registration (include/sf_register.h) on one MI355X: what registering one source of 10^5 and of 10^6 surfels against a
destination of the same size costs at 10 iterations, and 256 entries of 4096 surfels each in one call, with two yardsticks measured
in the same process and the same rounds, alternating: join.thin(dry_run) of the same destination(s) at the same cell -- it
clears and fills the same voxel table with the same insert kernel (and adds a flag pass and a scan), so it is the cost of the
table -- and sf_microbench_copy of the bytes ONE linearisation reads at the least: per sampled surfel 32 B of its own (position
and normal), eight key words of 8 B, one bid of 8 B and 32 B of its partner (position and normal), 136 B. The copy is the floor
of one linearisation; a call makes iterations + 1 of them.

A destination is a corner of three perpendicular planes, one surfel per cell of a jittered 5 mm grid; the source is the same
surfels in reversed order, moved by the inverse of a small motion, and the call starts from the identity. All three calls return
after their results are in host memory, so a round brackets each with a host clock (the call itself drains the handle's stream).
The maps are uploaded once: no call changes them. The figures are medians over the rounds, with the smallest and the largest
beside them.

NOT measured here: the kernels alone (a run under a kernel-tracing profiler gives them), the share of the probes, of the
gathers and of the reduction, other cells than 0.1 m, strides, real maps.

usage: python tools/register_bench.py [--rounds 10] [--json profiles/register_bench.json]
"""
import argparse
import json
import os
import sys
import time

import torch  # first, as bench.py does: the process then holds the HIP runtime torch brought

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import staticfusion_amd as sf
from staticfusion_amd import join, register

ROWS, COLS = 60, 80
SPACING = 0.005
BYTES_PER_SAMPLED = 32 + 8 * 8 + 8 + 32


def corner(n, seed):
    """about n surfels (exactly n: the rest of the third plane is cut) on three planes through (0.3, -0.2, 1)"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n / 3.0)))
    out = []
    for ax in range(3):
        u, v = [a for a in (0, 1, 2) if a != ax]
        gi, gj = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
        s = np.zeros((side * side, 12), np.float32)
        p = np.tile(np.array([0.3, -0.2, 1.0]), (side * side, 1))
        p[:, u] += (gi.ravel() + rng.uniform(0.1, 0.9, side * side)) * SPACING
        p[:, v] += (gj.ravel() + rng.uniform(0.1, 0.9, side * side)) * SPACING
        s[:, 0:3] = p
        s[:, 8 + ax] = 1.0
        out.append(s)
    s = np.concatenate(out)[:n]
    s[:, 3] = rng.uniform(0.25, 0.75, n)
    s[:, 4], s[:, 6], s[:, 7], s[:, 11] = 0x808080, 1.0, 1.0, SPACING
    return s


def moved(surfels, w=(0.006, -0.004, 0.003), t=(0.004, -0.002, 0.003)):
    """the surfels in reversed order, in a frame from which a rotation by about w (radians) and a translation t lead back"""
    wx, wy, wz = w
    K = np.array([[0, -wz, wy], [wz, 0, -wx], [-wy, wx, 0]], np.float64)
    R = np.eye(3) + K + K @ K / 2
    R, _ = np.linalg.qr(R)
    R = R * np.sign(np.diag(R))
    s = np.array(surfels[::-1], np.float32)
    s[:, 0:3] = ((s[:, 0:3].astype(np.float64) - np.array(t)) @ R).astype(np.float32)
    s[:, 8:11] = (s[:, 8:11].astype(np.float64) @ R).astype(np.float32)
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    api = sf.load()
    s = sf.Solver(api, ROWS, COLS, 1, api.default_params_struct())
    eye = np.eye(4, dtype=np.float32)
    reg = register.Registrar(s)
    rp, jp = register.Params(iterations=10), join.Params(cell=0.1, dry_run=True)
    rows, clocks = [], []
    for n_entries, count in ((1, 100000), (1, 1000000), (256, 4096)):
        dst_s = [corner(count, 7 + m) for m in range(min(n_entries, 4))]
        src_s = [moved(d) for d in dst_s]
        dst, src = [], []
        for m in range(n_entries):
            for store, surf in ((dst, dst_s), (src, src_s)):
                mp = sf.SurfelMap(s, max(count, ROWS * COLS))  # (a map holds at least one frame)
                mp.upload(surf[m % len(surf)], eye, 2)
                store.append(mp)
        s.synchronize()
        sampled = n_entries * count
        read_bytes = max(sampled * BYTES_PER_SAMPLED, 1 << 20)
        t = dict(register=[], thin=[], copy=[])
        res = None
        for r in range(a.rounds + 1):  # round 0 warms: block growth, code objects
            t0 = time.perf_counter()
            res = reg.register_maps(dst, src, None, rp)
            t1 = time.perf_counter()
            join.thin(dst, jp)
            t2 = time.perf_counter()
            gbs = s.microbench_copy(read_bytes, 5)
            if r:
                t["register"].append(1e3 * (t1 - t0))
                t["thin"].append(1e3 * (t2 - t1))
                t["copy"].append(1e3 * 2 * read_bytes / (gbs * 1e9))
        med = {k: float(np.median(v)) for k, v in t.items()}
        lin = int(res["iterations_done"].max()) + 1
        per = 1e6 * med["register"] / (sampled * lin)
        per_less_table = 1e6 * max(med["register"] - med["thin"], 0.0) / (sampled * lin)
        row = dict(entries=n_entries, surfels_per_map=count, iterations=10, linearisations=lin, rounds=a.rounds, register_ms=round(med["register"], 3),
                   thin_dry_run_ms=round(med["thin"], 3), copy_of_one_linearisation_ms=round(med["copy"], 3),
                   spread_ms={k: [round(min(v), 3), round(max(v), 3)] for k, v in t.items()}, ns_per_sampled_surfel_and_linearisation=round(per, 4),
                   the_same_less_the_thin=round(per_less_table, 4), one_linearisation_over_copy=round((med["register"] - med["thin"]) / lin / med["copy"], 2),
                   status=sorted(set(int(x) for x in res["status"])), n_first=int(res["n_first"].sum()), n_last=int(res["n_last"].sum()),
                   n_sampled=int(res["n_sampled"].sum()))
        rows.append(row)
        print("%4d entr%s x %7d surfels, %2d linearisations: register %9.3f ms (%7.4f ns per sampled surfel and linearisation; less the thin %7.4f), thin(dry_run) %8.3f ms, "
              "copy of one linearisation's bytes %7.3f ms, one linearisation / copy %6.2f; pairs %d -> %d of %d"
              % (n_entries, "y" if n_entries == 1 else "ies", count, lin, med["register"], per, per_less_table, med["thin"], med["copy"], row["one_linearisation_over_copy"],
                 row["n_first"], row["n_last"], row["n_sampled"]))
        for mp in dst + src:
            mp.close()
        try:
            clocks.append(int(torch.cuda.clock_rate()))
        except Exception:
            pass
    out = dict(rows=rows, bytes_per_sampled_surfel=BYTES_PER_SAMPLED, device=torch.cuda.get_device_name(0), shader_clock_mhz=clocks)
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    reg.close()
    s.close()


if __name__ == "__main__":
    main()
