"""The carve (include/sf_carve.h) on one MI355X: what carving one map of 10^5 and of 10^6 surfels by 1, 4 and 16 QVGA frames
costs, and 256 maps of 4096 surfels by 4 frames each, with two yardsticks measured in the same process and the same rounds,
alternating: map_window.cull of the same maps at the same kept fraction -- it reads the same 48 B per surfel and runs the same
scan and the same ordered write, so it is the floor of what a carve can cost -- and sf_microbench_copy of the same bytes.

A map is a wall 2 m in front of a camera at the origin, one surfel per cell of a jittered grid in the map's point order,
facing the camera. The frames see the wall where it is on the right half of the image (SUPPORTED) and one metre behind it on the
left half (THROUGH), from poses a few millimetres apart, so the left half of every map is carved (min_votes 1); the cull keeps
the same number of surfels by a confidence threshold. Both calls return after their counts are in host memory, so a round
brackets each call with a host clock (the call itself drains the handle's stream); the maps are uploaded again before every
call, outside the bracket. The figures are medians over the rounds, with the smallest and the largest beside them.

NOT measured here: the kernel alone (a run under a kernel-tracing profiler gives it), other windows than the default 3 x 3,
host images (the frames are read from the handle's stream, as sfe_carve_streams does), real maps.

usage: python tools/carve_bench.py [--rounds 10] [--json FILE]
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
from staticfusion_amd import carve, map_window, view

ROWS, COLS, F = 240, 320, 280.0


def wall(n, seed):
    """n surfels on a wall at z = 2 that fills the view, x outer and y inner, facing the camera; the left half gets confidence
    0.1, the right half 1: the cull's threshold keeps what the carve keeps"""
    rng = np.random.default_rng(seed)
    nx = int(np.ceil(np.sqrt(n * COLS / ROWS)))
    ny = -(-n // nx)
    gx, gy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    u = ((gx.ravel()[:n] + rng.uniform(0.2, 0.8, n)) / nx) * (COLS - 4) + 1.5
    v = ((gy.ravel()[:n] + rng.uniform(0.2, 0.8, n)) / ny) * (ROWS - 4) + 1.5
    s = np.zeros((n, 12), np.float32)
    s[:, 0], s[:, 1], s[:, 2] = (u - COLS / 2) * 2.0 / F, (v - ROWS / 2) * 2.0 / F, 2.0
    s[:, 3] = np.where(u < COLS / 2, 0.1, 1.0)
    s[:, 4], s[:, 5], s[:, 6], s[:, 7], s[:, 10], s[:, 11] = 0x808080, 1.0, 1.0, 1.0, -1.0, 2.0 / F
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    api = sf.load()
    p = api.default_params_struct()
    s = sf.Solver(api, ROWS, COLS, 1, p)
    depth = np.full((ROWS, COLS), 2.0, np.float32)
    depth[:, :COLS // 2] = 3.0
    s.set_current(0, depth, np.full_like(depth, 0.5))
    eye = np.eye(4, dtype=np.float32)
    crv = carve.Carver(s)
    cases = [(1, 100000, k) for k in (1, 4, 16)] + [(1, 1000000, k) for k in (1, 4, 16)] + [(256, 4096, 4)]
    rows, clocks = [], []
    for n_maps, count, frames in cases:
        surf = [wall(count, 7 + m) for m in range(min(n_maps, 4))]
        maps = [sf.SurfelMap(s, max(count, ROWS * COLS)) for _ in range(n_maps)]  # (a map holds at least one frame)
        entries = []
        for m in range(n_maps):
            for k in range(frames):
                T = eye.copy()
                T[0, 3], T[1, 3] = 0.001 * k, -0.001 * (m % 7)
                entries.append((m, view.View(T, COLS / 2, ROWS / 2, F, F, ROWS, COLS, min_confidence=0.0), 0))
        cp, flt = carve.Params(min_votes=1), [map_window.Filter(min_confidence=0.5)] * n_maps
        bytes_moved = n_maps * count * 48

        def fill():
            for m, mp in enumerate(maps):
                mp.upload(surf[m % len(surf)], eye, 2)
            s.synchronize()

        t = dict(carve=[], cull=[], copy=[])
        out = {}
        for r in range(a.rounds + 1):  # round 0 warms: block growth, code objects
            fill()
            t0 = time.perf_counter()
            out["carve"] = crv.carve(maps, cp, entries)
            t1 = time.perf_counter()
            fill()
            t2 = time.perf_counter()
            out["cull"] = map_window.cull(maps, flt)
            t3 = time.perf_counter()
            gbs = s.microbench_copy(max(bytes_moved, 1 << 20), 5)
            if r:
                t["carve"].append(1e3 * (t1 - t0))
                t["cull"].append(1e3 * (t3 - t2))
                t["copy"].append(1e3 * 2 * max(bytes_moved, 1 << 20) / (gbs * 1e9))
        kept_carve, kept_cull = sum(c["n_out"] for c in out["carve"]), sum(out["cull"])
        med = {k: float(np.median(v)) for k, v in t.items()}
        pairs = n_maps * count * frames
        row = dict(maps=n_maps, surfels_per_map=count, frames_per_map=frames, rounds=a.rounds, carve_ms=round(med["carve"], 3), cull_ms=round(med["cull"], 3),
                   copy_ms=round(med["copy"], 3), spread_ms={k: [round(min(v), 3), round(max(v), 3)] for k, v in t.items()},
                   ns_per_surfel_entry=round(1e6 * med["carve"] / pairs, 3), carve_over_cull=round(med["carve"] / med["cull"], 2),
                   kept_by_carve=int(kept_carve), kept_by_cull=int(kept_cull), through=int(sum(c["n_through"] for c in out["carve"])),
                   supported=int(sum(c["n_supported"] for c in out["carve"])))
        rows.append(row)
        print("%4d map(s) x %7d surfels x %2d frame(s): carve %8.3f ms (%6.3f ns per surfel-entry), cull %8.3f ms, copy of the same bytes %7.3f ms, carve / cull %5.2f; "
              "kept %d / %d" % (n_maps, count, frames, med["carve"], row["ns_per_surfel_entry"], med["cull"], med["copy"], row["carve_over_cull"], kept_carve, kept_cull))
        for mp in maps:
            mp.close()
        try:
            clocks.append(int(torch.cuda.clock_rate()))
        except Exception:
            pass
    res = dict(rows=rows, device=torch.cuda.get_device_name(0), shader_clock_mhz=clocks)
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    crv.close()
    s.close()


if __name__ == "__main__":
    main()
