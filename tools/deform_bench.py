"""Deformation graphs (include/sf_deform.h) on one MI355X: what bending a map of 10^5 and of 10^6 surfels costs under graphs of 64,
256 and 1024 nodes, with the rigid move of the body maps (sfp_move_maps, the same 96 bytes per surfel read and written: the
memory-bound floor of any in-place pass over a map) on the same map beside every figure.

Surfels and nodes are uniform in a 4 m cube; the transforms are identities (the arithmetic is the same and the map stays where
it is, so every round sees the same input). A round runs the two calls one after the other -- the apply and the move --, each
bracketed by a host clock around the call and a synchronisation of the handle's stream; the figures are medians over the rounds, with the
smallest and the largest beside them. An apply returns after its counts have been read back, so its bracket holds the upload of
the nodes, the kernel and one small device-to-host copy; the move's bracket holds its table upload and its kernel.

Pairs per second = surfels x nodes / time of the apply: the distance tests of the brute-force search.

NOT measured here: the time of the kernel alone (a run under a kernel-tracing profiler gives it), clustered surfels (a wave
whose lanes agree on their nearest nodes takes fewer insertion branches), finite time windows, several maps per call.

usage: python tools/deform_bench.py [--rounds 20] [--json FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import staticfusion_amd as sf
from staticfusion_amd import body_maps, deform


def timed(s, fn):
    t0 = time.perf_counter()
    fn()
    s.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    api = sf.load()
    s = sf.Solver(api, 120, 160, 1, api.default_params_struct())  # (the handle only owns the stream here)
    rng = np.random.default_rng(1)
    rows = []
    for n in (100_000, 1_000_000):
        surf = np.zeros((n, 12), np.float32)
        surf[:, 0:3] = rng.uniform(0, 4, (n, 3))
        surf[:, 3] = 1.0
        surf[:, 10] = 1.0
        m = sf.SurfelMap(s, n)
        m.upload(surf, np.eye(4, dtype=np.float32), 2)
        for G in (64, 256, 1024):
            g = deform.Graph(s)
            g.set(rng.uniform(0, 4, (G, 3)).astype(np.float32), np.zeros(G, np.float32))
            calls = dict(apply=lambda: deform.apply_maps([m], g), move=lambda: body_maps.move([m]))
            for fn in calls.values():  # warm-up: block growth, code objects
                timed(s, fn)
            t = {k: [] for k in calls}
            for _ in range(a.rounds):
                for k, fn in calls.items():
                    t[k].append(timed(s, fn))
            med = {k: float(np.median(v)) for k, v in t.items()}
            row = dict(surfels=n, nodes=G, rounds=a.rounds, apply_ms=round(med["apply"], 4), move_ms=round(med["move"], 4),
                       spread_ms={k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()}, apply_over_move=round(med["apply"] / med["move"], 2),
                       gpairs_per_s=round(n * G / med["apply"] / 1e6, 1), move_gbs=round(n * 96 / med["move"] / 1e6, 1))
            rows.append(row)
            print("%8d surfels %5d nodes: apply %8.3f ms, move %7.3f ms, apply / move %6.2f, %7.1f G pairs/s"
                  % (n, G, med["apply"], med["move"], row["apply_over_move"], row["gpairs_per_s"]))
            g.close()
        assert np.abs(m.download()[:, 0:3] - surf[:, 0:3]).max() < 1e-3  # identities: the map is where it was, to rounding
        m.close()
    print(json.dumps(dict(rows=rows)))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(dict(rows=rows), fh, indent=1)
            fh.write("\n")
    s.close()


if __name__ == "__main__":
    main()
