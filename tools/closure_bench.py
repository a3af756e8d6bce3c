"""Closure constraints (include/sf_closure.h) on one MI355X: what building the constraints of 256 and of 4096 QVGA closures in one
call costs at stride 4, with the 2n scores of the same (map, view) pairs (score.score_images_device: the same 2n draws, then
one pass over every pixel instead of one over every sixteenth) measured in the same rounds, alternating.

The expectation to test: the two draws dominate, and a build costs about what those 2n scores cost.

One map of one surfel per pixel of a 320 x 240 wall serves as map_new of every entry, a second -- the same wall under another
noise -- as map_old; the views of the entries differ by a small translation each, so every entry draws both maps anew. A round
runs the two calls one after the other, each bracketed by a host clock around the call and a synchronisation of the handle's
stream; the figures are medians over the rounds, with the smallest and the largest beside them. A build returns after its
counts and its records have been read back, so its bracket holds the uploads of the tables, the drawing stage, the counting
pass, the scan, one synchronisation for the counts, the writing pass and the copy of the records; the score's bracket holds
its uploads, the drawing stage and its kernel (its records stay on the device). Beside the build, the same call as a size
query (out == NULL: everything up to the counts, no writing pass and no records copied out) is timed too, which separates the
device work from the copy of the records into host memory.

NOT measured here: the kernels alone (a run under a kernel-tracing profiler gives them), other strides, entries of different
sizes, maps that differ between the entries.

usage: python tools/closure_bench.py [--rounds 20] [--entries 256 4096] [--json FILE]
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
from staticfusion_amd import closure, score, view

ROWS, COLS, F = 240, 320, 280.0


def wall(seed, t_init):
    """one surfel per pixel of a wall 2 m in front of a camera at the origin, 2 cm of noise, facing the camera"""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(COLS) + 0.5, np.arange(ROWS) + 0.5)
    z = 2.0 + rng.normal(0, 0.02, u.shape)
    s = np.zeros((ROWS * COLS, 12), np.float32)
    s[:, 0], s[:, 1], s[:, 2] = ((u - COLS / 2) * z / F).ravel(), ((v - ROWS / 2) * z / F).ravel(), z.ravel()
    s[:, 3], s[:, 4], s[:, 5], s[:, 6], s[:, 7], s[:, 10] = 1.0, 0x808080, 1.0, t_init, t_init, -1.0
    s[:, 11] = z.ravel() / F
    return s


def timed(s, fn):
    t0 = time.perf_counter()
    fn()
    s.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--entries", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    api = sf.load()
    s = sf.Solver(api, 120, 160, 1, api.default_params_struct())  # (the handle only owns the stream here)
    eye = np.eye(4, dtype=np.float32)
    m_new, m_old = sf.SurfelMap(s, ROWS * COLS), sf.SurfelMap(s, ROWS * COLS)
    m_new.upload(wall(1, 20.0), eye, 21)
    m_old.upload(wall(2, 1.0), eye, 21)
    bld = closure.Builder(s)
    depth = torch.full((COLS, ROWS), 2.0, dtype=torch.float32, device="cuda")  # column-major, like every image of sf.h
    rows = []
    for n in a.entries:
        poses = []
        for q in range(n):
            T = eye.copy()
            T[0, 3], T[1, 3] = 0.0005 * (q % 64), 0.0005 * (q // 64)
            poses.append(T)
        vf = [view.View(T, COLS / 2, ROWS / 2, F, F, ROWS, COLS, min_confidence=0.0) for T in poses]
        vt = [view.View(T, COLS / 2, ROWS / 2, F, F, ROWS, COLS, min_confidence=0.0) for T in poses]
        cp = closure.Params(stride=4)
        pair_maps = [m for _ in range(n) for m in (m_new, m_old)]
        pair_views = [v for q in range(n) for v in (vf[q], vt[q])]
        records = torch.zeros((2 * n, 12), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        sp = score.Params(use_grey=False, use_b=False)
        dp = [depth.data_ptr()] * (2 * n)
        out = {}

        def build():
            out["build"] = bld.build([m_new] * n, [m_old] * n, vf, vt, cp)

        calls = dict(build=build, count=lambda: bld.sizes([m_new] * n, [m_old] * n, vf, vt, cp), score=lambda: score.score_images_device(pair_maps, pair_views, dp, None, None, sp, records.data_ptr()))
        for fn in calls.values():  # warm-up: block growth, code objects
            timed(s, fn)
        t = {k: [] for k in calls}
        for _ in range(a.rounds):
            for k, fn in calls.items():
                t[k].append(timed(s, fn))
        med = {k: float(np.median(v)) for k, v in t.items()}
        recs, counts = out["build"]
        n_both = int(records.cpu().numpy()[:, 3].sum())
        row = dict(entries=n, stride=4, rounds=a.rounds, build_ms=round(med["build"], 3), count_only_ms=round(med["count"], 3), score_2n_ms=round(med["score"], 3),
                   spread_ms={k: [round(min(v), 3), round(max(v), 3)] for k, v in t.items()}, build_over_score=round(med["build"] / med["score"], 3),
                   count_over_score=round(med["count"] / med["score"], 3),
                   records=int(recs.shape[0]), links=int(sum(c["n_links"] for c in counts)), samples=int(sum(c["n_samples"] for c in counts)),
                   score_n_both=n_both)
        rows.append(row)
        print("%5d QVGA entries at stride 4: build %9.3f ms (%7.1f us per entry, %d records), its counts alone %9.3f ms, the 2n scores %9.3f ms, "
              "build / scores %5.2f, counts alone / scores %5.2f"
              % (n, med["build"], 1e3 * med["build"] / n, row["records"], med["count"], med["score"], row["build_over_score"], row["count_over_score"]))
    print(json.dumps(dict(rows=rows)))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(dict(rows=rows), fh, indent=1)
            fh.write("\n")
    bld.close()
    for m in (m_new, m_old):
        m.close()
    s.close()


if __name__ == "__main__":
    main()
