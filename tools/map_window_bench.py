"""What a cull costs (include/sf_map_window.h): M maps of N surfels each, a filter that keeps a given fraction of every map
(the kept surfels scattered through the buffer), all maps in one sfw_cull_maps.

Reports, per load policy of the record reads (SF_WINDOW_POLICY: default, nt = the move pass non-temporal, nt2 = both passes):
  - wall milliseconds of the call (it returns after the counts have been read back, so the clock covers the table upload,
    the three launches and the read-back), median of --reps calls, each on freshly uploaded maps;
  - the bytes of the MODEL of DESIGN.md section 18 (per kept surfel 48 B read by the predicate pass + 48 B read + 48 B written
    by the move; per dropped surfel 96 B read) divided by that time;
beside them Solver.microbench_copy of the same number of bytes on the same box (the streaming ceiling a device copy reaches),
and the route the call replaces: sf_map_download, a NumPy filter, sf_map_upload, per map.

usage: python tools/map_window_bench.py [--maps 64] [--surfels 100000] [--keep 0.5] [--reps 5] [--json OUT]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import staticfusion_amd as sf
from staticfusion_amd import map_window

TICK = 20
POLICIES = ("default", "nt", "nt2")


def model_bytes(kept, dropped):
    return 144 * kept + 96 * dropped


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=64)
    ap.add_argument("--surfels", type=int, default=100000)
    ap.add_argument("--keep", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    api = sf.load()
    s = sf.Solver(api, 120, 160, 1, api.default_params_struct())
    M, N = a.maps, a.surfels
    rng = np.random.default_rng(5)
    surf = rng.uniform(-1.0, 1.0, (N, 12)).astype(np.float32)
    recent = rng.uniform(0.0, 1.0, N) < a.keep
    surf[:, 7] = np.where(recent, TICK - 1, TICK - 10)
    keep = map_window.Filter(max_age=1)
    kept, dropped = int(recent.sum()) * M, int((~recent).sum()) * M
    maps = [sf.SurfelMap(s, max(N, 120 * 160)) for _ in range(M)]
    pose = np.eye(4, dtype=np.float32)

    def fill():
        for m in maps:
            m.upload(surf, pose, TICK)

    out = dict(maps=M, surfels=N, keep=a.keep, kept=kept, dropped=dropped, model_bytes=model_bytes(kept, dropped), reps=a.reps, policies={})
    print("%d maps x %d surfels, %.0f %% kept: the model moves %.1f MB per cull" % (M, N, 100.0 * kept / (kept + dropped), out["model_bytes"] / 1e6))
    times = {p: [] for p in POLICIES}
    for rep in range(a.reps + 1):  # the first round warms up (code objects, the handle's tables); the policies alternate
        for p in POLICIES:
            os.environ["SF_WINDOW_POLICY"] = p
            fill()
            s.synchronize()
            t0 = time.perf_counter()
            got = map_window.cull(maps, [keep] * M)
            dt = time.perf_counter() - t0
            assert sum(got) == kept, (sum(got), kept)
            if rep:
                times[p].append(dt)
    del os.environ["SF_WINDOW_POLICY"]
    for p in POLICIES:
        ms = 1e3 * float(np.median(times[p]))
        out["policies"][p] = dict(ms=ms, ms_all=[1e3 * t for t in times[p]], model_gb_s=out["model_bytes"] / (ms * 1e-3) / 1e9)
        print("  sfw_cull_maps, loads %-8s %8.3f ms (min %.3f, max %.3f)   %7.1f GB/s of the model" % (p, ms, 1e3 * min(times[p]), 1e3 * max(times[p]), out["policies"][p]["model_gb_s"]))
    nbytes = min(M * N * 48, 1 << 30)
    out["copy_gb_s"] = float(s.microbench_copy(nbytes, 20))
    out["copy_bytes"] = nbytes
    print("  device copy of %.0f MB (microbench_copy, read + write counted): %.1f GB/s" % (nbytes / 1e6, out["copy_gb_s"]))
    # the route the call replaces, on a few maps (it is per map anyway)
    few = maps[: min(M, 4)]
    fill()
    host = []
    for m in few:
        t0 = time.perf_counter()
        info, d = m.info(), m.download()
        d = d[(np.float32(info["tick"]) - d[:, 7]) <= np.float32(1)]
        m.upload(d, info["pose"], info["tick"])
        host.append(time.perf_counter() - t0)
    out["host_route_ms_per_map"] = 1e3 * float(np.median(host))
    best = min(out["policies"][p]["ms"] for p in POLICIES)
    print("  download + NumPy + upload: %.3f ms per map = %.1f ms for %d maps (the cull: %.3f ms for all of them, %.0f x)"
          % (out["host_route_ms_per_map"], out["host_route_ms_per_map"] * M, M, best, out["host_route_ms_per_map"] * M / best))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    for m in maps:
        m.close()
    s.close()


if __name__ == "__main__":
    main()
