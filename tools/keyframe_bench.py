"""Place recognition (include/sf_keyframes.h) on one MI355X: what encoding the current frames of B QVGA streams costs, and what
a query of the same B streams against a filled database costs.

Every figure is the median of 5 calls, each bracketed by a synchronisation of the handle's stream, in one process with
sf_microbench_copy (the streaming ceiling of the box at that moment). The calls are the host-facing ones, so a figure holds
the upload of the call's frame table, the launch and the copy of the results to host memory.

Byte model of the encode: 8 bytes per pixel of the grid (depth + grey, each read once); written: words x 4 bytes per frame.
The rate is set beside the copy rate (bytes read + bytes written per second of a plain 16-byte copy): the fraction says how
much of a streaming kernel's bandwidth the encode reaches. Byte model of the query: B x count x words x 4 bytes of database
codes, which stay in the caches when the database is small.

usage: python tools/keyframe_bench.py [--streams 2048] [--cell 8] [--ferns 256] [--slots 4096] [--json FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

import staticfusion_amd as sf
from staticfusion_amd import keyframes
from staticfusion_amd.synth import Scene, quantise_and_decimate, se3_exp
from view_bench import median_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--cell", type=int, default=8)
    ap.add_argument("--ferns", type=int, default=256)
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    api = sf.load()
    rows, cols, n = 240, 320, a.streams
    s = sf.Solver(api, rows, cols, n, api.default_params_struct())  # (the handle only holds the frames here)
    scene = Scene(seed=77, sphere=False)
    views = []
    for k in range(8):  # eight views of a room, dealt round the streams
        depth, inten = scene.render(se3_exp(np.array([0.05 * k, 0.0, 0.02 * k, 0.0, 0.04 * k - 0.14, 0.0])), 2 * cols, 2 * rows, stride=2)
        views.append(quantise_and_decimate(depth, inten, max_depth=4.5, decimate=False))
    for q in range(n):
        s.set_current(q, *views[q % 8])
    db = keyframes.KeyframeDb(s, a.cell, n_ferns=a.ferns, capacity=a.slots)
    info = db.info()
    streams = np.arange(n, dtype=np.int32)
    res = dict(streams=n, rows=rows, cols=cols, cell=a.cell, ferns=a.ferns, words=info["words"], slots=a.slots)
    copy = [s.microbench_copy(256 << 20, 10)]
    out = {}

    def encode():
        out["codes"] = db.encode_streams(streams)

    res["encode_ms"] = median_ms(s, encode)
    copy.append(s.microbench_copy(256 << 20, 10))
    assert all(np.array_equal(out["codes"][q], out["codes"][q % 8]) for q in range(n)) and len({c.tobytes() for c in out["codes"][:8]}) > 1
    read = n * info["grid_rows"] * info["grid_cols"] * a.cell * a.cell * 8
    res["encode_bytes_read"] = int(read)
    res["encode_gbs"] = round(read / (res["encode_ms"] * 1e-3) / 1e9, 1)
    # a filled database: the eight codes with random nibbles changed, under 64 tags
    rng = np.random.default_rng(1)
    codes = out["codes"][rng.integers(0, 8, a.slots)].copy()
    flip = rng.integers(0, a.ferns, (a.slots, 6))
    for k in range(6):
        codes[np.arange(a.slots), flip[:, k] // 8] ^= (np.uint32(1) << (4 * (flip[:, k] % 8)).astype(np.uint32))
    db.set(codes, np.tile(np.eye(4, dtype=np.float32), (a.slots, 1, 1)), np.arange(a.slots) % 64, np.arange(a.slots))

    def query():
        out["matches"] = db.query_streams(streams, None, 4)

    res["query_ms"] = median_ms(s, query)
    copy.append(s.microbench_copy(256 << 20, 10))
    res["query_code_bytes"] = int(n * a.slots * info["words"] * 4)
    res["query_gbs"] = round(res["query_code_bytes"] / (res["query_ms"] * 1e-3) / 1e9, 1)
    res["query_minus_encode_ms"] = round(res["query_ms"] - res["encode_ms"], 3)  # (a query of streams encodes them first)
    res["copy_gbs"] = [round(c, 1) for c in copy]
    res["encode_fraction_of_copy"] = round(res["encode_gbs"] / float(np.median(copy)), 3)
    assert (out["matches"]["distance"][:, 0] <= 6).all()
    print("%d streams %dx%d, cell %d, %d ferns (%d words); device copy %s GB/s" % (n, cols, rows, a.cell, a.ferns, info["words"], res["copy_gbs"]))
    print("sfk_encode_streams: %.3f ms, %.2f GB read = %.0f GB/s = %.2f of the copy rate" % (res["encode_ms"], read / 1e9, res["encode_gbs"], res["encode_fraction_of_copy"]))
    print("sfk_query_streams (m = 4) against %d slots: %.3f ms (%.3f ms beyond the encode), %.2f GB of codes = %.0f GB/s"
          % (a.slots, res["query_ms"], res["query_minus_encode_ms"], res["query_code_bytes"] / 1e9, res["query_gbs"]))
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
