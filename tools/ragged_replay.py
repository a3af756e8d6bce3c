#!/usr/bin/env python3
"""What compaction buys a ragged batch (include/sf_migrate.h).

N sequences of different lengths (drawn once from a seeded uniform range) are replayed from HBM pools through
sf_process_sequence_frames_device, K frames per launch, twice:

  (a) today's loop: one handle of N streams; a stream whose sequence has ended gets frame_index = -1 and is solved again and
      again until the longest sequence ends;
  (b) after every chunk the live streams are compacted into a handle of the next smaller size that holds them
      (sfm_copy_streams; the ladder N, N/2, N/4, ... is created before the clock starts).

One JSON line: useful stream-frames per second of both loops, the time spent in the copies, the copy's achieved bytes per
second beside sf_microbench_copy of the same byte count in the same run, and the shader clock both loops got. Both loops run
the throughput build, so the streams that live to the end must agree bit for bit (`identical`).

    python tools/ragged_replay.py --streams 2048 --min-len 40 --max-len 200 --chunk 20
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import staticfusion_amd as sf  # noqa: E402
from staticfusion_amd import streams  # noqa: E402
from staticfusion_amd.synth import make_sequence  # noqa: E402


def device_pools(seqs):
    """[pool frame][cols][rows] depth and intensity pools in HBM (the HIP runtime of the product library)"""
    hiprt = ctypes.CDLL(sf.LIB)
    col = lambda x: np.ascontiguousarray(np.asarray(x, np.float32).T).ravel()
    ptrs = []
    for ch in (0, 1):
        h = np.stack([col(f[ch]) for sq in seqs for f in sq["frames"]])
        ptr = ctypes.c_void_p()
        assert hiprt.hipMalloc(ctypes.byref(ptr), ctypes.c_size_t(h.nbytes)) == 0
        assert hiprt.hipMemcpy(ptr, h.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(h.nbytes), 1) == 0
        ptrs.append(ptr)
    return hiprt, ptrs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--min-len", type=int, default=40)
    ap.add_argument("--max-len", type=int, default=200)
    ap.add_argument("--chunk", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--rows", type=int, default=240)
    ap.add_argument("--cols", type=int, default=320)
    ap.add_argument("--min-handle", type=int, default=64, help="smallest handle of the ladder")
    a = ap.parse_args()
    N, K, D, F = a.streams, a.chunk, 2, 16
    api = sf.load().with_variant("throughput")
    p = api.default_params_struct()
    p.kb = 1.05
    seqs = [make_sequence(1000 + q, F, sphere=True, out_rows=a.rows, out_cols=a.cols) for q in range(D)]
    hiprt, pools = device_pools(seqs)
    pd, pi = pools[0].value, pools[1].value
    rng = np.random.RandomState(a.seed)
    length = rng.randint(a.min_len, a.max_len + 1, size=N)  # frames of sequence b, frame 0 included
    phase = (np.arange(N) // D * 3) % F
    which = np.arange(N) % D

    def pool_frame(b, t):
        """frame t of sequence b: its pool sequence played forwards and backwards (the motion stays continuous), or -1 past its end"""
        t = np.asarray(t)
        x = (phase[b] + t) % (2 * F - 2)
        tri = np.where(x < F, x, 2 * F - 2 - x)
        return np.where(t < length[b], which[b] * F + tri, -1).astype(np.int32)

    t_end = int(length.max())
    useful = int((length - 1).sum())  # frame 0 only fills the ring
    all_b = np.arange(N)
    last = np.flatnonzero(length == t_end)[:8]  # streams that live to the end: compared between the loops

    def clock(handles, before=None):
        c = [h.shader_clock_counters() for h in handles]
        now = (sum(x[0] for x in c), sum(x[1] for x in c))
        return now if before is None else sf.Solver.shader_clock_mhz(before, now)

    # ---- (a) one handle, ended streams solved again
    H = sf.Solver(api, a.rows, a.cols, N, p)
    H.advance_sequences_device(pd, pi, pool_frame(all_b, 0), D * F)
    H.push_history(0)
    H.synchronize()
    c0 = clock([H])
    t0 = time.perf_counter()
    t = 1
    while t < t_end:
        k = min(K, t_end - t)
        idx = np.stack([pool_frame(all_b, t + q) for q in range(k)])
        H.process_sequence_frames_device(pd, pi, idx, D * F, t)
        t += k
    H.synchronize()
    sec_a = time.perf_counter() - t0
    mhz_a = clock([H], c0)
    T_a = [H.T(int(b)) for b in last]
    launches_a = (t_end - 1 + K - 1) // K
    H.close()

    # ---- (b) compaction after every chunk
    sizes = [N]
    while sizes[-1] // 2 >= a.min_handle:
        sizes.append(sizes[-1] // 2)
    ladder = [sf.Solver(api, a.rows, a.cols, n, p) for n in sizes]
    cur, live = 0, all_b.copy()  # live[slot] = sequence in that slot of the current handle
    ladder[0].advance_sequences_device(pd, pi, pool_frame(all_b, 0), D * F)
    ladder[0].push_history(0)
    for h in ladder[1:]:  # slots nothing is ever copied into hold a still scene with a full ring: solved like any ended stream
        for _ in range(2):
            h.advance_sequences_device(pd, pi, pool_frame(all_b[: h.batch_size], 0), D * F)
        for c in range(5):
            h.push_history(c)
    for h in ladder:
        h.synchronize()
    c0 = clock(ladder)
    copies, copy_sec, copy_bytes, solved = 0, 0.0, 0, 0
    per_stream = streams.blob_bytes(a.rows, a.cols, ladder[0].levels, 0) - 64
    t0 = time.perf_counter()
    t = 1
    while t < t_end:
        k = min(K, t_end - t)
        h = ladder[cur]
        idx = np.full((k, h.batch_size), -1, np.int32)
        for q in range(k):
            idx[q, : len(live)] = pool_frame(live, t + q)
        h.process_sequence_frames_device(pd, pi, idx, D * F, t)
        solved += k * h.batch_size
        t += k
        keep = np.flatnonzero(length[live] > t)
        nxt = cur
        while nxt + 1 < len(sizes) and sizes[nxt + 1] >= len(keep):
            nxt += 1
        if nxt != cur and len(keep):
            h.synchronize()
            c = time.perf_counter()
            streams.copy_streams(ladder[nxt], np.arange(len(keep)), t, h, keep, t)
            ladder[nxt].synchronize()
            copy_sec += time.perf_counter() - c
            copies += 1
            copy_bytes += per_stream * len(keep)
            live, cur = live[keep], nxt
    ladder[cur].synchronize()
    sec_b = time.perf_counter() - t0
    mhz_b = clock(ladder, c0)
    slot_of = {int(b): q for q, b in enumerate(live)}
    T_b = [ladder[cur].T(slot_of[int(b)]) for b in last]
    # the same bytes through the plain streaming kernel, now (same clocks, same box)
    one_copy = max(4096, (copy_bytes // max(copies, 1)) // 16 * 16)
    plain_gbs = ladder[0].microbench_copy(one_copy, 5)
    for h in ladder:
        h.close()
    for ptr in pools:
        hiprt.hipFree(ptr)
    print(json.dumps({
        "tool": "ragged_replay", "streams": N, "rows": a.rows, "cols": a.cols, "lengths": [a.min_len, a.max_len], "seed": a.seed,
        "chunk_frames": K, "longest": t_end, "useful_stream_frames": useful, "build": "throughput",
        "resolve_ended": {"seconds": round(sec_a, 4), "useful_stream_frames_per_s": round(useful / sec_a, 1), "solved_stream_frames": int(N * (t_end - 1)),
                          "launches": launches_a, "shader_clock_mhz": round(mhz_a, 1)},
        "compacted": {"seconds": round(sec_b, 4), "useful_stream_frames_per_s": round(useful / sec_b, 1), "solved_stream_frames": int(solved),
                      "ladder": sizes, "copies": copies, "copy_seconds": round(copy_sec, 5), "copied_streams_bytes": int(copy_bytes),
                      "copy_gb_per_s": round(2.0 * copy_bytes / copy_sec / 1e9, 2) if copy_sec else None,
                      "microbench_copy_gb_per_s": round(plain_gbs, 2), "microbench_copy_bytes": int(one_copy),
                      "shader_clock_mhz": round(mhz_b, 1)},
        "speedup": round(sec_a / sec_b, 3),
        "identical": bool(all(np.array_equal(x, y) for x, y in zip(T_a, T_b))),
        "note": "copy_seconds is host time around synchronised copies (launch latency included); copy_gb_per_s and microbench_copy_gb_per_s both count bytes read + written",
    }))


if __name__ == "__main__":
    main()
