"""The IRLS streaming passes in isolation (sf_irls_pass_kernel): achieved GB/s per pass and ablations."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse
os.environ.setdefault("SF_VARIANT", "throughput")  # the 256-thread build the numbers in DESIGN.md §5.1 refer to (a batch of 512 would select the other)
import staticfusion_amd as sf
from staticfusion_amd.synth import make_batch
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--workload", default="static")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--slices", type=int, default=1, help="workgroups per stream (experiment: records resident in the Infinity Cache)")
ap.add_argument("--serpentine", action="store_true", help="pass 1 then pass 2 back to back over the same records, pass 2 upwards against "
                "pass 2 back down from where pass 1 ended (the solver's order), at levels 0 and 1; alternating, --rounds times")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--window-px", default=None, help="with --serpentine: comma-separated load-policy windows of the sweeps in pixels (sf_irls.h: "
                "pass_division; 0 = every record nt), each timed against the all-default policy, alternating; 'rule' = the window the host derives")
a = ap.parse_args()
api = sf.load()
p = bench.make_params(api, a.workload)
pairs = make_batch(8, sphere=(a.workload == "sphere"), distinct=8)
s = sf.Solver(api, 240, 320, a.batch, p)
for b in range(a.batch):
    s.set_current(b, *pairs[b % 8]["new"]); s.set_prediction(b, *pairs[b % 8]["old"])
s.process_frame(0); s.synchronize()
npx = 240 * 320
if a.serpentine and not a.window_px:
    # which 3 = both passes upwards, 4 = pass 2 back down; | (L << 4): level L's pixel count and geometry (sf.h: sf_microbench_pass)
    bpp = 29.0 if p.segmentation_enabled else 28.0
    for L in (0, 1):
        px = 2 * a.batch * a.reps * (npx >> (2 * L))  # two passes per repetition
        for which in (3, 4):
            s.microbench_pass(which | (L << 4), a.slices << 8, 2)
        ms = {3: [], 4: []}
        for r in range(a.rounds):
            for which in ((3, 4) if r % 2 == 0 else (4, 3)):  # alternate who goes first
                ms[which].append(s.microbench_pass(which | (L << 4), a.slices << 8, a.reps))
        for which, name in ((3, "forward "), (4, "serpentine")):
            v = ms[which]
            print("level %d %-10s pass 1 + pass 2 x %d: ms per launch %s  mean %.3f  streamed(%d B/px) %7.1f GB/s" % (
                L, name, a.reps, " ".join("%.3f" % x for x in v), sum(v) / len(v), bpp, bpp * px / (sum(v) / len(v)) / 1e6))
        ratios = [y / x for x, y in zip(ms[3], ms[4])]
        print("level %d serpentine / forward time: mean %.4f  per round: %s" % (L, sum(ms[4]) / sum(ms[3]), " ".join("%.4f" % x for x in ratios)))
def _timed(which, reps, policy=None, window=None):
    """one launch of the isolated passes with the load policy given through the per-launch environment hooks (include/sf.h)"""
    for k, v in (("SF_PASS_POLICY", policy), ("SF_PASS_WINDOW_PX", window)):
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = str(v)
    try:
        return s.microbench_pass(which, a.slices << 8, reps)
    finally:
        os.environ.pop("SF_PASS_POLICY", None); os.environ.pop("SF_PASS_WINDOW_PX", None)
if a.serpentine and a.window_px:
    # the serpentine pair (which 4) under each window against the all-default policy, at levels 0 and 1
    print("resident workgroups of a frame launch: %d per CU, %d in all; batch %d" % (s.resident_workgroups() + (a.batch,)))
    for L in (0, 1):
        for w in a.window_px.split(","):
            win = None if w == "rule" else int(w)
            _timed(4 | (L << 4), 2, "default"); _timed(4 | (L << 4), 2, None, win)
            ms = {0: [], 1: []}
            for r in range(a.rounds):
                for nt in ((0, 1) if r % 2 == 0 else (1, 0)):
                    ms[nt].append(_timed(4 | (L << 4), a.reps, None if nt else "default", win if nt else None))
            print("level %d window %8s px (%6.1f KB): ms per launch default %s | windowed %s | windowed / default mean %.4f per round %s" % (
                L, w, (win or 0) * 28 / 1024.0, " ".join("%.3f" % x for x in ms[0]), " ".join("%.3f" % x for x in ms[1]),
                sum(ms[1]) / sum(ms[0]), " ".join("%.4f" % (y / x) for x, y in zip(ms[0], ms[1]))))
for which in (() if a.serpentine else (1, 2)):
    for variant, name in ((0, "product"), (1, "loads only"), (2, "no accumulation")):
        s.microbench_pass(which, variant | (a.slices << 8), 2)
        ms = s.microbench_pass(which, variant | (a.slices << 8), a.reps)
        px = a.batch * a.reps * npx
        bpp = 29.0 if p.segmentation_enabled else 28.0  # 7 float planes (+ 1 label byte with segmentation)
        print("pass %d %-16s %8.3f ms  %6.2f Gpx/s  streamed(%d B/px) %7.1f GB/s  algorithmic(30 B/px/pass) %7.1f GB/s" % (
            which, name, ms, px / ms / 1e6, bpp, bpp * px / ms / 1e6, 30.0 * px / ms / 1e6))
import ctypes as C
t = (C.c_int64 * 32)()
api.check(api.get_stage_profile(s.h, t))
if t[23] > 0:
    print("shader clock during the last pass launch: %.0f MHz (s_memtime ticks %d / 100 MHz ticks %d)" % (100.0 * t[22] / t[23], t[22], t[23]))
