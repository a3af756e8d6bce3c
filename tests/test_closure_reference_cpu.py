"""The restatement of the closure constraints (tests/closure_ref.py) against answers written out by hand, no GPU: a 4 x 4 view at
stride 2 over three surfels, whose four samples, records and counts are stated below; the sum that needs more than 32 bits; the
scenes of tests/closure_cases.py do what the GPU tests use them for; and the doubled wall, whose pose difference is a pure
translation, so that every link's dst - src equals that translation to within a bound computed from the magnitudes."""
import numpy as np

import closure_cases as cc
import closure_ref as cr
import view_ref
from staticfusion_amd import view

F = np.float32


def flat(x, y, z, r, t_init, t_last=1.0):
    """a surfel facing a camera at the origin"""
    s = np.zeros(12, F)
    s[0:3], s[3], s[4], s[5], s[6], s[7], s[10], s[11] = (x, y, z), 1.0, 0x102030, 1.0, t_init, t_last, -1.0, r
    return s


def test_a_four_by_four_view_at_stride_two_by_hand():
    """fx = fy = 2, cx = cy = 2: pixel (x, y) looks along ((x + 0.5 - 2) / 2, (y + 0.5 - 2) / 2, 1). Stride 2 samples x, y in {1, 3}
    in the order (1,1), (3,1), (1,3), (3,3); the rays of x = 1 and x = 3 meet the plane z = 2 at x = -0.5 and x = +1.5.
    view_from is the identity; view_to is the identity but for its translation (0, 0, 0.25). The NEW map holds
      N0 at (-0.5, -0.5, 2), radius 0.3, init time 10: drawn at sample (1,1) only
      N1 at ( 1.5, -0.5, 2), radius 0.3, init time  1: drawn at sample (3,1) only
    and the OLD map, seen from a camera 0.25 nearer the wall (pose z = 0.25),
      O0 at (-0.4375, -0.4375, 2), radius 0.3, init time 2: from z = 0.25 its ray (x=1,y=1) meets z' = 1.75 at (-0.4375, -0.4375): drawn at (1,1)
      O1 at (-0.4375,  1.3125, 2), radius 0.3, init time 3: drawn at sample (1,3)
    Sample (1,1): both, dz = |2 - 1.75| = 0.25 <= 0.3, gap 10 - 2 > 0: LINK N0 -> N0 + (0, 0, 0.25), and its PIN O0.
    Sample (3,1): new only. Sample (1,3): old only. Sample (3,3): nothing."""
    eye = np.eye(4, dtype=F)
    nearer = eye.copy()
    nearer[2, 3] = 0.25
    vf = view.View(eye, 2.0, 2.0, 2.0, 2.0, 4, 4, min_confidence=0.0)
    vt = view.View(nearer, 2.0, 2.0, 2.0, 2.0, 4, 4, min_confidence=0.0)
    new = np.stack([flat(-0.5, -0.5, 2.0, 0.3, 10.0), flat(1.5, -0.5, 2.0, 0.3, 1.0)])
    old = np.stack([flat(-0.4375, -0.4375, 2.0, 0.3, 2.0), flat(-0.4375, 1.3125, 2.0, 0.3, 3.0)])
    A, O = view_ref.render(new, vf), view_ref.render(old, vt)
    assert [int(A["index"][y, x]) for y, x in ((1, 1), (1, 3), (3, 1), (3, 3))] == [0, 1, -1, -1]
    assert [int(O["index"][y, x]) for y, x in ((1, 1), (1, 3), (3, 1), (3, 3))] == [0, -1, 1, -1]
    assert A["depth"][1, 1] == F(2.0) and O["depth"][1, 1] == F(1.75)
    for pins, n_pins in ((0, 0), (1, 1), (2, 2)):
        p = cc.params(stride=2, pins=pins, gate_abs=0.3, gate_rel=0.0, w_link=3.0, w_pin=0.5)
        recs, c = cr.build_entry(new, 1, old, 1, vf, vt, p, first=7)
        assert c == dict(n_samples=4, n_new=2, n_old=2, n_both=1, n_near=1, n_apart=1, n_links=1, n_pins=n_pins, n_dropped=0, first=7,
                         sum_dz=4096, sum_shift=4096), (pins, c)  # 0.25 m * 16384, twice
        assert recs.shape[0] == 1 + n_pins
        assert recs[0]["src"].tolist() == [-0.5, -0.5, 2.0] and recs[0]["dst"].tolist() == [-0.5, -0.5, 2.25] and recs[0]["time"] == 10 and recs[0]["weight"] == 3
        if pins:
            assert recs[1]["src"].tolist() == recs[1]["dst"].tolist() == [-0.4375, -0.4375, 2.0] and recs[1]["time"] == 2 and recs[1]["weight"] == 0.5
        if pins == 2:  # the pin of sample (1,3), where only the old part is drawn, comes last: sample order
            assert recs[2]["src"].tolist() == [-0.4375, 1.3125, 2.0] and recs[2]["time"] == 3
    # the gate one step tighter than dz, and the time gap on the boundary
    _, c = cr.build_entry(new, 1, old, 1, vf, vt, cc.params(stride=2, gate_abs=0.2499, gate_rel=0.0))
    assert (c["n_both"], c["n_near"], c["n_links"], c["sum_dz"]) == (1, 0, 0, 0)
    _, c = cr.build_entry(new, 1, old, 1, vf, vt, cc.params(stride=2, gate_abs=0.25, gate_rel=0.0, min_time_gap=8.0))
    assert (c["n_near"], c["n_apart"], c["n_links"], c["n_pins"], c["sum_dz"], c["sum_shift"]) == (1, 0, 0, 0, 4096, 0)
    # stride 1: sixteen samples; stride 3: s2 = 1, one sample at (1, 1); stride 4: s2 = 2, one at (2, 2); stride 8: s2 = 4, none
    assert [cr.build_entry(new, 1, old, 1, vf, vt, cc.params(stride=s))[1]["n_samples"] for s in (1, 2, 3, 4, 8, 16)] == [16, 4, 1, 1, 0, 0]
    assert cr.max_records(4, 4, 2) == 8


def test_sample_order_is_rows_outer_columns_inner():
    assert cr.sample_positions(7, 3) == [1, 4] and cr.sample_positions(1, 2) == [] and cr.sample_positions(4096, 4096) == [2048]
    mask = np.array([cr.LINK | cr.PIN, cr.PIN, 0, cr.LINK], np.int32)
    links, pins = np.zeros(4, cr.RECORD), np.zeros(4, cr.RECORD)
    links["time"], pins["time"] = [10, 11, 12, 13], [20, 21, 22, 23]
    assert cr.ordered(mask, links, pins)["time"].tolist() == [10, 20, 21, 13]


def far_planes(rows=512, cols=512):
    """two far-apart planes, each one large surfel: every sample of a rows x cols view has dz >= 32"""
    f = float(cols)
    vf = view.View(np.eye(4, dtype=F), cols / 2.0, rows / 2.0, f, f, rows, cols, min_confidence=0.0, max_depth=100.0)
    return np.stack([flat(0, 0, 1.0, 3.0, 5.0)]), np.stack([flat(0, 0, 40.0, 90.0, 1.0)]), vf


def test_a_sum_that_needs_more_than_32_bits():
    """The carry case of sum_dz on the restatement: 2^18 samples of dz = 39 m, clipped to 32 m = 2^19 units each, sum to 2^37.
    tests/test_gpu_closure.py runs the same scene on the device."""
    new, old, v = far_planes()
    recs, c = cr.build_entry(new, 1, old, 1, v, v, cc.params(stride=1, pins=0, gate_abs=np.inf, min_time_gap=100.0))
    assert c["n_samples"] == c["n_both"] == c["n_near"] == 1 << 18 and c["sum_dz"] == 1 << 37 and c["sum_dz"] > 1 << 32 and c["n_apart"] == 0 and recs.shape[0] == 0


def test_the_scenes_do_what_the_gpu_tests_use_them_for():
    counts = {k: cc.reference(k)[1] for k in ("64x48/s1/p1", "64x48/s7/p2", "16x16/s1/p2", "16x16/s2/p1", "1x65/s1/p1", "257x1/s1/p1", "1x1/s1/p1", "1x1/s2/p1",
                                              "64x48/s4096/p1", "64x48/s64/p1", "64x48/s3/p1", "age", "all", "none", "gap", "hole", "count/1025", "same/1025")}
    n = lambda k, f: counts[k][0][f]  # noqa: E731
    assert [n(k, "n_samples") for k in ("1x1/s2/p1", "64x48/s4096/p1", "1x1/s1/p1", "64x48/s64/p1", "64x48/s7/p2", "16x16/s2/p1", "1x65/s1/p1", "16x16/s1/p2",
                                        "257x1/s1/p1", "64x48/s3/p1", "64x48/s1/p1")] == [0, 0, 1, 1, 63, 64, 65, 256, 257, 336, 3072]
    c = counts["64x48/s1/p1"][0]  # the gates cut about half, the time gap about half of that, and non-finite times drop records
    assert 0.3 * c["n_both"] < c["n_near"] < 0.7 * c["n_both"] and 0.25 * c["n_near"] < c["n_apart"] < 0.75 * c["n_near"] and c["n_both"] > 1000
    assert c["n_dropped"] > 20 and c["n_links"] + c["n_dropped"] >= c["n_apart"] and c["n_pins"] > 0
    assert counts["16x16/s1/p2"][0]["n_dropped"] > 0 and counts["16x16/s1/p2"][0]["n_pins"] > counts["16x16/s1/p2"][0]["n_links"]
    c = counts["gap"][0]
    assert 0.3 * c["n_near"] < c["n_apart"] < 0.6 * c["n_near"] and c["n_near"] == c["n_both"] > 1500
    assert counts["all"][0]["n_links"] == counts["all"][0]["n_pins"] == counts["all"][0]["n_samples"] == 256  # every sample emits two records
    assert counts["none"][0]["n_links"] == counts["none"][0]["n_pins"] == 0 and counts["none"][0]["n_both"] > 100  # and none does
    # the age test of view_from keeps about a third of the new map
    (new, tick, old, _, vf, vt, p), = cc.CASES["age"]()
    kept = int((F(tick) - new[:, 7] <= F(vf.max_age)).sum())
    assert 0.25 * new.shape[0] < kept < 0.42 * new.shape[0]
    no_age = cr.build_entry(new, tick, old, tick, cc.geom_view(cc.GEOMS["64x48"], cc.POSE_FROM), vt, p)[1]
    assert 0 < counts["age"][0]["n_new"] < 0.8 * no_age["n_new"]
    # the hole: rows 16 .. 23 of the old part's drawing are empty, so the workgroups of samples 1024 .. 1535 emit no record, their neighbours do
    (new, tick, old, _, vf, vt, p), = cc.CASES["hole"]()
    o = view_ref.render(old, vt, tick=tick)["index"]
    assert np.all(o[16:24] == -1) and (o[12:16] >= 0).sum() > 50 and (o[24:28] >= 0).sum() > 50
    assert counts["hole"][0]["n_pins"] > 1000
    assert counts["same/1025"][0]["n_links"] > 500 and counts["count/1025"][0]["n_pins"] > 500


def test_the_doubled_wall_links_by_the_pose_difference():
    """view_from is a pure translation t = WALL_SHIFT and view_to the identity, so dst = (src - t') with t' the float translation
    column of inverse(view_from.pose): dst - src = -t up to rounding. The bound: |src| < 4 m and |t| < 0.07 m per coordinate;
    h.r = src.r + T[12 + r] with the three products by 0 and 1 exact, so h carries one rounding of a value below 4 (half an
    ulp: 2^-23 * 4 / 2 = 2.4e-7); dst.r = h.r + 0 exactly; dst - src is rounded once more (a value below 0.07: 3.7e-9), and
    the inverse translation differs from -t by at most half an ulp of 0.07 (3.7e-9) plus the float conversion of t (exact here:
    dyadic). Sum: below 2.5e-7 per coordinate; the test allows 3e-7."""
    whole, old, vf, vt, tick = cc.doubled_wall()
    p = cc.params(stride=2, pins=1, gate_abs=0.01, gate_rel=0.0, min_time_gap=10.0)
    recs, c = cr.build_entry(whole, tick, whole, tick, vf, vt, p)
    assert c["n_samples"] == 32 * 24 and c["n_links"] == c["n_pins"] and c["n_dropped"] == 0
    assert c["n_links"] > 0.9 * c["n_samples"]  # the two sightings overlap nearly everywhere
    links, pins = recs[0::2], recs[1::2]
    assert np.all(links["time"] >= 20) and np.all(pins["time"] <= 2) and np.array_equal(pins["src"], pins["dst"])
    d = links["dst"].astype(np.float64) - links["src"].astype(np.float64)
    assert np.abs(d + cc.WALL_SHIFT).max() <= 3e-7, np.abs(d + cc.WALL_SHIFT).max()
    assert np.abs(links["src"]).max() < 4.0
    shift_units = np.rint(np.linalg.norm(cc.WALL_SHIFT) * 16384)  # every link's shift, to within one unit of 1/16384 m
    assert abs(c["sum_shift"] - c["n_links"] * shift_units) <= c["n_links"]
    # the old part as a map of its own: the same bound
    recs2, c2 = cr.build_entry(whole, tick, old, tick, vf, vt, p)
    assert c2["n_links"] == c2["n_pins"] > 0.9 * c2["n_samples"]
    assert np.abs((recs2[0::2]["dst"].astype(np.float64) - recs2[0::2]["src"]) + cc.WALL_SHIFT).max() <= 3e-7
