"""The rules OBSERVE and DECIDE of the carve (staticfusion_amd/csrc/sf_carve_rules.h), checks that need no GPU. The pure-host
calls sfe_observe and sfe_decide agree with tests/carve_ref.py exactly, in class and in the three counts, over the table of
tests/carve_cases.py: r exactly on the tolerance and one ulp beyond it from both sides; a frame depth of 0, negative, NaN, inf,
exactly z_max and one ulp above it; a denominator of 0, negative and tiny; the projection exactly on 0 and on cols / rows; the
window clipped at each border and corner; windows 0 and 3 with min_pixels 1 and 49; min_cos on its boundary, a back-facing, a
zero and a NaN normal; each of the four culls; a negative fy; min_votes and max_support on their boundaries. The same table is
replayed by a stand-alone program that includes the real header, built with the address and undefined-behaviour sanitizers,
with guard words behind its outputs (a child process: nothing is loaded into python under a sanitizer)."""
import os
import re
import struct
import subprocess

import numpy as np

import carve_cases as cc
import carve_ref as cr
import view_ref
from conftest import ROOT

F = np.float32
_EXPECTED = []


def expected():
    """[(case, class, found)] from the restatement, computed once"""
    if not _EXPECTED:
        for case in cc.observe_cases():
            name, s, tick, v, img, p = case
            cls, found = cr.observe(s[None, :], tick, v, img, p)
            _EXPECTED.append((case, int(cls[0]), tuple(int(x) for x in found[0])))
    return _EXPECTED


def test_the_table_reaches_what_it_is_meant_to_reach():
    """conditions on the restatement alone: the boundary cases fall on the side the header's comparisons give them"""
    seen = {case[0]: (cls, found) for case, cls, found in expected()}
    assert len(seen) == len(expected())  # the names are distinct
    U, T, S, O = cr.UNSEEN, cr.THROUGH, cr.SUPPORTED, cr.OCCLUDED
    assert seen["r on +tol"] == (S, (0, 1, 0)) and seen["r one ulp beyond +tol"] == (T, (1, 0, 0))
    assert seen["r on -tol"] == (S, (0, 1, 0)) and seen["r one ulp beyond -tol"] == (O, (0, 0, 1))
    for k in ("z zero", "z negative", "z NaN", "z inf", "z one ulp above z_max"):
        assert seen[k] == (U, (0, 0, 0)), k
    assert seen["z on z_max"] == (T, (1, 0, 0))
    # zp = 1 / lx: of the seven columns of the window those with lx <= 0 are invalid, the five others see a frame at 5 m behind them
    assert seen["den zero and negative"] == (T, (5 * 6, 0, 0)) and seen["den zero and negative, frame in front"] == (S, (0, 2 * 6, 3 * 6))
    assert seen["zp below 0.4"][1] == (2 * 6, 0, 0)  # zp = 1 and 0.5; 1/3 and 1/4 lie below 0.4
    assert seen["den tiny positive"][1][0] == seen["den tiny negative"][1][0] == 5 * 6
    assert seen["qx exactly 0"][0] == T and seen["qy exactly 0"][0] == T and seen["qx just below cols"][0] == T
    assert seen["qx exactly cols"][0] == U and seen["qy exactly rows"][0] == U and seen["qx negative"][0] == U
    assert seen["window 3, 49 pixels through"] == (T, (49, 0, 0)) and seen["window 3, 48 of 49 pixels through"] == (U, (48, 0, 0))
    assert seen["window 3, 47 through and one in front"] == (O, (47, 0, 1)) and seen["window 3, min_pixels 1"][0] == T
    assert seen["window 0, min_pixels 1, in front"] == (O, (0, 0, 1))
    sizes = {w: [sum(seen["window %d at pixel (%d, %d)" % (w, i, j)][1]) for i, j in ((0, 0), (3, 2))] for w in (1, 3)}
    assert sizes[1][0] <= 4 and sizes[1][1] <= 9 and sizes[3][0] <= 16 and sizes[3][1] <= 42  # clipped windows hold fewer pixels
    assert seen["min_cos 1 on the axis"][0] == T and seen["min_cos 1, a short normal"][0] == T and seen["min_cos 1, off the axis"][0] == U
    assert seen["min_cos just below"][0] == T and seen["min_cos just above"][0] == U and seen["min_cos 0"][0] == T
    for k in ("a back-facing normal", "a normal at a right angle, min_cos 0", "a zero normal", "a NaN normal", "an inf normal", "a NaN position"):
        assert seen[k] == (U, (0, 0, 0)), k
    for k in ("beyond max_depth", "nearer than 0.4", "below min_confidence", "too old", "a NaN time with the age test on"):
        assert seen[k] == (U, (0, 0, 0)), k
    for k in ("on max_depth", "on 0.4", "on min_confidence", "a NaN confidence", "just young enough", "a NaN time with the age test off"):
        assert seen[k][0] == T, k
    assert {seen["negative fy %d" % k][0] for k in range(4)} - {U} and len({seen["under a pose %d" % k][0] for k in range(40)}) == 4
    want = [vt >= mv and vs <= ms for vt, vs, mv, ms in cc.DECIDE_CASES]
    assert [bool(cr.decide(vt, vs, cc.params(min_votes=mv, max_support=ms))) for vt, vs, mv, ms in cc.DECIDE_CASES] == want and 4 < sum(want) < 12


def test_the_pure_host_calls_equal_the_restatement():
    from staticfusion_amd import carve

    for (name, s, tick, v, img, p), cls, found in expected():
        got = carve.observe(s, tick, cc.as_product_view(v), img, cc.as_product(p))
        assert got == (cls, found), (name, got, cls, found)
    for vt, vs, mv, ms in cc.DECIDE_CASES:
        p = cc.params(min_votes=mv, max_support=ms)
        assert carve.decide(vt, vs, cc.as_product(p)) == bool(cr.decide(vt, vs, p)), (vt, vs, mv, ms)


def test_the_rules_on_the_host_under_the_sanitizers(tmp_path):
    path = str(tmp_path / "table.bin")
    raw = lambda a, t: np.ascontiguousarray(a, t).tobytes()  # noqa: E731
    rows = expected()
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(rows)))
        for (name, s, tick, v, img, p), cls, found in rows:
            f.write(raw(s, F) + raw(view_ref.invert_pose(v.pose[:]), F))
            f.write(struct.pack("<8f", v.cx, v.cy, v.fx, v.fy, v.max_depth, v.min_confidence, float(tick), float(v.max_age)))
            f.write(struct.pack("<3i", v.max_age >= 0, v.rows, v.cols))
            f.write(struct.pack("<4f4i", p.tol_abs, p.tol_rel, p.z_max, p.min_cos, p.window, p.min_pixels, p.min_votes, p.max_support))
            f.write(raw(np.asarray(img, F).T, F))  # column-major: (v, u) at v + u * rows
            f.write(struct.pack("<4i", cls, *found))
        f.write(struct.pack("<i", len(cc.DECIDE_CASES)))
        for vt, vs, mv, ms in cc.DECIDE_CASES:
            f.write(struct.pack("<5i", vt, vs, mv, ms, bool(cr.decide(vt, vs, cc.params(min_votes=mv, max_support=ms)))))
    exe = str(tmp_path / "carve_rules_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "carve_rules_host.cpp"), "-o", exe])
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode())
    m = re.match(r"ok (\d+)\n", r.stdout.decode())
    assert m and int(m.group(1)) >= 3 * len(rows) + len(cc.DECIDE_CASES) and not r.stderr
