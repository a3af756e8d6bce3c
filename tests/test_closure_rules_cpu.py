"""The PER SAMPLE rule of the closure constraints (staticfusion_amd/csrc/sf_closure_rules.h), checks that need no GPU. The
pure-host call sfc_link_sample agrees with tests/closure_ref.py bit for bit (np.array_equal) over the table of
tests/closure_cases.py: each absence, dz exactly on the gate and one ulp beyond it from both sides, gate_abs 0 and +inf (with the
clip of the sum at 32 m), min_time_gap on the boundary, just inside it and -inf, NaN and inf times and positions (dropped, the
pin kept), a dst that overflows, every pins mode. And a stand-alone C++ program includes the real header -- the text the kernel
compiles -- and replays the same table under the address and undefined-behaviour sanitizers, with guard words behind its outputs
(a child process: nothing is loaded into python)."""
import functools
import os
import re
import struct
import subprocess

import numpy as np

import closure_cases as cc
import closure_ref as cr
import view_ref
from conftest import ROOT

F = np.float32


def column_major(pose):
    return np.ascontiguousarray(np.asarray(pose, F).T.ravel())


@functools.lru_cache(maxsize=None)
def expected():
    """[(row of the table, mask, records, q_dz, q_shift)] by the restatement, computed once"""
    out = []
    zero = np.zeros(12, F)
    for row in cc.rule_table():
        name, sa, so, zA, zO, pose_from, pose_to, p = row
        T, P = view_ref.invert_pose(column_major(pose_from)), column_major(pose_to)
        mask, links, pins, q_dz, q_shift = cr.link_samples([sa is not None], zero if sa is None else sa, [so is not None], zero if so is None else so, [zA], [zO], T, P, p)
        recs = cr.ordered(mask, links, pins)
        m1, r1 = cr.link_sample(sa, so, zA, zO, T, P, p)
        assert m1 == int(mask[0]) and cr.same_records(r1, recs)
        out.append((row, int(mask[0]), recs, int(q_dz[0]), int(q_shift[0]), T, P))
    return out


def test_the_table_covers_what_it_is_for():
    seen = {}
    for (name, sa, so, zA, zO, _, _, p), mask, recs, q_dz, q_shift, _, _ in expected():
        seen[(name, p.pins)] = (mask, recs.shape[0], q_dz, q_shift)
        assert recs.shape[0] == bool(mask & cr.LINK) + bool(mask & cr.PIN)
        assert np.all(np.isfinite(recs["src"])) and np.all(np.isfinite(recs["dst"])) and np.all(np.isfinite(recs["time"]))
    L, P_, A_, N_, B_ = cr.LINK, cr.PIN, cr.APART, cr.NEAR, cr.BOTH
    assert seen[("plain", 0)][0] == B_ | N_ | A_ | L and seen[("plain", 1)][0] == seen[("plain", 2)][0] == B_ | N_ | A_ | L | P_
    assert seen[("no a", 1)][0] == 0 and seen[("no a", 2)][0] == P_ and seen[("no o", 2)][0] == 0 and seen[("neither", 2)][0] == 0
    for pins in (0, 1, 2):
        assert seen[("on the gate", pins)][0] & N_ and not seen[("one ulp beyond", pins)][0] & N_  # dz <= gate, exactly
        assert seen[("on the gate from below", pins)][0] & N_ and not seen[("one ulp beyond from below", pins)][0] & N_
        assert seen[("on the gate", pins)][2] == 4096  # 0.25 m in 1/16384 m
        assert seen[("gate 0 equal", pins)][0] & N_ and not seen[("gate 0 apart", pins)][0] & N_
        assert seen[("gate inf", pins)][0] & N_ and seen[("gate inf", pins)][2] == 17 * 16384
        assert seen[("gate inf, clip", pins)][2] == 32 * 16384  # dz = 38.5, clipped
        assert seen[("gap on the boundary", pins)][0] & N_ and not seen[("gap on the boundary", pins)][0] & A_  # 12 - 3 > 9 is false
        assert seen[("gap just inside", pins)][0] & A_ and seen[("gap -inf", pins)][0] & A_ and not seen[("gap negative", pins)][0] & A_
        assert not seen[("a time NaN", pins)][0] & A_  # a comparison with a NaN operand is false: no link is made, none dropped
        assert seen[("a time inf", pins)][0] & cr.LINK_DROPPED and not seen[("a time inf", pins)][0] & L
        assert not seen[("both times inf", pins)][0] & A_  # inf - inf is NaN
        assert seen[("o time -inf", pins)][0] & A_ and seen[("o time -inf", pins)][0] & L
    assert seen[("a time inf", 1)][0] & P_ and seen[("a time inf", 1)][1] == 1  # the dropped link does not take its pin with it
    assert seen[("o time NaN", 2)][0] & cr.PIN_DROPPED and not seen[("o time NaN", 1)][0] & (P_ | cr.PIN_DROPPED)
    assert seen[("o time -inf", 1)][0] & cr.PIN_DROPPED and seen[("o time -inf", 1)][1] == 1
    assert seen[("a position NaN", 1)][0] & cr.LINK_DROPPED and seen[("a position NaN", 1)][0] & P_
    assert seen[("a position inf", 2)][0] & cr.LINK_DROPPED and seen[("o position inf", 2)][0] & cr.PIN_DROPPED and seen[("o position NaN", 1)][0] & cr.PIN_DROPPED
    assert seen[("dst overflows", 1)][0] & cr.LINK_DROPPED and seen[("dst overflows", 1)][0] & P_
    assert seen[("plain", 1)][3] > 0  # a link that is written has a shift


def test_the_pure_host_call_equals_the_restatement():
    from staticfusion_amd import closure

    for (name, sa, so, zA, zO, pose_from, pose_to, p), mask, recs, _, _, _, _ in expected():
        got_mask, got = closure.link_sample(sa, so, zA, zO, pose_from, pose_to, cc.as_product(p))
        assert got_mask == mask, (name, p.pins, got_mask, mask)
        assert got.dtype == closure.RECORD and cr.same_records(got, recs), (name, p.pins)
        if mask & cr.PIN:
            assert np.array_equal(got[-1]["src"], so[0:3]) and np.array_equal(got[-1]["dst"], so[0:3]) and got[-1]["weight"] == F(p.w_pin)
        if mask & cr.LINK:
            assert np.array_equal(got[0]["src"], sa[0:3]) and got[0]["time"] == sa[6] and got[0]["weight"] == F(p.w_link)


def test_the_rule_on_the_host_under_the_sanitizers(tmp_path):
    path = str(tmp_path / "table.bin")
    raw = lambda a, t: np.ascontiguousarray(a, t).tobytes()  # noqa: E731
    rows = expected()
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(rows)))
        zero = np.zeros(12, F)
        for (name, sa, so, zA, zO, _, _, p), mask, recs, q_dz, q_shift, T, P in rows:
            f.write(struct.pack("<3i", sa is not None, so is not None, p.pins))
            f.write(struct.pack("<7f", zA, zO, p.gate_abs, p.gate_rel, p.min_time_gap, p.w_link, p.w_pin))
            f.write(raw(zero if sa is None else sa, F)[:32] + raw(zero if so is None else so, F)[:32] + raw(T, F) + raw(P, F))
            f.write(struct.pack("<i2qi", mask, q_dz, q_shift, recs.shape[0]) + recs.tobytes())
        for extent, stride in ((1, 1), (1, 2), (65, 1), (64, 7), (48, 7), (4096, 4096), (4096, 4095), (2048, 4096), (2049, 4096), (37, 3)):
            f.write(struct.pack("<3i", extent, stride, len(cr.sample_positions(extent, stride))))
    exe = str(tmp_path / "closure_rules_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "closure_rules_host.cpp"), "-o", exe])
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode())
    m = re.match(r"ok (\d+)\n", r.stdout.decode())
    assert m and int(m.group(1)) >= 5 * len(rows) + 10 and not r.stderr
