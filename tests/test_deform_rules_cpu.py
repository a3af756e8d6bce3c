"""The rules of the deformation graphs (staticfusion_amd/csrc/sf_deform_rules.h), checks that need no GPU. The pure-host calls of
the library -- sfd_bind_point, sfd_deform_surfel, sfd_edges, sfd_deform_poses -- agree with tests/deform_ref.py bit for bit
(np.array_equal) on graphs of 1, 3, 4, 5 and 257 nodes: nodes on a lattice with queries on nodes, edge midpoints, face centres
and cell centres, so that (d2, j) ties occur at every rank, fourth against fifth included; duplicate nodes (dmax2 == 0); NaN
and inf positions and times; time windows that leave 0, 1 and 5 nodes eligible. And a stand-alone C++ program includes the two
real headers -- the text the kernel compiles, and the solver -- and replays the same tables and the solver cases of
tests/test_deform_solve_cpu.py under the address and undefined-behaviour sanitizers (a child process: nothing is loaded into
python)."""
import functools
import os
import re
import struct
import subprocess

import numpy as np

import deform_cases as dc
import deform_ref as dr
from conftest import ROOT

F = np.float32
SIZES = (1, 3, 4, 5, 257)
WINDOWS = (np.inf, 0.0, 1.0)


def poses_for(seed, n=6):
    rng = np.random.default_rng(seed)
    out = np.tile(np.eye(4, dtype=F), (n, 1, 1))
    for q in range(n):
        out[q, :3, :3] = dc.rotation(rng.normal(size=3), rng.uniform(0, 3)).astype(F)
        out[q, :3, 3] = rng.uniform(-0.2, 1.5, 3)
    return out, (np.arange(n) % 5).astype(F)


@functools.lru_cache(maxsize=None)
def tables():
    """[(name, G, window, pos, times, M, surfels, poses, taus, expected dict)]: computed once, shared by both tests"""
    out = []
    for G in SIZES:
        queries = dc.lattice_queries(G)
        if queries.shape[0] > 240:  # (257 nodes: a sample across the lattice, the ties are the same in every cell)
            queries = queries[::queries.shape[0] // 240]
        for name, (pos, times) in (("lattice", dc.lattice_nodes(G)), ("duplicates", dc.duplicate_nodes(G)), ("special", dc.special_nodes(G))):
            M = dc.random_affine(G, seed=G)
            surf = dc.surfels(queries.shape[0] + 30, seed=G + 1, queries=queries)
            poses, taus = poses_for(G)
            for window in WINDOWS:
                out.append(make_table(name, G, window, pos, times, M, surf, poses, taus))
    # the time window by hand: node times 0 .. 4; tau 10 leaves no node, tau 5 one, and an infinite window all five
    pos, times = dc.lattice_nodes(5)
    surf = dc.surfels(3, seed=9, queries=pos[:3] + F(0.125))
    surf[:, 6] = [10.0, 5.0, 2.0]
    poses, taus = poses_for(3)
    for window, eligible in ((1.0, [0, 1, 3]), (np.inf, [5, 5, 5])):
        assert [int((np.abs(times - t) <= F(window)).sum()) for t in surf[:, 6]] == eligible
        out.append(make_table("window", 5, window, pos, times, dc.random_affine(5, 2), surf, poses, taus))
    return out


def make_table(name, G, window, pos, times, M, surf, poses, taus):
    m, idx, w = dr.bind(pos, times, window, surf[:, 0:3], surf[:, 6])
    deformed, m2 = dr.deform(pos, times, M, window, surf)
    assert np.array_equal(m, m2)
    want = dict(m=m, idx=idx, w=w, surfels=deformed, edges=dr.edges(pos, times, window), poses=dr.deform_poses(pos, times, M, window, poses, taus))
    return (name, G, float(window), pos, times, M, surf, poses, taus, want)


def test_the_tables_cover_what_they_are_for():
    seen_m, tie45, flat, dmax0 = set(), 0, 0, 0
    for name, G, window, pos, times, M, surf, poses, taus, want in tables():
        seen_m |= set(int(x) for x in want["m"])
        with np.errstate(all="ignore"):
            d2 = ((surf[:, None, 0:3] - pos[None]) ** 2).sum(axis=2)
        srt = np.sort(np.where(np.isnan(d2), np.inf, d2), axis=1)
        if G >= 5 and window == np.inf and name == "lattice":
            tie45 += int((srt[:, 3] == srt[:, 4]).sum())
        if name == "duplicates" and G >= 5 and window == np.inf:
            dmax0 += int((srt[:, 4] == 0).sum())
        flat += int(((want["m"] > 1) & (want["w"][:, 0] == F(1) / np.maximum(want["m"], 1).astype(F))).sum())
        assert want["edges"].shape == (G, 4) and not np.any(want["edges"] == np.arange(G)[:, None])
    assert seen_m == {0, 1, 2, 3, 4} and tie45 > 20 and dmax0 > 0 and flat > 20


def test_the_pure_host_calls_equal_the_restatement():
    from staticfusion_amd import deform

    for name, G, window, pos, times, M, surf, poses, taus, want in tables():
        for q in range(surf.shape[0]):
            m, idx, w = deform.bind_point(pos, times, surf[q, 0:3], surf[q, 6], window)
            assert m == want["m"][q] and np.array_equal(idx, want["idx"][q]) and np.array_equal(w, want["w"][q]), (name, G, window, q)
            m, out = deform.deform_surfel(pos, times, M, surf[q], window)
            assert m == want["m"][q] and np.array_equal(out, want["surfels"][q]), (name, G, window, q)
            if m == 0:
                assert out.tobytes() == surf[q].tobytes()  # an unbound surfel stays bit for bit
            else:
                assert out[3:8].tobytes() == surf[q, 3:8].tobytes() and out[11] == surf[q, 11]
        assert np.array_equal(deform.edges(pos, times, window), want["edges"]), (name, G, window)
        got = deform.deform_poses(pos, times, M, poses, taus, window)
        assert np.array_equal(got, want["poses"]), (name, G, window)
        R = got[:, :3, :3].astype(np.float64)  # (what Gram-Schmidt is for: the axes are orthonormal to fp32 rounding)
        assert np.abs(np.einsum("nij,nik->njk", R, R) - np.eye(3)).max() < 1e-5


def solver_cases():
    """the cases of tests/test_deform_solve_cpu.py, as (pos, times, src, dst, con_times, weights, kwargs)"""
    import test_deform_solve_cpu as ts

    return [c[1:] for c in ts.cases()]


def test_the_rules_and_the_solver_on_the_host_under_the_sanitizers(tmp_path):
    path = str(tmp_path / "tables.bin")
    i32 = lambda *v: struct.pack("<%di" % len(v), *v)
    raw = lambda a, t: np.ascontiguousarray(a, t).tobytes()
    with open(path, "wb") as f:
        tabs = tables()
        f.write(i32(len(tabs)))
        for name, G, window, pos, times, M, surf, poses, taus, want in tabs:
            f.write(i32(G, surf.shape[0], poses.shape[0]) + struct.pack("<f", window))
            f.write(raw(pos, F) + raw(times, F) + raw(M, F) + raw(surf, F))
            f.write(raw(want["m"], np.int32) + raw(want["idx"], np.int32) + raw(want["w"], F) + raw(want["surfels"], F) + raw(want["edges"], np.int32))
            f.write(raw(np.transpose(poses, (0, 2, 1)), F) + raw(taus, F) + raw(np.transpose(want["poses"], (0, 2, 1)), F))
        cases = solver_cases()
        f.write(i32(len(cases)))
        for pos, times, src, dst, ct, wts, kw in cases:
            G, C = pos.shape[0], np.asarray(src).reshape(-1, 3).shape[0]
            p = dict(dr.SOLVE_DEFAULTS, **kw)
            M, rep = dr.solve(pos, times, src, dst, ct, wts, **kw)
            cons = np.zeros((C, 8), F)
            if C:
                cons[:, 0:3], cons[:, 3:6] = src, dst
                cons[:, 6], cons[:, 7] = ct, wts
            energy = np.zeros(33)
            energy[:rep["energy"].shape[0]] = rep["energy"]
            f.write(i32(G, C, p["iterations"]) + struct.pack("<3f", p["time_window"], p["w_reg"], p["damping"]))
            f.write(raw(pos, F) + raw(times, F) + raw(np.tile(np.eye(3, 4, dtype=F), (G, 1, 1)), F) + raw(cons, F))
            f.write(i32(rep["status"], rep["iterations_done"], rep["n_bound"]) + raw(energy, np.float64) + raw(M, F))
    exe = str(tmp_path / "deform_rules_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "deform_rules_host.cpp"), "-o", exe])
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode())
    m = re.match(r"ok (\d+)\n", r.stdout.decode())
    assert m and int(m.group(1)) > 20000 and not r.stderr
