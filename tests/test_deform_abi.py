"""Deformation graphs (include/sf_deform.h), the checks that need no GPU: the header, the ctypes table of
staticfusion_amd/deform.py and the exports of the three libraries name the same functions -- none of them part of include/sf.h,
whose version has not moved, like those of the other companions --, no other header or binding names them, the header spells no
other companion's prefix and includes sf.h only, the structs have the documented sizes, offsets and field order, the defaults are
the header's, and the pure-host parameter checks refuse every case of the header's list."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import deform_ref as dr
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "sf_deform.h")
OTHER_PREFIXES = ("sfm_", "sfw_", "sfv_", "sfs_", "sfk_", "sfr_", "sfa_", "sfj_", "sft_", "sfb_", "sfp_", "sfo_", "SF_FN")


def declared():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)  # declarations only: the comments name the functions too
    return sorted(set(re.findall(r"\b(sfd_\w+)\s*\(", txt)))


def test_header_table_and_exports_name_the_same_functions():
    import staticfusion_amd as sf
    from staticfusion_amd import align, bodies, body_maps, capi, deform, join, keyframes, map_window, regions, score, streams, tracks, view

    names = declared()
    assert len(names) == 24 and {"sfd_graph_create", "sfd_graph_destroy", "sfd_graph_info", "sfd_graph_set", "sfd_graph_get", "sfd_sample_nodes", "sfd_bind_point",
                                 "sfd_deform_surfel", "sfd_edges", "sfd_default_params", "sfd_check_params", "sfd_deform_poses", "sfd_bind_maps", "sfd_apply_maps",
                                 "sfd_solve"} <= set(names)
    assert names == sorted(deform.SIGNATURES.keys())
    for lib in ("libsf_hip.so", "libsf_hip_precise.so", "libsf_hip_reforder.so"):  # the three link the same host objects
        path = os.path.join(os.path.dirname(sf.LIB), lib)
        assert os.path.exists(path), lib
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert sorted(set(re.findall(r" T (sfd_\w+)", out))) == names, lib
        assert "sfd_bind_core" not in out and "sfd_solve_core" not in out and "orphan_graphs" not in out, "the shared text is not exported"
        # ... nor what orphans a graph now (sf_parts.h, sf_host.h), nor the graph's own hook and type
        assert not re.search(r"SfPart|shelled|orphan_all|part_destroy|check_part|check_live_handle|_ZT[VIS]\d+sfd_graph", out), lib
    # a companion of the ABI, not a part of it; no other header or binding names sfd_*, and this header and its binding name
    # none of the prefixes the other ABI tests search every header and every binding for, nor the oracle's
    for path in glob.glob(os.path.join(ROOT, "include", "*")):
        if os.path.basename(path) != "sf_deform.h":
            assert "sfd_" not in open(path).read(), path
    txt = open(HEADER).read()
    assert not any(p in txt for p in OTHER_PREFIXES)
    assert re.findall(r'#include\s+"([^"]+)"', txt) == ["sf.h"]
    binding = open(os.path.join(ROOT, "staticfusion_amd", "deform.py")).read()
    assert not any(p in binding for p in OTHER_PREFIXES)
    assert re.search(r"#define\s+SF_ABI_VERSION\s+5\b", open(os.path.join(ROOT, "include", "sf.h")).read())
    assert not any(k.startswith("sfd") or "deform" in k for k in capi.SIGNATURES)  # (the names of sf.h without "sf_")
    others = (align, bodies, body_maps, join, keyframes, map_window, regions, score, streams, tracks, view)
    for other in others:
        assert not any(k.startswith("sfd_") for k in other.SIGNATURES), other.__name__
    assert tuple(o.version() for o in others) == (1,) * 11
    assert deform.version() == 1 == deform.VERSION
    assert deform._product().api.lib is sf.load().lib and deform._product().api.lib is join._product().api.lib  # one loaded copy
    for path in glob.glob(os.path.join(ROOT, "oracle", "*")):  # the oracle's sources do not have the prefix
        if os.path.isfile(path) and not path.endswith(".so"):
            assert "sfd_" not in open(path, errors="replace").read(), path
    # the constants of the header are the binding's
    consts = dict(re.findall(r"#define\s+(SFD_\w+)\s+(\d+)", txt))
    assert (int(consts["SFD_MAX_NODES"]), int(consts["SFD_SOLVE_MAX_NODES"]), int(consts["SFD_MAX_ITERATIONS"]), int(consts["SFD_OK"]), int(consts["SFD_DEGENERATE"])) \
        == (deform.MAX_NODES, deform.SOLVE_MAX_NODES, deform.MAX_ITERATIONS, deform.OK, deform.DEGENERATE) == (1024, 256, 32, dr.OK, dr.DEGENERATE)


def test_the_oracle_binding_is_refused(ora):
    from staticfusion_amd import SfError, deform

    with pytest.raises(SfError):
        deform._bind(ora)


def test_struct_sizes_and_layouts():
    from staticfusion_amd import deform

    b = deform._product()
    assert b.params_bytes() == C.sizeof(deform.SfdParams) == 32
    assert b.counts_bytes() == C.sizeof(deform.SfdCounts) == 32
    assert b.info_bytes() == C.sizeof(deform.SfdInfo) == 16
    assert b.constraint_bytes() == C.sizeof(deform.SfdConstraint) == 32
    assert b.solve_params_bytes() == C.sizeof(deform.SfdSolveParams) == 32
    assert b.report_bytes() == C.sizeof(deform.SfdReport) == 280
    layouts = {"sfd_params": (deform.SfdParams, ("time_window", "reserved"), [0, 4]),
               "sfd_counts": (deform.SfdCounts, ("n_surfels", "n_bound", "n_unbound", "n_short", "reserved"), [0, 4, 8, 12, 16]),
               "sfd_info": (deform.SfdInfo, ("max_nodes", "n_nodes", "reserved"), [0, 4, 8]),
               "sfd_constraint": (deform.SfdConstraint, ("src", "dst", "time", "weight"), [0, 12, 24, 28]),
               "sfd_solve_params": (deform.SfdSolveParams, ("time_window", "w_reg", "damping", "iterations", "reserved"), [0, 4, 8, 12, 16]),
               "sfd_report": (deform.SfdReport, ("status", "iterations_done", "n_bound", "n_unbound", "energy"), [0, 4, 8, 12, 16])}
    txt = open(HEADER).read()
    for struct, (cls, names, offsets) in layouts.items():
        assert [getattr(cls, k).offset for k in names] == offsets, struct
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), txt, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body) == list(names) == [k for k, _ in cls._fields_], struct
    assert deform.COUNT_FIELDS == layouts["sfd_counts"][1][:-1] == dr.COUNT_FIELDS


def test_defaults_are_the_headers_and_pass_the_checks():
    from staticfusion_amd import deform

    p = deform.default_params()
    assert (p.time_window, list(p.reserved)) == (float("inf"), [0] * 7)
    assert bytes(p) == bytes(deform.Params()) and p.time_window == dr.DEFAULTS["time_window"]
    deform.check_params(p)
    v = deform.default_solve_params()
    keys = ("time_window", "w_reg", "damping", "iterations")
    assert tuple(getattr(v, k) for k in keys) == (float("inf"), 1.0, np.float32(1e-6), 8) and list(v.reserved) == [0] * 4
    assert bytes(v) == bytes(deform.SolveParams()) and tuple(getattr(v, k) for k in keys) == tuple(np.float32(dr.SOLVE_DEFAULTS[k]) for k in keys)
    deform.check_solve_params(v)
    b = deform._product()
    assert b.default_params(None) == -1 and b.default_solve_params(None) == -1
    txt = open(HEADER).read()
    assert len(re.findall(r"parameter defaults, NOT tuned values", txt)) == 2
    assert "time_window +inf. These" in txt and "time_window +inf, w_reg 1, damping 1e-6, iterations 8." in txt


def test_check_params_without_a_gpu():
    from staticfusion_amd import SfError, deform

    b = deform._product()
    assert b.check_params(None) == -1 and b.check_solve_params(None) == -1  # null: SF_ERR_ARG
    nan, inf = float("nan"), float("inf")
    for kw in (dict(time_window=0.0), dict(time_window=1e-30), dict(time_window=inf), dict(time_window=1e30)):
        deform.check_params(deform.Params(**kw))
    p = deform.Params()
    p.reserved[3] = -12345  # not read
    deform.check_params(p)
    for kw in (dict(time_window=nan), dict(time_window=-inf), dict(time_window=-1e-30), dict(time_window=-1.0)):
        with pytest.raises(SfError, match="failed with -1"):
            deform.check_params(deform.Params(**kw))
    for kw in (dict(time_window=0.0), dict(time_window=inf), dict(w_reg=0.0), dict(w_reg=1e30), dict(damping=0.0), dict(damping=1e30), dict(iterations=1),
               dict(iterations=32)):
        deform.check_solve_params(deform.SolveParams(**kw))
    bad = [dict(time_window=nan), dict(time_window=-inf), dict(time_window=-1.0), dict(w_reg=nan), dict(w_reg=inf), dict(w_reg=-inf), dict(w_reg=-1e-9),
           dict(damping=nan), dict(damping=inf), dict(damping=-inf), dict(damping=-1e-9), dict(iterations=0), dict(iterations=-1), dict(iterations=33)]
    for kw in bad:
        with pytest.raises(SfError, match="failed with -1"):
            deform.check_solve_params(deform.SolveParams(**kw))


def test_the_pure_host_calls_refuse_what_the_header_lists():
    from staticfusion_amd import SfError, deform

    pos, times = np.zeros((2, 3), np.float32), np.zeros(2, np.float32)
    M = np.tile(np.eye(3, 4, dtype=np.float32), (2, 1, 1))
    s = np.zeros(12, np.float32)
    with pytest.raises(SfError, match="failed with -1"):
        deform.bind_point(np.zeros((0, 3)), np.zeros(0), [0, 0, 0], 0.0)  # G == 0
    with pytest.raises(SfError, match="failed with -1"):
        deform.bind_point(np.zeros((1025, 3)), np.zeros(1025), [0, 0, 0], 0.0)  # G > SFD_MAX_NODES
    for window in (float("nan"), -1.0):
        with pytest.raises(SfError, match="failed with -1"):
            deform.bind_point(pos, times, [0, 0, 0], 0.0, window)
        with pytest.raises(SfError, match="failed with -1"):
            deform.edges(pos, times, window)
    bad_M = M.copy()
    bad_M[1, 2, 3] = np.inf
    with pytest.raises(SfError, match="failed with -1"):
        deform.deform_surfel(pos, times, bad_M, s)
    with pytest.raises(SfError, match="failed with -1"):
        deform.deform_poses(pos, times, bad_M, [np.eye(4)], [0.0])
    bad_pose = np.eye(4, dtype=np.float32)
    bad_pose[0, 0] = np.nan
    with pytest.raises(SfError, match="failed with -1"):
        deform.deform_poses(pos, times, M, [bad_pose], [0.0])
    with pytest.raises(SfError, match="failed with -1"):
        deform.solve(np.zeros((257, 3)), np.zeros(257), np.zeros((1, 3)), np.zeros((1, 3)), 0.0)  # G > SFD_SOLVE_MAX_NODES
    with pytest.raises(SfError, match="failed with -1"):
        deform.solve(pos, times, [[np.nan, 0, 0]], [[0, 0, 0]], 0.0)
    with pytest.raises(SfError, match="failed with -1"):
        deform.solve(pos, times, [[0, 0, 0]], [[0, 0, 0]], 0.0, weights=-1.0)
    with pytest.raises(SfError, match="failed with -1"):
        deform.solve(pos, times, [[0, 0, 0]], [[0, 0, 0]], 0.0, M=bad_M)
