"""Closure constraints (include/sf_closure.h), the checks that need no GPU: the header, the ctypes table of
staticfusion_amd/closure.py and the exports of the three libraries name the same functions -- none of them part of include/sf.h,
whose version has not moved, like those of the other companions --, no other header or binding names them, the header includes
sf.h, sf_view.h and sf_deform.h, the structs have the documented sizes, offsets and field order, a record has the layout of the
constraint of sf_deform.h, the defaults are the header's, and the pure-host calls refuse every case of the header's list."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import closure_cases as cc
import closure_ref as cr
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "sf_closure.h")


def declared():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)  # declarations only: the comments name the functions too
    return sorted(set(re.findall(r"\b(sfc_\w+)\s*\(", txt)))


def test_header_table_and_exports_name_the_same_functions():
    import staticfusion_amd as sf
    from staticfusion_amd import align, bodies, body_maps, capi, closure, deform, join, keyframes, map_window, regions, score, streams, tracks, view

    names = declared()
    assert names == ["sfc_build", "sfc_builder_create", "sfc_builder_destroy", "sfc_check_params", "sfc_counts_bytes", "sfc_default_params", "sfc_link_sample",
                     "sfc_max_records", "sfc_params_bytes", "sfc_version"]
    assert names == sorted(closure.SIGNATURES.keys())
    for lib in ("libsf_hip.so", "libsf_hip_precise.so", "libsf_hip_reforder.so"):  # the three link the same host objects
        path = os.path.join(os.path.dirname(sf.LIB), lib)
        assert os.path.exists(path), lib
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert sorted(set(re.findall(r" T (sfc_\w+)", out))) == names, lib
        assert "sfc_link_core" not in out and "orphan_builders" not in out, "the shared text is not exported"
        # ... nor what orphans a builder now (sf_parts.h, sf_host.h), nor the builder's own hook and type
        assert not re.search(r"SfPart|shelled|orphan_all|part_destroy|check_part|check_live_handle|_ZT[VIS]\d+sfc_builder", out), lib
    # a companion of the ABI, not a part of it; no other header or binding names sfc_*
    for path in glob.glob(os.path.join(ROOT, "include", "*")):
        if os.path.basename(path) != "sf_closure.h":
            assert "sfc_" not in open(path).read(), path
    txt = open(HEADER).read()
    assert re.findall(r'#include\s+"([^"]+)"', txt) == ["sf.h", "sf_view.h", "sf_deform.h"]
    assert "SF_FN" not in txt and "sfo_" not in txt
    assert re.search(r"#define\s+SF_ABI_VERSION\s+5\b", open(os.path.join(ROOT, "include", "sf.h")).read())
    assert not any(k.startswith("sfc") or "closure" in k for k in capi.SIGNATURES)  # (the names of sf.h without "sf_")
    others = (align, bodies, body_maps, deform, join, keyframes, map_window, regions, score, streams, tracks, view)
    for other in others:
        assert not any(k.startswith("sfc_") for k in other.SIGNATURES), other.__name__
    assert tuple(o.version() for o in others) == (1,) * 12
    assert closure.version() == 1 == closure.VERSION
    assert closure._product().api.lib is sf.load().lib and closure._product().api.lib is deform._product().api.lib  # one loaded copy
    for path in glob.glob(os.path.join(ROOT, "oracle", "*")):  # the oracle's sources do not have the prefix
        if os.path.isfile(path) and not path.endswith(".so"):
            assert "sfc_" not in open(path, errors="replace").read(), path
    # the constants of the header are the binding's and the restatement's
    consts = dict(re.findall(r"#define\s+(SFC_\w+)\s+(\d+)", txt))
    bits = ("BOTH", "NEAR", "APART", "LINK", "PIN", "LINK_DROPPED", "PIN_DROPPED")
    assert [int(consts["SFC_FOUND_" + k]) for k in bits] == [getattr(closure, "FOUND_" + k) for k in bits] == [getattr(cr, k) for k in bits] == [1, 2, 4, 8, 16, 32, 64]
    assert int(consts["SFC_MAX_STRIDE"]) == closure.MAX_STRIDE == 4096
    # the header states its rules, its refusals and what it leaves out
    for word in ("ENTRY q", "IMAGES.", "SAMPLES.", "PER SAMPLE", "OUTPUT ORDER", "COUNTS", "REFUSALS", "OUT OF SCOPE", "sfw_extract", "sfw_append", "invert = 1"):
        assert word in txt, word
    # the line of sf_deform.h that names this interface's job keeps its text
    assert "the solver (apply takes any A); building constraints; writing anything back" in open(os.path.join(ROOT, "include", "sf_deform.h")).read()


def test_the_oracle_binding_is_refused(ora):
    from staticfusion_amd import SfError, closure

    with pytest.raises(SfError):
        closure._bind(ora)


def test_struct_sizes_and_layouts():
    from staticfusion_amd import closure, deform

    b = closure._product()
    assert b.params_bytes() == C.sizeof(closure.SfcParams) == 32
    assert b.counts_bytes() == C.sizeof(closure.SfcCounts) == 64
    assert closure.RECORD.itemsize == cr.RECORD.itemsize == C.sizeof(deform.SfdConstraint) == deform._product().constraint_bytes() == 32
    assert [(k, closure.RECORD.fields[k][1]) for k in closure.RECORD.names] == [(k, getattr(deform.SfdConstraint, k).offset) for k, _ in deform.SfdConstraint._fields_]
    assert closure.RECORD == cr.RECORD
    count_names = ("n_samples", "n_new", "n_old", "n_both", "n_near", "n_apart", "n_links", "n_pins", "n_dropped", "first", "reserved", "sum_dz", "sum_shift")
    layouts = {"sfc_params": (closure.SfcParams, ("stride", "pins", "gate_abs", "gate_rel", "min_time_gap", "w_link", "w_pin", "reserved"), [0, 4, 8, 12, 16, 20, 24, 28]),
               "sfc_counts": (closure.SfcCounts, count_names, [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 48, 56]),
               "sfc_record": (None, closure.RECORD.names, [closure.RECORD.fields[k][1] for k in closure.RECORD.names])}
    txt = open(HEADER).read()
    for struct, (cls, names, offsets) in layouts.items():
        if cls is not None:
            assert [getattr(cls, k).offset for k in names] == offsets, struct
            assert list(names) == [k for k, _ in cls._fields_], struct
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), txt, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body) == list(names), struct
    assert layouts["sfc_record"][2] == [0, 12, 24, 28]
    assert closure.COUNT_FIELDS == tuple(k for k in count_names if k != "reserved") == cr.COUNT_FIELDS


def test_defaults_are_the_headers_and_pass_the_checks():
    from staticfusion_amd import closure

    p = closure.default_params()
    keys = ("stride", "pins", "gate_abs", "gate_rel", "min_time_gap", "w_link", "w_pin")
    assert tuple(getattr(p, k) for k in keys) == (4, 1, np.float32(0.1), np.float32(0.05), 0.0, 1.0, 1.0) and p.reserved == 0
    assert bytes(p) == bytes(closure.Params()) == bytes(cc.as_product(cc.params()))
    assert sorted(cr.DEFAULTS) == sorted(keys) and all(np.float32(getattr(p, k)) == np.float32(cr.DEFAULTS[k]) for k in keys)
    closure.check_params(p)
    assert closure._product().default_params(None) == -1
    txt = open(HEADER).read()
    assert len(re.findall(r"parameter defaults, NOT tuned values", txt)) == 1
    assert "stride 4, pins 1, gate_abs 0.1, gate_rel 0.05, min_time_gap 0, w_link 1, w_pin 1." in txt


def test_check_params_without_a_gpu():
    from staticfusion_amd import SfError, closure

    b = closure._product()
    assert b.check_params(None) == -1  # null: SF_ERR_ARG
    nan, inf = float("nan"), float("inf")
    good = [dict(stride=1), dict(stride=4096), dict(pins=0), dict(pins=2), dict(gate_abs=0.0), dict(gate_abs=inf), dict(gate_rel=0.0), dict(gate_rel=1e30),
            dict(min_time_gap=-inf), dict(min_time_gap=-1e30), dict(min_time_gap=1e30), dict(w_link=0.0), dict(w_pin=0.0), dict(w_link=1e30, w_pin=1e30)]
    for kw in good:
        closure.check_params(closure.Params(**kw))
    p = closure.Params()
    p.reserved = -12345  # not read
    closure.check_params(p)
    bad = [dict(stride=0), dict(stride=-1), dict(stride=4097), dict(pins=-1), dict(pins=3), dict(gate_abs=nan), dict(gate_rel=nan), dict(min_time_gap=nan),
           dict(w_link=nan), dict(w_pin=nan), dict(gate_abs=-1e-9), dict(gate_abs=-inf), dict(gate_rel=-1e-9), dict(gate_rel=inf), dict(gate_rel=-inf),
           dict(w_link=-1e-9), dict(w_link=inf), dict(w_link=-inf), dict(w_pin=-1e-9), dict(w_pin=inf), dict(w_pin=-inf), dict(min_time_gap=inf)]
    for kw in bad:
        with pytest.raises(SfError, match="failed with -1"):
            closure.check_params(closure.Params(**kw))


def test_max_records_without_a_gpu():
    from staticfusion_amd import SfError, closure

    for g in cc.GEOMS.values():
        v = cc.geom_view(g, cc.POSE_FROM)
        for stride in (1, 2, 3, 4, 7, 64, 4095, 4096):
            assert closure.max_records(v, stride) == cr.max_records(v.rows, v.cols, stride), (g, stride)
    big = cc.geom_view((4096, 4096, 2048.0, 2048.0, 3000.0, 3000.0), cc.POSE_FROM)
    assert closure.max_records(big, 1) == 2 * 4096 * 4096 and closure.max_records(big, 4096) == 2 and closure.max_records(big, 2048) == 2 * 4
    v = cc.geom_view(cc.GEOMS["64x48"], cc.POSE_FROM)
    assert closure._product().max_records(None, 1) == -1
    for stride in (0, -1, 4097):
        with pytest.raises(SfError, match="failed with -1"):
            closure.max_records(v, stride)
    bad = cc.geom_view(cc.GEOMS["64x48"], cc.POSE_FROM)
    bad.fx = 0.0  # a view sfv_check_view refuses
    with pytest.raises(SfError, match="failed with -1"):
        closure.max_records(bad, 1)
    bad = cc.geom_view(cc.GEOMS["64x48"], cc.POSE_FROM)
    bad.pose[3] = float("nan")
    with pytest.raises(SfError, match="failed with -1"):
        closure.max_records(bad, 1)


def test_link_sample_refuses_what_the_header_lists():
    from staticfusion_amd import SfError, closure

    b = closure._product()
    fp = C.POINTER(C.c_float)
    a, o = np.zeros(12, np.float32), np.zeros(12, np.float32)
    pose = np.ascontiguousarray(np.eye(4, dtype=np.float32).ravel())
    out = np.full(2, -7.0, closure.RECORD)
    before = out.tobytes()
    k = C.c_int32(-7)
    p = closure.Params()
    ap, op, pp = a.ctypes.data_as(fp), o.ctypes.data_as(fp), pose.ctypes.data_as(fp)
    z = C.c_float(1.0)
    assert b.link_sample(ap, op, z, z, None, pp, C.byref(p), out.ctypes.data, C.byref(k)) == -1  # null arguments
    assert b.link_sample(ap, op, z, z, pp, None, C.byref(p), out.ctypes.data, C.byref(k)) == -1
    assert b.link_sample(ap, op, z, z, pp, pp, None, out.ctypes.data, C.byref(k)) == -1
    assert b.link_sample(ap, op, z, z, pp, pp, C.byref(p), None, C.byref(k)) == -1
    assert b.link_sample(ap, op, z, z, pp, pp, C.byref(p), out.ctypes.data, None) == -1
    for kw in (dict(stride=0), dict(pins=3), dict(gate_abs=-1.0), dict(w_pin=float("inf")), dict(min_time_gap=float("inf")), dict(gate_rel=float("nan"))):
        bad = closure.Params(**kw)
        assert b.link_sample(ap, op, z, z, pp, pp, C.byref(bad), out.ctypes.data, C.byref(k)) == -1, kw
    for v in (np.nan, np.inf):
        bad_pose = pose.copy()
        bad_pose[13] = v
        assert b.link_sample(ap, op, z, z, bad_pose.ctypes.data_as(fp), pp, C.byref(p), out.ctypes.data, C.byref(k)) == -1
        assert b.link_sample(ap, op, z, z, pp, bad_pose.ctypes.data_as(fp), C.byref(p), out.ctypes.data, C.byref(k)) == -1
    assert out.tobytes() == before and k.value == -7  # a refusal writes nothing
    with pytest.raises(SfError, match="failed with -1"):
        closure.link_sample(a, o, 1.0, 1.0, np.eye(4), np.eye(4), closure.Params(pins=7))
    # both absences are no refusal: nothing is found
    mask, recs = closure.link_sample(None, None, 0.0, 0.0, np.eye(4), np.eye(4))
    assert mask == 0 and recs.shape == (0,)
