"""The carve (include/sf_carve.h), the checks that need no GPU: the header, the ctypes table of staticfusion_amd/carve.py and the
exports of the three libraries name the same functions -- none of them part of include/sf.h, whose version has not moved, like
those of the other companions --, nothing of the parts' lifetime or of the shared rule text is exported, no other header,
binding or oracle source names them, the structs have the documented sizes, offsets and field order, the defaults are the
header's, and the pure-host calls refuse every case of the header's list."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import carve_cases as cc
import carve_ref as cr
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "sf_carve.h")


def declared():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)  # declarations only: the comments name the functions too
    return sorted(set(re.findall(r"\b(sfe_\w+)\s*\(", txt)))


def test_header_table_and_exports_name_the_same_functions():
    import staticfusion_amd as sf
    from staticfusion_amd import align, bodies, body_maps, capi, carve, closure, deform, join, keyframes, map_window, regions, score, streams, tracks, view

    names = declared()
    assert names == ["sfe_carve_images", "sfe_carve_streams", "sfe_carver_create", "sfe_carver_destroy", "sfe_check_params", "sfe_counts_bytes", "sfe_decide",
                     "sfe_default_params", "sfe_observe", "sfe_params_bytes", "sfe_version"]
    assert names == sorted(carve.SIGNATURES.keys())
    for lib in ("libsf_hip.so", "libsf_hip_precise.so", "libsf_hip_reforder.so"):  # the three link the same host objects
        path = os.path.join(os.path.dirname(sf.LIB), lib)
        assert os.path.exists(path), lib
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert sorted(set(re.findall(r" T (sfe_\w+)", out))) == names, lib
        assert "sfe_observe_core" not in out and "sfe_decide_core" not in out and "sfe_dot" not in out, "the shared text is not exported"
        assert not re.search(r"SfPart|shelled|orphan_all|part_destroy|check_part|check_live_handle|_ZT[VIS]\d+sfe_carver", out), lib
    # a companion of the ABI, not a part of it; no other header or binding names sfe_*, and this header names none of the
    # prefixes the other ABI tests search every header for, nor the oracle's
    for path in glob.glob(os.path.join(ROOT, "include", "*")):
        if os.path.basename(path) != "sf_carve.h":
            assert "sfe_" not in open(path).read(), path
    txt = open(HEADER).read()
    for prefix in ("sfa_", "sfb_", "sfc_", "sfd_", "sfj_", "sfp_", "sft_", "sfo_", "SF_FN"):
        assert prefix not in txt, prefix
    assert re.findall(r'#include\s+"([^"]+)"', txt) == ["sf.h", "sf_view.h"]
    assert re.search(r"#define\s+SF_ABI_VERSION\s+5\b", open(os.path.join(ROOT, "include", "sf.h")).read())
    assert not any(k.startswith("sfe") or "carve" in k for k in capi.SIGNATURES)  # (the names of sf.h without "sf_")
    others = (align, bodies, body_maps, closure, deform, join, keyframes, map_window, regions, score, streams, tracks, view)
    for other in others:
        assert not any(k.startswith("sfe_") for k in other.SIGNATURES), other.__name__
    assert tuple(o.version() for o in others) == (1,) * 13
    assert carve.version() == 1 == carve.VERSION
    assert carve._product().api.lib is sf.load().lib and carve._product().api.lib is score._product().api.lib  # one loaded copy
    for path in glob.glob(os.path.join(ROOT, "oracle", "*")):  # the oracle's sources do not have the prefix
        if os.path.isfile(path) and not path.endswith(".so"):
            assert "sfe_" not in open(path, errors="replace").read(), path
    # the constants of the header are the binding's and the restatement's
    consts = dict(re.findall(r"#define\s+(SFE_\w+)\s+(\d+)", txt))
    classes = ("UNSEEN", "THROUGH", "SUPPORTED", "OCCLUDED")
    assert [int(consts["SFE_CLASS_" + k]) for k in classes] == [getattr(carve, "CLASS_" + k) for k in classes] == [getattr(cr, k) for k in classes] == [0, 1, 2, 3]
    assert int(consts["SFE_MAX_WINDOW"]) == carve.MAX_WINDOW == 3
    # the header states its rules, its refusals and what it leaves out
    for word in ("OBSERVE", "DECIDE", "EFFECT", "REFUSALS", "OUT OF SCOPE", "UNMEASURED", "NOT TOUCHED AT ALL", "AFTER A CALL THAT CHANGES A MAP", "sfw_cull_maps",
                 "sfs_score_", "sfv_check_view", "b images", "lowering confidence", "votes kept from call to call", "paging the carved surfels out",
                 "a device-pointer form", "writing anything into a stream"):
        assert word in txt, word
    # the line of sf_body_maps.h that names this interface's job keeps its text
    assert "free-space violations" in open(os.path.join(ROOT, "include", "sf_body_maps.h")).read()
    # one part more, named where the parts are named
    csrc = os.path.join(ROOT, "staticfusion_amd", "csrc")
    assert re.search(r"^HOST_PARTS\s*:=.*\bclosure carve$", open(os.path.join(csrc, "Makefile")).read(), re.M)
    assert "sfe_*" in open(os.path.join(csrc, "sf_call_block.h")).read() and "sfe_carver" in open(os.path.join(csrc, "sf_parts.h")).read()
    assert "sf_hip_carve.hip" in open(os.path.join(csrc, "sf_host.h")).read()


def test_the_oracle_binding_is_refused(ora):
    from staticfusion_amd import SfError, carve

    with pytest.raises(SfError):
        carve._bind(ora)


def test_struct_sizes_and_layouts():
    from staticfusion_amd import carve

    b = carve._product()
    assert b.params_bytes() == C.sizeof(carve.SfeParams) == 48
    assert b.counts_bytes() == C.sizeof(carve.SfeCounts) == 32
    param_names = ("tol_abs", "tol_rel", "z_max", "min_cos", "window", "min_pixels", "min_votes", "max_support", "dry_run", "reserved")
    count_names = ("n_in", "n_judged", "n_through", "n_supported", "n_occluded", "n_carved", "n_out", "reserved")
    layouts = {"sfe_params": (carve.SfeParams, param_names, [0, 4, 8, 12, 16, 20, 24, 28, 32, 36]),
               "sfe_counts": (carve.SfeCounts, count_names, [0, 4, 8, 12, 16, 20, 24, 28])}
    txt = open(HEADER).read()
    for struct, (cls, names, offsets) in layouts.items():
        assert [getattr(cls, k).offset for k in names] == offsets, struct
        assert list(names) == [k for k, _ in cls._fields_], struct
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), txt, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body) == list(names), struct
    assert carve.COUNT_FIELDS == tuple(k for k in count_names if k != "reserved") == cr.COUNT_FIELDS


def test_defaults_are_the_headers_and_pass_the_checks():
    from staticfusion_amd import carve

    p = carve.default_params()
    keys = ("tol_abs", "tol_rel", "z_max", "min_cos", "window", "min_pixels", "min_votes", "max_support", "dry_run")
    assert tuple(getattr(p, k) for k in keys) == (np.float32(0.02), np.float32(0.01), 8.0, np.float32(0.2), 1, 5, 2, 0, 0) and list(p.reserved) == [0, 0, 0]
    assert bytes(p) == bytes(carve.Params()) == bytes(cc.as_product(cc.params()))
    assert sorted(cr.DEFAULTS) == sorted(keys) and all(np.float32(getattr(p, k)) == np.float32(cr.DEFAULTS[k]) for k in keys)
    carve.check_params(p)
    assert carve._product().default_params(None) == -1
    txt = open(HEADER).read()
    assert len(re.findall(r"parameter defaults, NOT tuned values", txt)) == 1
    assert "tol_abs 0.02, tol_rel 0.01, z_max 8, min_cos 0.2, window 1, min_pixels 5, min_votes 2, max_support 0, dry_run 0." in txt


def test_check_params_without_a_gpu():
    from staticfusion_amd import SfError, carve

    b = carve._product()
    assert b.check_params(None) == -1  # null: SF_ERR_ARG
    nan, inf = float("nan"), float("inf")
    good = [dict(tol_abs=0.0), dict(tol_rel=0.0), dict(tol_abs=1e30, tol_rel=1e30), dict(z_max=1e-30), dict(z_max=32.0), dict(min_cos=0.0), dict(min_cos=1.0),
            dict(window=0, min_pixels=1), dict(window=3, min_pixels=49), dict(window=2, min_pixels=25), dict(min_pixels=1), dict(min_pixels=9), dict(min_votes=1),
            dict(min_votes=65535), dict(max_support=65535), dict(dry_run=True)]
    for kw in good:
        carve.check_params(carve.Params(**kw))
    p = carve.Params()
    p.reserved[0], p.reserved[2] = -12345, 7  # not read
    carve.check_params(p)
    bad = [dict(tol_abs=nan), dict(tol_rel=nan), dict(z_max=nan), dict(min_cos=nan), dict(tol_abs=inf), dict(tol_rel=inf), dict(z_max=inf), dict(min_cos=inf),
           dict(tol_abs=-1e-9), dict(tol_rel=-1e-9), dict(tol_abs=-inf), dict(z_max=0.0), dict(z_max=-1.0), dict(z_max=np.nextafter(np.float32(32), np.float32(33))),
           dict(min_cos=-1e-9), dict(min_cos=np.nextafter(np.float32(1), np.float32(2))), dict(window=-1), dict(window=4), dict(min_pixels=0), dict(min_pixels=10),
           dict(window=0, min_pixels=2), dict(window=3, min_pixels=50), dict(min_pixels=-1), dict(min_votes=0), dict(min_votes=-1), dict(min_votes=65536),
           dict(max_support=-1), dict(max_support=65536), dict(dry_run=2), dict(dry_run=-1)]
    for kw in bad:
        with pytest.raises(SfError, match="failed with -1"):
            carve.check_params(carve.Params(**kw))


def test_observe_and_decide_refuse_what_the_header_lists():
    from staticfusion_amd import SfError, carve

    b = carve._product()
    fp = C.POINTER(C.c_float)
    s = cc.surfel()
    v = cc.as_product_view(cc.plain_view())
    img = np.full((v.cols, v.rows), 3.0, np.float32)
    out = np.full(5, -7, np.int32)  # the three counts with guard words around them
    found = C.cast(out.ctypes.data + 4, C.POINTER(C.c_int32))
    p = carve.Params(window=0, min_pixels=1)
    sp, ip = s.ctypes.data_as(fp), img.ctypes.data_as(fp)
    assert b.observe(sp, cc.TICK, C.byref(v), ip, C.byref(p), found) == carve.CLASS_THROUGH and list(out) == [-7, 1, 0, 0, -7]
    out[:] = -7
    assert b.observe(None, cc.TICK, C.byref(v), ip, C.byref(p), found) == -1 and b.observe(sp, cc.TICK, None, ip, C.byref(p), found) == -1
    assert b.observe(sp, cc.TICK, C.byref(v), None, C.byref(p), found) == -1 and b.observe(sp, cc.TICK, C.byref(v), ip, None, found) == -1
    assert b.observe(sp, cc.TICK, C.byref(v), ip, C.byref(p), None) == -1
    for kw in (dict(window=4), dict(min_pixels=0), dict(tol_abs=-1.0), dict(z_max=33.0), dict(min_cos=2.0), dict(min_votes=0), dict(dry_run=3)):
        bad = carve.Params(**kw)
        assert b.observe(sp, cc.TICK, C.byref(v), ip, C.byref(bad), found) == -1, kw
        assert b.decide(2, 0, C.byref(bad)) == -1, kw
    for kw in (dict(fx=0.0), dict(fy=float("nan")), dict(rows=0), dict(cols=4097), dict(max_depth=0.4)):
        bv = cc.plain_view()
        vars(bv).update(kw)
        assert b.observe(sp, cc.TICK, C.byref(cc.as_product_view(bv)), ip, C.byref(p), found) == -1, kw
    bv = cc.as_product_view(cc.plain_view())
    bv.pose[13] = float("inf")
    assert b.observe(sp, cc.TICK, C.byref(bv), ip, C.byref(p), found) == -1
    assert list(out) == [-7] * 5  # a refusal writes nothing
    for vt, vs in ((-1, 0), (0, -1), (65536, 0), (0, 65536)):
        assert b.decide(vt, vs, C.byref(p)) == -1
    assert b.decide(2, 0, None) == -1 and b.decide(2, 0, C.byref(carve.Params())) == 1 and b.decide(1, 0, C.byref(carve.Params())) == 0
    with pytest.raises(SfError, match="failed with -1"):
        carve.observe(s, cc.TICK, v, np.zeros((v.rows, v.cols), np.float32), carve.Params(window=7))
    with pytest.raises(SfError, match="failed with -1"):
        carve.decide(70000, 0)
    with pytest.raises(SfError):
        carve.observe(s, cc.TICK, v, np.zeros((v.rows + 1, v.cols), np.float32))  # an image of another size than the view
