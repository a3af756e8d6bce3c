"""Joined and thinned maps (include/sf_join.h), the checks that need no GPU: the header, the ctypes table of
staticfusion_amd/join.py and the exports of the three libraries name the same eleven functions -- none of them part of
include/sf.h, whose version has not moved, and no other header or binding names them --, the two structs have the documented
sizes and offsets, the defaults are the documented ones, and the pure-host parameter check refuses every case of the header."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "sf_join.h")


def declared():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)  # declarations only: the comments name the functions too
    return sorted(set(re.findall(r"\b(sfj_\w+)\s*\(", txt)))


def test_header_table_and_exports_name_the_same_functions():
    import staticfusion_amd as sf
    from staticfusion_amd import align, capi, join, keyframes, map_window, regions, score, streams, view

    names = declared()
    assert len(names) == 11 and "sfj_thin_maps" in names and "sfj_merge_maps" in names and "sfj_thin_extract" in names
    assert names == sorted(join.SIGNATURES.keys())
    for lib in ("libsf_hip.so", "libsf_hip_precise.so", "libsf_hip_reforder.so"):  # the three link the same host objects
        path = os.path.join(os.path.dirname(sf.LIB), lib)
        assert os.path.exists(path), lib
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert sorted(set(re.findall(r" T (sfj_\w+)", out))) == names, lib
    # a companion of the ABI, not a part of it; no other header or binding names sfj_*
    for path in glob.glob(os.path.join(ROOT, "include", "*")):
        if os.path.basename(path) != "sf_join.h":
            assert "sfj_" not in open(path).read(), path
    assert "SF_FN" not in open(HEADER).read()
    assert re.search(r"#define\s+SF_ABI_VERSION\s+5\b", open(os.path.join(ROOT, "include", "sf.h")).read())
    assert not any(k.startswith("sfj") or "join" in k or "thin" in k or "merge" in k for k in capi.SIGNATURES)  # (the names of sf.h without "sf_")
    for other in (align, keyframes, map_window, regions, score, streams, view):
        assert not any(k.startswith("sfj_") for k in other.SIGNATURES), other.__name__
    assert (view.version(), score.version(), map_window.version(), streams.version(), keyframes.version(), regions.version(), align.version()) == (1,) * 7
    assert join.version() == 1 == join.VERSION
    assert join._product().api.lib is sf.load().lib and join._product().api.lib is map_window._product().api.lib  # one loaded copy


def test_the_oracle_binding_is_refused(ora):
    from staticfusion_amd import SfError, join

    with pytest.raises(SfError):
        join._bind(ora)


def test_struct_sizes_offsets_and_defaults():
    from staticfusion_amd import join

    b = join._product()
    assert b.params_bytes() == C.sizeof(join.SfjParams) == 32
    assert b.counts_bytes() == C.sizeof(join.SfjCounts) == 32
    assert [getattr(join.SfjParams, k).offset for k, _ in join.SfjParams._fields_] == [0, 4, 8, 12, 16]
    assert [getattr(join.SfjCounts, k).offset for k, _ in join.SfjCounts._fields_] == [0, 4, 8, 12, 16, 20, 24]
    assert [k for k, _ in join.SfjCounts._fields_][:6] == list(join.COUNT_FIELDS)
    d = join.default_params()
    want = (np.float32(0.02), np.float32(0), -1, 0)
    assert (d.cell, d.min_confidence, d.stamp, d.dry_run) == want and list(d.reserved) == [0, 0, 0, 0]
    p = join.Params()
    assert (p.cell, p.min_confidence, p.stamp, p.dry_run) == want
    assert b.default_params(None) == -1
    txt = re.sub(r"[\s*]+", " ", open(HEADER).read())  # (the comment's line breaks and margin)
    for word in ("averaging the attributes", "thinning the destination", "an origin or a rotation", "levels of detail", "reordering", "refined pose"):
        assert word in txt.split("OUT OF SCOPE")[1], word


def test_check_params_without_a_gpu():
    from staticfusion_amd import SfError, join

    join.check_params(join.Params())
    tiny = float(np.nextafter(np.float32(0), np.float32(1)))
    smallest_with_finite_inverse = float(np.float32(2.0 ** -128))  # 1 / 2^-128 = 2^128 overflows; 2^-127 does not
    join.check_params(join.Params(cell=float(np.float32(2.0 ** -127)), min_confidence=-3.0, stamp=-7, dry_run=True))
    join.check_params(join.Params(cell=3e38, min_confidence=float("inf"), stamp=2 ** 31 - 1))
    join.check_params(join.Params(min_confidence=float("-inf")))
    nan, inf = float("nan"), float("inf")
    refused = [dict(cell=nan), dict(cell=inf), dict(cell=-inf), dict(cell=0.0), dict(cell=-0.0), dict(cell=-0.02), dict(cell=tiny),
               dict(cell=smallest_with_finite_inverse), dict(min_confidence=nan)]
    for bad in refused:
        with pytest.raises(SfError, match="failed with -1"):
            join.check_params(join.Params(**bad))
    b = join._product()
    assert b.check_params(None) == -1  # null: SF_ERR_ARG
    for dry in (2, -1, 7):
        p = join.Params()
        p.dry_run = dry
        assert b.check_params(C.byref(p)) == -1
    # the pure-host functions refuse what they cannot answer and write nothing
    key = C.c_uint64(77)
    pos = (C.c_float * 3)(0.0, 0.0, 0.0)
    assert b.voxel_key(None, pos, C.byref(key)) == -1 and b.voxel_key(C.byref(join.Params()), None, C.byref(key)) == -1
    assert b.voxel_key(C.byref(join.Params()), pos, None) == -1 and b.voxel_key(C.byref(join.Params(cell=nan)), pos, C.byref(key)) == -1
    assert key.value == 77
    assert b.table_slots(-1) == -1 and b.table_slots(2 ** 29 + 1) == -1 and b.table_slots(2 ** 29) == 2 ** 30
    for slots in (0, -64, 32, 63, 65, 96, 2 ** 31 - 1):
        assert b.hash_slot(5, slots) == -1, slots
