"""Region tracks (include/sf_tracks.h), the checks that need no GPU: the header, the ctypes table of staticfusion_amd/tracks.py and
the exports of the three libraries name the same functions -- none of them part of include/sf.h, whose version has not moved,
like those of the other companions --, no other header or binding names them, the structs have the documented sizes and
offsets, the defaults are the header's, and the pure-host parameter check refuses every case of the header's list."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import track_ref as tr
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "sf_tracks.h")


def declared():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)  # declarations only: the comments name the functions too
    return sorted(set(re.findall(r"\b(sft_\w+)\s*\(", txt)))


def test_header_table_and_exports_name_the_same_functions():
    import staticfusion_amd as sf
    from staticfusion_amd import align, capi, join, keyframes, map_window, regions, score, streams, tracks, view

    names = declared()
    assert len(names) == 19 and "sft_update_streams" in names and "sft_update_images_device" in names and "sft_assign" in names and "sft_relative" in names
    assert names == sorted(tracks.SIGNATURES.keys())
    for lib in ("libsf_hip.so", "libsf_hip_precise.so", "libsf_hip_reforder.so"):  # the three link the same host objects
        path = os.path.join(os.path.dirname(sf.LIB), lib)
        assert os.path.exists(path), lib
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert sorted(set(re.findall(r" T (sft_\w+)", out))) == names, lib
    # a companion of the ABI, not a part of it; no other header or binding names sft_*, and this header names neither of the
    # two prefixes the other ABI tests search every header for
    for path in glob.glob(os.path.join(ROOT, "include", "*")):
        if os.path.basename(path) != "sf_tracks.h":
            assert "sft_" not in open(path).read(), path
    txt = open(HEADER).read()
    assert "sfa_" not in txt and "sfj_" not in txt and "SF_FN" not in txt
    assert re.search(r"#define\s+SF_ABI_VERSION\s+5\b", open(os.path.join(ROOT, "include", "sf.h")).read())
    assert not any(k.startswith("sft") or "track" in k for k in capi.SIGNATURES)  # (the names of sf.h without "sf_")
    others = (align, join, keyframes, map_window, regions, score, streams, view)
    for other in others:
        assert not any(k.startswith("sft_") for k in other.SIGNATURES), other.__name__
    assert tuple(o.version() for o in others) == (1,) * 8
    assert tracks.version() == 1 == tracks.VERSION
    assert tracks._product().api.lib is sf.load().lib and tracks._product().api.lib is regions._product().api.lib  # one loaded copy


def test_the_oracle_binding_is_refused(ora):
    from staticfusion_amd import SfError, tracks

    with pytest.raises(SfError):
        tracks._bind(ora)


def test_struct_sizes_and_layouts():
    from staticfusion_amd import tracks

    b = tracks._product()
    assert b.camera_bytes() == C.sizeof(tracks.SftCamera) == 80 and b.params_bytes() == C.sizeof(tracks.SftParams) == 32
    assert b.track_bytes() == tracks.TRACK_DTYPE.itemsize == tr.TRACK_DTYPE.itemsize == 136
    assert b.summary_bytes() == tracks.SUMMARY_DTYPE.itemsize == tr.SUMMARY_DTYPE.itemsize == 32
    assert b.info_bytes() == tracks.INFO_DTYPE.itemsize == 32 and b.slot_bytes() == tracks.SLOT_DTYPE.itemsize == 16
    assert tracks.TRACK_DTYPE == tr.TRACK_DTYPE and tracks.SUMMARY_DTYPE == tr.SUMMARY_DTYPE
    assert [tracks.TRACK_DTYPE.fields[k][1] for k in tracks.TRACK_FIELDS] == list(range(0, 56, 4))
    assert [tracks.TRACK_DTYPE.fields[k][1] for k in ("qmin", "qmax", "sum_v", "sum_u", "sum_z", "sum_b", "sum_q")] == [56, 68, 80, 88, 96, 104, 112]
    assert [tracks.SUMMARY_DTYPE.fields[k][1] for k in tracks.SUMMARY_FIELDS] == list(range(0, 32, 4))
    assert [getattr(tracks.SftCamera, k).offset for k in ("pose", "cx", "cy", "fx", "fy")] == [0, 64, 68, 72, 76]
    assert [getattr(tracks.SftParams, k).offset for k in ("min_overlap", "min_share", "use_depth_gate", "dz_abs", "dz_rel", "reserved")] == [0, 4, 8, 12, 16, 20]
    # the struct declarations of the header, word for word in the order of the dtypes
    txt = open(HEADER).read()
    body = re.search(r"typedef struct sft_track \{(.*?)\} sft_track;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+)(?:\[3\])?\s*[,;]", body)
    assert fields == list(tracks.TRACK_DTYPE.names)


def test_defaults_are_the_headers_and_pass_the_check():
    from staticfusion_amd import tracks

    p = tracks.default_params()
    got = (p.min_overlap, p.min_share, p.use_depth_gate, p.dz_abs, p.dz_rel)
    assert got == (1, 256, 1, np.float32(0.10), np.float32(0.05))
    assert bytes(p) == bytes(tracks.Params())
    assert got == tuple(np.float32(tr.DEFAULTS[k]) if isinstance(tr.DEFAULTS[k], float) else tr.DEFAULTS[k]
                        for k in ("min_overlap", "min_share", "use_depth_gate", "dz_abs", "dz_rel"))
    tracks.check_params(p)
    assert tracks._product().default_params(None) == -1
    assert re.search(r"parameter defaults, NOT tuned values", open(HEADER).read())


def test_check_params_without_a_gpu():
    from staticfusion_amd import SfError, tracks

    b = tracks._product()
    assert b.check_params(None) == -1  # null: SF_ERR_ARG
    nan, inf = float("nan"), float("inf")
    good = [dict(min_overlap=1), dict(min_overlap=2 ** 31 - 1), dict(min_share=0), dict(min_share=1024), dict(use_depth_gate=0), dict(dz_abs=0.0, dz_rel=0.0),
            dict(dz_abs=1e30), dict(dz_rel=1e30)]
    for kw in good:
        tracks.check_params(tracks.Params(**kw))
    p = tracks.Params()
    p.reserved[0], p.reserved[2] = -12345, 7  # not read
    tracks.check_params(p)
    bad = [dict(min_overlap=0), dict(min_overlap=-1), dict(min_share=-1), dict(min_share=1025), dict(dz_abs=-1e-9), dict(dz_abs=nan), dict(dz_abs=inf),
           dict(dz_abs=-inf), dict(dz_rel=-1e-9), dict(dz_rel=nan), dict(dz_rel=inf), dict(use_depth_gate=2), dict(use_depth_gate=-1)]
    for kw in bad:
        with pytest.raises(SfError, match="failed with -1"):
            tracks.check_params(tracks.Params(**kw))
