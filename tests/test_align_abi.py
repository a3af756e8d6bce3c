"""Pose refinement (include/sf_align.h), the checks that need no GPU: the header, the ctypes table of staticfusion_amd/align.py
and the exports of the three libraries name the same ten functions -- none of them part of include/sf.h, whose version has
not moved, and no other header or binding names them --, the three structs have the documented sizes and offsets, the
defaults are the documented ones, and the pure-host parameter check refuses every case of the header's refusal list."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import align_ref
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "sf_align.h")


def declared():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)  # declarations only: the comments name the functions too
    return sorted(set(re.findall(r"\b(sfa_\w+)\s*\(", txt)))


def test_header_table_and_exports_name_the_same_functions():
    import staticfusion_amd as sf
    from staticfusion_amd import align, capi, keyframes, map_window, regions, score, streams, view

    names = declared()
    assert len(names) == 10 and "sfa_refine_streams" in names and "sfa_refine_images_device" in names and "sfa_step" in names
    assert names == sorted(align.SIGNATURES.keys())
    for lib in ("libsf_hip.so", "libsf_hip_precise.so", "libsf_hip_reforder.so"):  # the three link the same host objects
        path = os.path.join(os.path.dirname(sf.LIB), lib)
        assert os.path.exists(path), lib
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert sorted(set(re.findall(r" T (sfa_\w+)", out))) == names, lib
        assert "sfa_step_core" not in out and "sfv_draw_keys" not in out, "the shared step and drawing stage are not exported"
    # a companion of the ABI, not a part of it; no other header or binding names sfa_*
    for path in glob.glob(os.path.join(ROOT, "include", "*")):
        if os.path.basename(path) != "sf_align.h":
            assert "sfa_" not in open(path).read(), path
    assert "SF_FN" not in open(HEADER).read()
    assert re.search(r"#define\s+SF_ABI_VERSION\s+5\b", open(os.path.join(ROOT, "include", "sf.h")).read())
    assert not any(k.startswith("sfa") or "align" in k for k in capi.SIGNATURES)  # (its keys are the names of sf.h without "sf_")
    for other in (keyframes, map_window, regions, score, streams, view):
        assert not any(k.startswith("sfa_") for k in other.SIGNATURES), other.__name__
    assert (view.version(), score.version(), map_window.version(), streams.version(), keyframes.version(), regions.version()) == (1,) * 6
    assert align.version() == 1 == align.VERSION
    assert align._product().api.lib is sf.load().lib and align._product().api.lib is score._product().api.lib  # one loaded copy


def test_the_oracle_binding_is_refused(ora):
    from staticfusion_amd import SfError, align

    with pytest.raises(SfError):
        align._bind(ora)


def test_struct_sizes_offsets_and_defaults():
    from staticfusion_amd import align

    b = align._product()
    assert b.params_bytes() == C.sizeof(align.SfaParams) == 32
    assert b.result_bytes() == align.RESULT_DTYPE.itemsize == 128
    assert b.system_bytes() == align.SYSTEM_DTYPE.itemsize == align_ref.SYSTEM_DTYPE.itemsize == 256
    assert align.SYSTEM_DTYPE == align_ref.SYSTEM_DTYPE
    assert [getattr(align.SfaParams, k).offset for k, _ in align.SfaParams._fields_] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert [align.SYSTEM_DTYPE.fields[k][1] for k in align.SYSTEM_DTYPE.names] == [0, 8, 16, 64, 232]
    assert [align.RESULT_DTYPE.fields[k][1] for k in align.RESULT_DTYPE.names] == [0, 64, 68, 72, 80, 88, 96, 104]
    assert (align.OK, align.FEW_PAIRS, align.DEGENERATE) == (0, 1, 2) == (align_ref.OK, align_ref.FEW_PAIRS, align_ref.DEGENERATE)
    txt = open(HEADER).read()
    for name, value in (("SFA_OK", 0), ("SFA_FEW_PAIRS", 1), ("SFA_DEGENERATE", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), txt)
    d = align.default_params()
    want = (np.float32(0.15), np.float32(8), np.float32(0.5), np.float32(0), 10, 1, 64, 1)
    assert (d.dist_max, d.z_max, d.b_min, d.damping, d.iterations, d.stride, d.min_pairs, d.use_b) == want
    p = align.Params()
    assert (p.dist_max, p.z_max, p.b_min, p.damping, p.iterations, p.stride, p.min_pairs, p.use_b) == want
    assert b.default_params(None) == -1
    assert "NOT tuned" in txt and "nobody has tuned them" in txt  # the header says what the defaults are not
    for word in ("photometric", "frame normals", "robust weights", "pyramids", "back into a stream or a map"):
        assert word in txt.split("OUT OF SCOPE")[1], word


def test_check_params_without_a_gpu():
    from staticfusion_amd import SfError, align

    align.check_params(align.Params())
    align.check_params(align.Params(dist_max=1.0, z_max=32.0, b_min=-1.0, damping=0.0, iterations=64, stride=16, min_pairs=6, use_b=False))
    tiny = float(np.nextafter(np.float32(0), np.float32(1)))
    align.check_params(align.Params(dist_max=tiny, z_max=tiny, damping=1e30, iterations=1, stride=1, min_pairs=2 ** 31 - 1))
    nan, inf = float("nan"), float("inf")
    above = lambda v: float(np.nextafter(np.float32(v), np.float32(v + 1)))  # noqa: E731
    refused = [dict(dist_max=nan), dict(dist_max=inf), dict(z_max=nan), dict(z_max=inf), dict(b_min=nan), dict(b_min=inf), dict(b_min=-inf),
               dict(damping=nan), dict(damping=inf), dict(dist_max=0.0), dict(dist_max=-0.1), dict(dist_max=above(1)), dict(z_max=0.0), dict(z_max=-1.0),
               dict(z_max=above(32)), dict(damping=-1e-6), dict(iterations=0), dict(iterations=-1), dict(iterations=65), dict(stride=0), dict(stride=-2),
               dict(stride=17), dict(min_pairs=5), dict(min_pairs=0), dict(min_pairs=-64), dict(use_b=2), dict(use_b=-1)]
    for bad in refused:
        with pytest.raises(SfError, match="failed with -1"):
            align.check_params(align.Params(**bad))
    b = align._product()
    assert b.check_params(None) == -1  # null: SF_ERR_ARG
    assert b.check_params(C.byref(align.Params(use_b=7))) == -1
    # sfa_step refuses null arguments and touches nothing
    rec = np.zeros(1, align.SYSTEM_DTYPE)
    d = np.full(12, 7.0)
    dp = d.ctypes.data_as(C.POINTER(C.c_double))
    assert b.step(None, 0.0, dp, dp) == -1 and b.step(rec.ctypes.data, 0.0, None, dp) == -1 and b.step(rec.ctypes.data, 0.0, dp, None) == -1
    assert (d == 7.0).all()
