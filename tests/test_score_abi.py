"""Pose scoring (include/sf_score.h), the checks that need no GPU: the header, the ctypes table of staticfusion_amd/score.py
and the exports of the three libraries name the same functions -- none of them part of include/sf.h, whose version has not
moved, like that of the views --, the two structs have the documented sizes, the defaults are the documented ones, and the
pure-host parameter check refuses every case of the header's refusal list."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "sf_score.h")


def declared():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)  # declarations only: the comments name the functions too
    return sorted(set(re.findall(r"\b(sfs_\w+)\s*\(", txt)))


def test_header_table_and_exports_name_the_same_functions():
    import staticfusion_amd as sf
    from staticfusion_amd import capi, score, view

    names = declared()
    assert len(names) == 8 and "sfs_score_streams" in names and "sfs_score_images_device" in names
    assert names == sorted(score.SIGNATURES.keys())
    for lib in ("libsf_hip.so", "libsf_hip_precise.so", "libsf_hip_reforder.so"):  # the three link the same host objects
        path = os.path.join(os.path.dirname(sf.LIB), lib)
        assert os.path.exists(path), lib
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert sorted(set(re.findall(r" T (sfs_\w+)", out))) == names, lib
        assert "sfv_plan" not in out and "sfv_draw_keys" not in out, "the shared drawing stage is not exported"
    # a companion of the ABI, not a part of it
    sf_h = open(os.path.join(ROOT, "include", "sf.h")).read()
    assert "sfs_" not in sf_h and "SF_FN" not in open(HEADER).read()
    assert re.search(r"#define\s+SF_ABI_VERSION\s+5\b", sf_h)
    assert not any(k.startswith("sfs") or "score" in k for k in capi.SIGNATURES)  # (its keys are the names of sf.h without "sf_")
    assert not any(k.startswith("sfs_") for k in view.SIGNATURES)
    assert view.version() == 1 and score.version() == 1 == score.VERSION
    assert score._product().api.lib is sf.load().lib and score._product().api.lib is view._product().api.lib  # one loaded copy


def test_the_oracle_binding_is_refused(ora):
    from staticfusion_amd import SfError, score

    with pytest.raises(SfError):
        score._bind(ora)


def test_struct_sizes_and_defaults():
    from staticfusion_amd import score

    b = score._product()
    assert b.params_bytes() == ctypes.sizeof(score.SfsParams) == 32
    assert b.score_bytes() == score.SCORE_DTYPE.itemsize == 96
    assert score.SCORE_DTYPE.names[:10] == score.FIELDS and all(score.SCORE_DTYPE.fields[k][1] == 8 * q for q, k in enumerate(score.FIELDS))
    d = score.default_params()
    want = (np.float32(0.02), np.float32(0.01), np.float32(8), np.float32(0.5), 1, 1)
    assert (d.tol_abs, d.tol_rel, d.max_residual, d.b_min, d.use_grey, d.use_b) == want
    p = score.Params()
    assert (p.tol_abs, p.tol_rel, p.max_residual, p.b_min, p.use_grey, p.use_b) == want
    assert b.default_params(None) == -1
    txt = open(HEADER).read()
    assert "NOT acceptance" in txt and "nobody has tuned them" in txt  # the header says what the defaults are not


def test_check_params_without_a_gpu():
    from staticfusion_amd import SfError, score

    score.check_params(score.Params())
    score.check_params(score.Params(tol_abs=0.0, tol_rel=0.0, max_residual=32.0, b_min=-1.0, use_grey=False, use_b=False))
    score.check_params(score.Params(max_residual=float(np.nextafter(np.float32(0), np.float32(1)))))
    nan, inf = float("nan"), float("inf")
    refused = [dict(tol_abs=nan), dict(tol_abs=inf), dict(tol_rel=nan), dict(tol_rel=inf), dict(max_residual=nan), dict(max_residual=inf),
               dict(b_min=nan), dict(b_min=inf), dict(b_min=-inf), dict(tol_abs=-1e-6), dict(tol_rel=-0.5), dict(max_residual=0.0),
               dict(max_residual=-1.0), dict(max_residual=float(np.nextafter(np.float32(32), np.float32(33)))), dict(use_grey=2), dict(use_grey=-1),
               dict(use_b=2), dict(use_b=-1)]
    for bad in refused:
        with pytest.raises(SfError, match="failed with -1"):
            score.check_params(score.Params(**bad))
    b = score._product()
    assert b.check_params(None) == -1  # null: SF_ERR_ARG
    assert b.check_params(ctypes.byref(score.Params(use_b=7))) == -1


def test_derived_fields():
    from staticfusion_amd import score

    rec = np.zeros(2, score.RESULT_DTYPE)
    rec[0] = (10, 1, 20, 8, 6, 1, 1, 8 * 16384, 8 * 16384 * 16384, 0)
    d = score.derived(rec)
    assert d["inlier_ratio"].tolist() == [0.75, 0.0] and d["overlap"].tolist() == [0.8, 0.0]
    assert d["mean_abs"].tolist() == [1.0, 0.0] and d["rms"].tolist() == [1.0, 0.0]
