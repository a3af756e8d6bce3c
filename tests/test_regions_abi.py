"""Moving regions (include/sf_regions.h), the checks that need no GPU: the header, the ctypes table of
staticfusion_amd/regions.py and the exports of the three libraries name the same functions, the nine the header lists -- none of them part of
include/sf.h, whose version has not moved, like those of the other companions --, the three structs have the documented
sizes, the defaults are the header's, and the pure-host parameter check refuses every case of the header's list."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import region_ref as rr
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "sf_regions.h")


def declared():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)  # declarations only: the comments name the functions too
    return sorted(set(re.findall(r"\b(sfr_\w+)\s*\(", txt)))


def test_header_table_and_exports_name_the_same_functions():
    import staticfusion_amd as sf
    from staticfusion_amd import capi, keyframes, map_window, regions, score, streams, view

    names = declared()
    assert len(names) == 9 and "sfr_label_streams" in names and "sfr_label_images_device" in names and "sfr_summary_bytes" in names
    assert names == sorted(regions.SIGNATURES.keys())
    for lib in ("libsf_hip.so", "libsf_hip_precise.so", "libsf_hip_reforder.so"):  # the three link the same host objects
        path = os.path.join(os.path.dirname(sf.LIB), lib)
        assert os.path.exists(path), lib
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert sorted(set(re.findall(r" T (sfr_\w+)", out))) == names, lib
    # a companion of the ABI, not a part of it
    sf_h = open(os.path.join(ROOT, "include", "sf.h")).read()
    assert "sfr_" not in sf_h and "SF_FN" not in open(HEADER).read()
    assert re.search(r"#define\s+SF_ABI_VERSION\s+5\b", sf_h)
    assert not any(k.startswith("sfr") or "region" in k for k in capi.SIGNATURES)  # (its keys are the names of sf.h without "sf_")
    for other in (view, score, map_window, streams, keyframes):
        assert not any(k.startswith("sfr_") for k in other.SIGNATURES)
        assert other.version() == 1
    assert regions.version() == 1 == regions.VERSION
    assert regions._product().api.lib is sf.load().lib and regions._product().api.lib is score._product().api.lib  # one loaded copy


def test_the_oracle_binding_is_refused(ora):
    from staticfusion_amd import SfError, regions

    with pytest.raises(SfError):
        regions._bind(ora)


def test_struct_sizes_and_layouts():
    from staticfusion_amd import regions

    b = regions._product()
    assert b.params_bytes() == C.sizeof(regions.SfrParams) == 32
    assert b.region_bytes() == regions.REGION_DTYPE.itemsize == rr.REGION_DTYPE.itemsize == 64
    assert b.summary_bytes() == regions.SUMMARY_DTYPE.itemsize == rr.SUMMARY_DTYPE.itemsize == 32
    assert regions.REGION_DTYPE == rr.REGION_DTYPE and regions.SUMMARY_DTYPE == rr.SUMMARY_DTYPE
    assert [regions.REGION_DTYPE.fields[k][1] for k in regions.REGION_FIELDS] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56]


def test_defaults_are_the_headers_and_pass_the_check():
    from staticfusion_amd import regions

    p = regions.default_params()
    got = (p.z_max, p.b_max, p.dz_abs, p.dz_rel, p.connectivity, p.min_pixels, p.use_b)
    assert got == (8.0, 0.5, np.float32(0.05), np.float32(0.02), 8, 16, 1)
    q = regions.Params()
    assert bytes(p) == bytes(q)
    assert got == tuple(np.float32(rr.DEFAULTS[k]) if isinstance(rr.DEFAULTS[k], float) else rr.DEFAULTS[k]
                        for k in ("z_max", "b_max", "dz_abs", "dz_rel", "connectivity", "min_pixels", "use_b"))
    regions.check_params(p)
    assert regions._product().default_params(None) == -1
    txt = open(HEADER).read()
    assert re.search(r"parameter defaults, NOT\s+\*?\s*tuned thresholds", txt)


def test_check_params_without_a_gpu():
    from staticfusion_amd import SfError, regions

    b = regions._product()
    assert b.check_params(None) == -1  # null: SF_ERR_ARG
    nan, inf = float("nan"), float("inf")
    good = [dict(z_max=32.0), dict(z_max=1e-6), dict(b_max=-3.0), dict(b_max=1e30), dict(dz_abs=0.0, dz_rel=0.0), dict(connectivity=4), dict(min_pixels=1),
            dict(min_pixels=2 ** 31 - 1), dict(use_b=0)]
    for kw in good:
        regions.check_params(regions.Params(**kw))
    p = regions.Params()
    p.reserved = -12345  # not read
    regions.check_params(p)
    bad = [dict(z_max=0.0), dict(z_max=-1.0), dict(z_max=32.000004), dict(z_max=nan), dict(z_max=inf), dict(b_max=nan), dict(b_max=inf), dict(b_max=-inf),
           dict(dz_abs=-1e-9), dict(dz_abs=nan), dict(dz_abs=inf), dict(dz_rel=-1e-9), dict(dz_rel=nan), dict(dz_rel=inf), dict(connectivity=0),
           dict(connectivity=6), dict(connectivity=-8), dict(connectivity=16), dict(min_pixels=0), dict(min_pixels=-1), dict(use_b=2), dict(use_b=-1)]
    for kw in bad:
        with pytest.raises(SfError, match="failed with -1"):
            regions.check_params(regions.Params(**kw))
