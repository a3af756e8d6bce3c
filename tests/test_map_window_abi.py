"""Bounded surfel maps (include/sf_map_window.h), the checks that need no GPU: the header, the ctypes table of
staticfusion_amd/map_window.py and the exports of the three libraries name the same functions -- none of them part of
include/sf.h --, the filter struct has the documented size, and the pure-host filter check accepts and refuses what the
header says."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "sf_map_window.h")


def declared():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)  # declarations only: the comments name the functions too
    return sorted(set(re.findall(r"\b(sfw_\w+)\s*\(", txt)))


def test_header_table_and_exports_name_the_same_functions():
    import staticfusion_amd as sf
    from staticfusion_amd import capi, map_window, streams

    names = declared()
    assert len(names) == 8 and "sfw_cull_maps" in names
    assert names == sorted(map_window.SIGNATURES.keys())
    out = subprocess.check_output(["nm", "-D", "--defined-only", sf.LIB]).decode()
    assert sorted(set(re.findall(r" T (sfw_\w+)", out))) == names
    # a companion of the ABI, not a part of it: sf.h declares none of them, its table has none
    sf_h = open(os.path.join(ROOT, "include", "sf.h")).read()
    assert "sfw_" not in sf_h and "SF_FN" not in open(HEADER).read()
    assert not any(k.startswith("sfw") or ("sfw_" + k) in names for k in capi.SIGNATURES)
    # the precise and reference-order libraries link the same host objects
    for other in ("libsf_hip_precise.so", "libsf_hip_reforder.so"):
        path = os.path.join(os.path.dirname(sf.LIB), other)
        assert os.path.exists(path), other
        o = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert sorted(set(re.findall(r" T (sfw_\w+)", o))) == names, other
    # both bindings -- and the stream migration's -- share one loaded copy of the library
    assert map_window._product().api.lib is sf.load().lib
    assert map_window._product().api.lib is streams._product().api.lib
    assert map_window.version() == 1 == map_window.VERSION


def test_the_oracle_binding_is_refused(ora):
    from staticfusion_amd import SfError, map_window

    with pytest.raises(SfError):
        map_window._bind(ora)


def test_filter_struct_size():
    from staticfusion_amd import map_window

    assert map_window.filter_bytes() == ctypes.sizeof(map_window.SfwFilter) == 32
    f = map_window.Filter()
    assert (f.min_confidence, f.max_age, tuple(f.centre), f.radius, f.invert) == (0.0, -1, (0.0, 0.0, 0.0), 0.0, 0)
    g = map_window.Filter(min_confidence=0.25, max_age=3, centre=[1, 2, 3], radius=4.5, invert=True)
    assert (g.min_confidence, g.max_age, tuple(g.centre), g.radius, g.invert) == (0.25, 3, (1.0, 2.0, 3.0), 4.5, 1)


def test_check_filter_without_a_gpu():
    from staticfusion_amd import SfError, map_window

    map_window.check_filter(map_window.Filter())  # the default filter
    map_window.check_filter(map_window.Filter(min_confidence=float("inf"), max_age=0, centre=[float("inf"), 0, 0], radius=1.0, invert=True))
    nan = float("nan")
    for bad in (dict(min_confidence=nan), dict(radius=nan), dict(centre=[nan, 0, 0]), dict(centre=[0, nan, 0]), dict(centre=[0, 0, nan], radius=2.0)):
        with pytest.raises(SfError, match="NaN"):
            map_window.check_filter(map_window.Filter(**bad))
    b = map_window._product()
    assert b.check_filter(None) != 0  # a null filter
