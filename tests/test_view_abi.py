"""Free-view rendering (include/sf_view.h), the checks that need no GPU: the header, the ctypes table of
staticfusion_amd/view.py and the exports of the three libraries name the same functions -- none of them part of
include/sf.h --, the view struct has the documented size, and the pure-host view check accepts the default view and refuses
every case of the header's refusal list."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "sf_view.h")


def declared():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)  # declarations only: the comments name the functions too
    return sorted(set(re.findall(r"\b(sfv_\w+)\s*\(", txt)))


def plain_view(**over):
    from staticfusion_amd import view

    kw = dict(pose=np.eye(4), cx=40.0, cy=30.0, fx=66.0, fy=66.0, rows=60, cols=80)
    kw.update(over)
    return view.View(**kw)


def test_header_table_and_exports_name_the_same_functions():
    import staticfusion_amd as sf
    from staticfusion_amd import capi, map_window, view

    names = declared()
    assert len(names) == 8 and "sfv_render_maps" in names and "sfv_render_surfels" in names
    assert names == sorted(view.SIGNATURES.keys())
    out = subprocess.check_output(["nm", "-D", "--defined-only", sf.LIB]).decode()
    assert sorted(set(re.findall(r" T (sfv_\w+)", out))) == names
    # a companion of the ABI, not a part of it: sf.h declares none of them, its table has none, its version has not moved
    sf_h = open(os.path.join(ROOT, "include", "sf.h")).read()
    assert "sfv_" not in sf_h and "SF_FN" not in open(HEADER).read()
    assert re.search(r"#define\s+SF_ABI_VERSION\s+5\b", sf_h)
    assert not any(k.startswith("sfv") or ("sfv_" + k) in names for k in capi.SIGNATURES)
    # the precise and reference-order libraries link the same host objects
    for other in ("libsf_hip_precise.so", "libsf_hip_reforder.so"):
        path = os.path.join(os.path.dirname(sf.LIB), other)
        assert os.path.exists(path), other
        o = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert sorted(set(re.findall(r" T (sfv_\w+)", o))) == names, other
    # this binding and the map window's share one loaded copy of the library
    assert view._product().api.lib is sf.load().lib
    assert view._product().api.lib is map_window._product().api.lib
    assert view.version() == 1 == view.VERSION


def test_the_oracle_binding_is_refused(ora):
    from staticfusion_amd import SfError, view

    with pytest.raises(SfError):
        view._bind(ora)


def test_view_struct_size_and_fields():
    from staticfusion_amd import view

    assert view.view_bytes() == ctypes.sizeof(view.SfvView) == 112
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = (1, 2, 3)
    v = view.View(T, 1.5, 2.5, 3.5, 4.5, 7, 9, min_confidence=0.5, max_depth=6.0, max_age=3, shade=view.SHADE_NORMAL)
    assert tuple(v.pose[12:15]) == (1.0, 2.0, 3.0)  # column-major: the translation is the last column
    assert (v.cx, v.cy, v.fx, v.fy, v.rows, v.cols, v.min_confidence, v.max_depth, v.max_age, v.shade) == (1.5, 2.5, 3.5, 4.5, 7, 9, 0.5, 6.0, 3, 1)
    assert np.array_equal(view.view_pose(v), T)
    d = plain_view()
    assert (d.min_confidence, d.max_depth, d.max_age, d.shade) == (0.25, 20.0, -1, view.SHADE_COLOUR)


def test_look_at_is_a_rigid_camera_pose():
    from staticfusion_amd import view

    T = view.look_at((1.0, -0.5, -2.0), (0.0, 0.0, 1.5))
    R = T[:3, :3].astype(np.float64)
    assert np.allclose(R.T @ R, np.eye(3), atol=1e-6) and np.linalg.det(R) > 0.999
    to_target = np.array([0.0, 0.0, 1.5]) - T[:3, 3]
    assert np.allclose(R[:, 2], to_target / np.linalg.norm(to_target), atol=1e-6)  # +z looks at the target
    assert R[1, 1] > 0  # +y (image rows) points down when the world's up is -y
    assert np.allclose(view.look_at((0, 0, 0), (0, 0, 1)), np.eye(4), atol=1e-7)


def test_check_view_without_a_gpu():
    from staticfusion_amd import SfError, view

    view.check_view(plain_view())  # what default_view fills, but for the handle's numbers
    view.check_view(plain_view(rows=1, cols=1))
    view.check_view(plain_view(rows=4096, cols=4096, min_confidence=0.0, max_age=0, shade=view.SHADE_NORMAL, fx=-5.0))
    nan, inf = float("nan"), float("inf")
    bad_pose = np.eye(4)
    bad_pose[1, 2] = nan
    inf_pose = np.eye(4)
    inf_pose[0, 3] = inf
    refused = [dict(pose=bad_pose), dict(pose=inf_pose), dict(cx=nan), dict(cy=inf), dict(fx=nan), dict(fy=-inf), dict(min_confidence=nan),
               dict(min_confidence=inf), dict(max_depth=nan), dict(max_depth=inf),
               dict(rows=0), dict(rows=4097), dict(cols=0), dict(cols=4097), dict(rows=-3),
               dict(fx=0.0), dict(fy=0.0), dict(fy=-0.0),
               dict(max_depth=0.4), dict(max_depth=0.0), dict(max_depth=-1.0), dict(max_depth=float(np.float32(0.4))),
               dict(shade=2), dict(shade=-1)]
    for bad in refused:
        with pytest.raises(SfError, match="failed with"):
            view.check_view(plain_view(**bad))
    view.check_view(plain_view(max_depth=float(np.nextafter(np.float32(0.4), np.float32(1)))))  # the first float above 0.4
    b = view._product()
    assert b.check_view(None) == -1  # a null view: SF_ERR_ARG
    assert b.check_view(ctypes.byref(plain_view(rows=0))) == -1
