"""Region motion (include/sf_bodies.h), the checks that need no GPU: the header, the ctypes table of staticfusion_amd/bodies.py and
the exports of the three libraries name the same functions -- none of them part of include/sf.h, whose version has not moved,
like those of the other companions --, no other header or binding names them, the structs have the documented sizes and
offsets (the camera and the system record those of the tracks and align headers), the defaults are the header's, and the
pure-host parameter check refuses every case of the header's list."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import body_ref as br
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "sf_bodies.h")


def declared():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)  # declarations only: the comments name the functions too
    return sorted(set(re.findall(r"\b(sfb_\w+)\s*\(", txt)))


def test_header_table_and_exports_name_the_same_functions():
    import staticfusion_amd as sf
    from staticfusion_amd import align, bodies, capi, join, keyframes, map_window, regions, score, streams, tracks, view

    names = declared()
    assert len(names) == 10 and "sfb_estimate_images" in names and "sfb_estimate_images_device" in names and "sfb_world_motion" in names
    assert names == sorted(bodies.SIGNATURES.keys())
    for lib in ("libsf_hip.so", "libsf_hip_precise.so", "libsf_hip_reforder.so"):  # the three link the same host objects
        path = os.path.join(os.path.dirname(sf.LIB), lib)
        assert os.path.exists(path), lib
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert sorted(set(re.findall(r" T (sfb_\w+)", out))) == names, lib
        assert "sfb_world_core" not in out and "handle_born" not in out and "handle_gone" not in out, "the shared text and the handle list are not exported"
    # a companion of the ABI, not a part of it; no other header or binding names sfb_*, and this header names none of the
    # prefixes the other ABI tests search every header for, nor the oracle's
    for path in glob.glob(os.path.join(ROOT, "include", "*")):
        if os.path.basename(path) != "sf_bodies.h":
            assert "sfb_" not in open(path).read(), path
    txt = open(HEADER).read()
    assert not any(p in txt for p in ("sfa_", "sfj_", "sft_", "sfo_", "SF_FN"))
    assert '#include "sf_tracks.h"' in txt and '#include "sf_align.h"' in txt
    assert re.search(r"#define\s+SF_ABI_VERSION\s+5\b", open(os.path.join(ROOT, "include", "sf.h")).read())
    assert not any(k.startswith("sfb") or "bod" in k for k in capi.SIGNATURES)  # (the names of sf.h without "sf_")
    others = (align, join, keyframes, map_window, regions, score, streams, tracks, view)
    for other in others:
        assert not any(k.startswith("sfb_") for k in other.SIGNATURES), other.__name__
    assert tuple(o.version() for o in others) == (1,) * 9
    assert bodies.version() == 1 == bodies.VERSION
    assert bodies._product().api.lib is sf.load().lib and bodies._product().api.lib is tracks._product().api.lib  # one loaded copy
    # the oracle's sources do not have the prefix
    for path in glob.glob(os.path.join(ROOT, "oracle", "*")):
        if os.path.isfile(path) and not path.endswith(".so"):
            assert "sfb_" not in open(path, errors="replace").read(), path


def test_the_oracle_binding_is_refused(ora):
    from staticfusion_amd import SfError, bodies

    with pytest.raises(SfError):
        bodies._bind(ora)


def test_struct_sizes_and_layouts():
    from staticfusion_amd import align, bodies, tracks

    b = bodies._product()
    assert b.params_bytes() == C.sizeof(bodies.SfbParams) == 32
    assert b.motion_bytes() == bodies.MOTION_DTYPE.itemsize == br.MOTION_DTYPE.itemsize == 192 and bodies.MOTION_DTYPE == br.MOTION_DTYPE
    assert b.camera_bytes() == C.sizeof(bodies.SfbCamera) == tracks._product().camera_bytes() == 80
    assert b.system_bytes() == align.SYSTEM_DTYPE.itemsize == align._product().system_bytes() == 256 and br.SYSTEM_DTYPE == align.SYSTEM_DTYPE
    assert [getattr(bodies.SfbParams, k).offset for k in ("dist_max", "z_max", "normal_dz", "damping", "iterations", "min_pairs", "reserved")] == [0, 4, 8, 12, 16, 20, 24]
    names = ("d", "w", "status", "iterations_done", "n_first", "ss_first", "n_last", "ss_last", "reserved")
    assert [bodies.MOTION_DTYPE.fields[k][1] for k in names] == [0, 64, 128, 132, 136, 144, 152, 160, 168]
    # the struct declarations of the header, word for word in the order of the dtypes; the two borrowed layouts against their headers
    txt = open(HEADER).read()

    def fields(header_text, struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header_text, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)

    assert fields(txt, "sfb_motion") == list(names)
    assert fields(txt, "sfb_params") == [k for k, _ in bodies.SfbParams._fields_]
    assert fields(txt, "sfb_camera") == fields(open(os.path.join(ROOT, "include", "sf_tracks.h")).read(), "sft_camera") == [k for k, _ in tracks.SftCamera._fields_]
    assert fields(txt, "sfb_system") == fields(open(os.path.join(ROOT, "include", "sf_align.h")).read(), "sfa_system") == list(align.SYSTEM_DTYPE.names)
    assert (bodies.OK, bodies.FEW_PAIRS, bodies.DEGENERATE) == (align.OK, align.FEW_PAIRS, align.DEGENERATE) == (0, 1, 2)
    assert [int(x) for x in re.findall(r"#define SFB_(?:OK|FEW_PAIRS|DEGENERATE) (\d)", txt)] == [0, 1, 2]


def test_defaults_are_the_headers_and_pass_the_check():
    from staticfusion_amd import bodies

    p = bodies.default_params()
    got = (p.dist_max, p.z_max, p.normal_dz, p.damping, p.iterations, p.min_pairs)
    assert got == (np.float32(0.10), 8.0, np.float32(0.05), 0.0, 10, 64)
    assert bytes(p) == bytes(bodies.Params())
    keys = ("dist_max", "z_max", "normal_dz", "damping", "iterations", "min_pairs")
    assert got == tuple(np.float32(br.DEFAULTS[k]) if isinstance(br.DEFAULTS[k], float) else br.DEFAULTS[k] for k in keys)
    bodies.check_params(p)
    assert bodies._product().default_params(None) == -1
    assert re.search(r"parameter defaults, NOT tuned\s+\*?\s*values", open(HEADER).read())


def test_check_params_without_a_gpu():
    from staticfusion_amd import SfError, bodies

    b = bodies._product()
    assert b.check_params(None) == -1  # null: SF_ERR_ARG
    nan, inf = float("nan"), float("inf")
    good = [dict(dist_max=1.0), dict(dist_max=1e-6), dict(z_max=32.0), dict(z_max=1e-3), dict(normal_dz=32.0), dict(normal_dz=1e-6), dict(damping=0.0),
            dict(damping=1e30), dict(iterations=1), dict(iterations=64), dict(min_pairs=6), dict(min_pairs=2 ** 31 - 1)]
    for kw in good:
        bodies.check_params(bodies.Params(**kw))
    p = bodies.Params()
    p.reserved[0], p.reserved[1] = -12345, 7  # not read
    bodies.check_params(p)
    bad = [dict(dist_max=0.0), dict(dist_max=-0.1), dict(dist_max=1.0001), dict(dist_max=nan), dict(dist_max=inf), dict(z_max=0.0), dict(z_max=-1.0),
           dict(z_max=32.5), dict(z_max=nan), dict(z_max=inf), dict(normal_dz=0.0), dict(normal_dz=-0.01), dict(normal_dz=32.5), dict(normal_dz=nan),
           dict(normal_dz=inf), dict(damping=-1e-9), dict(damping=nan), dict(damping=inf), dict(damping=-inf), dict(iterations=0), dict(iterations=65),
           dict(iterations=-1), dict(min_pairs=5), dict(min_pairs=0), dict(min_pairs=-1)]
    for kw in bad:
        with pytest.raises(SfError, match="failed with -1"):
            bodies.check_params(bodies.Params(**kw))
