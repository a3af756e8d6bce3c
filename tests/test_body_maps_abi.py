"""Body maps (include/sf_body_maps.h), the checks that need no GPU: the header, the ctypes table of staticfusion_amd/body_maps.py
and the exports of the three libraries name the same functions -- none of them part of include/sf.h, whose version has not moved,
like those of the other companions --, no other header or binding names them, the header spells no other companion's prefix, the
structs have the documented sizes, offsets and field order (the camera those of the tracks header), the defaults are the header's,
and the pure-host parameter check refuses every case of the header's list."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import body_map_ref as pr
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "sf_body_maps.h")


def declared():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)  # declarations only: the comments name the functions too
    return sorted(set(re.findall(r"\b(sfp_\w+)\s*\(", txt)))


def test_header_table_and_exports_name_the_same_functions():
    import staticfusion_amd as sf
    from staticfusion_amd import align, bodies, body_maps, capi, join, keyframes, map_window, regions, score, streams, tracks, view

    names = declared()
    assert len(names) == 11 and {"sfp_fuse_images", "sfp_fuse_images_device", "sfp_move_maps", "sfp_pixel_surfel", "sfp_merge_surfel"} <= set(names)
    assert names == sorted(body_maps.SIGNATURES.keys())
    for lib in ("libsf_hip.so", "libsf_hip_precise.so", "libsf_hip_reforder.so"):  # the three link the same host objects
        path = os.path.join(os.path.dirname(sf.LIB), lib)
        assert os.path.exists(path), lib
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert sorted(set(re.findall(r" T (sfp_\w+)", out))) == names, lib
        assert "sfp_pixel_surfel_core" not in out and "sfp_merge_core" not in out and "handle_alive" not in out, "the shared text and the handle list are not exported"
    # a companion of the ABI, not a part of it; no other header or binding names sfp_*, and this header names none of the
    # prefixes the other ABI tests search every header for, nor the oracle's
    for path in glob.glob(os.path.join(ROOT, "include", "*")):
        if os.path.basename(path) != "sf_body_maps.h":
            assert "sfp_" not in open(path).read(), path
    txt = open(HEADER).read()
    assert not any(p in txt for p in ("sft_", "sfa_", "sfj_", "sfb_", "sfo_", "SF_FN"))
    assert '#include "sf_bodies.h"' in txt and '#include "sf_join.h"' in txt
    assert re.search(r"#define\s+SF_ABI_VERSION\s+5\b", open(os.path.join(ROOT, "include", "sf.h")).read())
    assert not any(k.startswith("sfp") or "body_map" in k for k in capi.SIGNATURES)  # (the names of sf.h without "sf_")
    others = (align, bodies, join, keyframes, map_window, regions, score, streams, tracks, view)
    for other in others:
        assert not any(k.startswith("sfp_") for k in other.SIGNATURES), other.__name__
    assert tuple(o.version() for o in others) == (1,) * 10
    assert body_maps.version() == 1 == body_maps.VERSION
    assert body_maps._product().api.lib is sf.load().lib and body_maps._product().api.lib is join._product().api.lib  # one loaded copy
    # the oracle's sources do not have the prefix
    for path in glob.glob(os.path.join(ROOT, "oracle", "*")):
        if os.path.isfile(path) and not path.endswith(".so"):
            assert "sfp_" not in open(path, errors="replace").read(), path


def test_the_oracle_binding_is_refused(ora):
    from staticfusion_amd import SfError, body_maps

    with pytest.raises(SfError):
        body_maps._bind(ora)


def test_struct_sizes_and_layouts():
    from staticfusion_amd import body_maps, tracks

    b = body_maps._product()
    assert b.params_bytes() == C.sizeof(body_maps.SfpParams) == 32
    assert b.counts_bytes() == C.sizeof(body_maps.SfpCounts) == 32
    assert b.camera_bytes() == C.sizeof(body_maps.SfpCamera) == tracks._product().camera_bytes() == 80
    param_names = ("cell", "z_max", "normal_dz", "min_dot", "conf_new", "gain", "max_weight", "reserved")
    assert [getattr(body_maps.SfpParams, k).offset for k in param_names] == [0, 4, 8, 12, 16, 20, 24, 28]
    count_names = ("n_pixels", "n_candidates", "n_voxels", "n_merged", "n_added", "n_conflict", "n_out", "reserved")
    assert [getattr(body_maps.SfpCounts, k).offset for k in count_names] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert body_maps.COUNT_FIELDS == count_names[:-1] == pr.COUNT_FIELDS
    assert [getattr(body_maps.SfpCamera, k).offset for k in ("pose", "cx", "cy", "fx", "fy")] == [0, 64, 68, 72, 76]
    txt = open(HEADER).read()

    def fields(header_text, struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header_text, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)

    assert fields(txt, "sfp_params") == list(param_names) == [k for k, _ in body_maps.SfpParams._fields_]
    assert fields(txt, "sfp_counts") == list(count_names) == [k for k, _ in body_maps.SfpCounts._fields_]
    assert fields(txt, "sfp_camera") == fields(open(os.path.join(ROOT, "include", "sf_tracks.h")).read(), "sft_camera") == [k for k, _ in tracks.SftCamera._fields_]


def test_defaults_are_the_headers_and_pass_the_check():
    from staticfusion_amd import body_maps

    p = body_maps.default_params()
    keys = ("cell", "z_max", "normal_dz", "min_dot", "conf_new", "gain", "max_weight")
    got = tuple(getattr(p, k) for k in keys)
    assert got == tuple(np.float32(x) for x in (0.01, 8, 0.05, 0.8, 0.1, 0.25, 32)) and p.reserved == 0
    assert bytes(p) == bytes(body_maps.Params())
    assert got == tuple(np.float32(pr.DEFAULTS[k]) for k in keys)
    body_maps.check_params(p)
    assert body_maps._product().default_params(None) == -1
    txt = open(HEADER).read()
    assert re.search(r"parameter defaults, NOT\s+\*?\s*tuned values", txt) or re.search(r"parameter defaults, NOT tuned\s+\*?\s*values", txt)
    assert re.search(r"cell 0\.01, z_max 8, normal_dz 0\.05, min_dot 0\.8, conf_new 0\.1, gain 0\.25, max_weight 32\.", txt)


def test_check_params_without_a_gpu():
    from staticfusion_amd import SfError, body_maps

    b = body_maps._product()
    assert b.check_params(None) == -1  # null: SF_ERR_ARG
    nan, inf = float("nan"), float("inf")
    good = [dict(cell=1e-6), dict(cell=1e6), dict(z_max=32.0), dict(z_max=1e-3), dict(normal_dz=32.0), dict(normal_dz=1e-6), dict(min_dot=-1.0), dict(min_dot=1.0),
            dict(min_dot=0.0), dict(conf_new=0.0), dict(conf_new=1.0), dict(gain=1.0), dict(gain=1e-6), dict(max_weight=1.0), dict(max_weight=1e30)]
    for kw in good:
        body_maps.check_params(body_maps.Params(**kw))
    p = body_maps.Params()
    p.reserved = -12345  # not read
    body_maps.check_params(p)
    bad = []
    for k in ("cell", "z_max", "normal_dz", "min_dot", "conf_new", "gain", "max_weight"):
        bad += [{k: nan}, {k: inf}, {k: -inf}]
    bad += [dict(cell=0.0), dict(cell=-0.01), dict(cell=1e-45), dict(z_max=0.0), dict(z_max=-1.0), dict(z_max=32.5), dict(normal_dz=0.0), dict(normal_dz=-0.01),
            dict(normal_dz=32.5), dict(min_dot=-1.0001), dict(min_dot=1.0001), dict(conf_new=-1e-9), dict(conf_new=1.0001), dict(gain=0.0), dict(gain=-0.1),
            dict(gain=1.0001), dict(max_weight=0.999), dict(max_weight=0.0), dict(max_weight=-1.0)]
    for kw in bad:
        with pytest.raises(SfError, match="failed with -1"):
            body_maps.check_params(body_maps.Params(**kw))
