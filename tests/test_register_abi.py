"""The map registration (include/sf_register.h), the checks that need no GPU: the header, the ctypes table of
staticfusion_amd/register.py and the exports of the three libraries name the same functions -- none of them part of include/sf.h,
whose version has not moved, like those of the other companions --, nothing of the parts' lifetime or of the shared rule text is
exported, no other header, binding or oracle source names them, the structs have the documented sizes, offsets and field order,
and the defaults are the header's."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import register_cases as rc
import register_ref as rr
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "sf_register.h")


def declared():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)  # declarations only: the comments name the functions too
    return sorted(set(re.findall(r"\b(sfg_\w+)\s*\(", txt)))


def test_header_table_and_exports_name_the_same_functions():
    import staticfusion_amd as sf
    from staticfusion_amd import align, bodies, body_maps, capi, carve, closure, deform, join, keyframes, map_window, regions, register, score, streams, tracks, view

    names = declared()
    assert names == ["sfg_check_params", "sfg_default_params", "sfg_linearise", "sfg_params_bytes", "sfg_register_maps", "sfg_registrar_create",
                     "sfg_registrar_destroy", "sfg_result_bytes", "sfg_system_bytes", "sfg_version"]
    assert names == sorted(register.SIGNATURES.keys())
    for lib in ("libsf_hip.so", "libsf_hip_precise.so", "libsf_hip_reforder.so"):  # the three link the same host objects
        path = os.path.join(os.path.dirname(sf.LIB), lib)
        assert os.path.exists(path), lib
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert sorted(set(re.findall(r" T (sfg_\w+)", out))) == names, lib
        for word in ("sfg_pair_core", "sfg_representative", "sfg_fill_host", "sfg_linearise_host", "sfg_accumulate", "sfg_unit", "sfa_step_core"):
            assert word not in out, "the shared text is not exported"
        assert not re.search(r"SfPart|shelled|orphan_all|part_destroy|check_part|check_live_handle|_ZT[VIS]\d+sfg_registrar", out), lib
    # a companion of the ABI, not a part of it; no other header or binding names sfg_*, and this header names none of the
    # prefixes the other ABI tests search every header for, nor the oracle's
    for path in glob.glob(os.path.join(ROOT, "include", "*")):
        if os.path.basename(path) != "sf_register.h":
            assert "sfg_" not in open(path).read(), path
    txt = open(HEADER).read()
    for prefix in ("sfa_", "sfb_", "sfc_", "sfd_", "sfe_", "sfj_", "sfk_", "sfm_", "sfp_", "sfr_", "sfs_", "sft_", "sfv_", "sfw_", "sfo_", "SF_FN"):
        assert prefix not in txt, prefix
    assert re.findall(r'#include\s+"([^"]+)"', txt) == ["sf.h"]
    assert re.search(r"#define\s+SF_ABI_VERSION\s+5\b", open(os.path.join(ROOT, "include", "sf.h")).read())
    assert not any(k.startswith("sfg") or "register" in k for k in capi.SIGNATURES)  # (the names of sf.h without "sf_")
    others = (align, bodies, body_maps, carve, closure, deform, join, keyframes, map_window, regions, score, streams, tracks, view)
    for other in others:
        assert not any(k.startswith("sfg_") for k in other.SIGNATURES), other.__name__
    assert tuple(o.version() for o in others) == (1,) * 14
    assert register.version() == 1 == register.VERSION
    assert register._product().api.lib is sf.load().lib and register._product().api.lib is join._product().api.lib  # one loaded copy
    for path in glob.glob(os.path.join(ROOT, "oracle", "*")):  # the oracle's sources do not have the prefix
        if os.path.isfile(path) and not path.endswith(".so"):
            assert "sfg_" not in open(path, errors="replace").read(), path
    # the constants of the header are the binding's and the restatement's
    consts = dict(re.findall(r"#define\s+(SFG_\w+)\s+(\d+)", txt))
    for k in ("OK", "FEW_PAIRS", "DEGENERATE"):
        assert int(consts["SFG_" + k]) == getattr(register, k) == getattr(rr, k)
    assert (register.NOT_PAIRED, register.NOT_SAMPLED) == (rr.NOT_PAIRED, rr.NOT_SAMPLED) == (-1, -2)
    # the header states its rules, its refusals and what it leaves out, and names the other interfaces by file
    for word in ("TABLE", "ESTIMATE", "SAMPLE", "PAIR", "LOOP", "WHY THIS RULE", "REFUSALS", "OUT OF SCOPE", "sf_join.h", "sf_align.h", "sf_deform.h",
                 "sf_body_maps.h", "REPRESENTATIVE", "2 x 2 x 2", "dist_max <= 0.5f * cell", "strictly", "colour terms", "robust weights beyond the gates",
                 "a global search", "multi-resolution", "writing T into a map, a stream or a merge", "a device-pointer form", "symmetric pairing"):
        assert word in txt, word
    # one part more, named where the parts are named
    csrc = os.path.join(ROOT, "staticfusion_amd", "csrc")
    assert re.search(r"^HOST_PARTS\s*\+=\s*register$", open(os.path.join(csrc, "Makefile")).read(), re.M)
    assert "sfg_*" in open(os.path.join(csrc, "sf_call_block.h")).read() and "sfg_registrar" in open(os.path.join(csrc, "sf_parts.h")).read()
    assert "sf_hip_register.hip" in open(os.path.join(csrc, "sf_host.h")).read()
    # the rule text includes nothing of the library beyond the key of the join and the system; the step is included, not restated
    rules = open(os.path.join(csrc, "sf_register_rules.h")).read()
    assert re.findall(r'#include\s+"([^"]+)"', rules) == ["sf_join_key.h", "sf_p2p_system.h"] and "__global__" not in rules
    system = open(os.path.join(csrc, "sf_p2p_system.h")).read()
    assert not re.findall(r'#include\s+"([^"]+)"', system) and "__global__" not in system
    device = open(os.path.join(csrc, "sf_register.h")).read()
    shared = open(os.path.join(csrc, "sf_p2p_device.h")).read()  # the state, the reduction and the step's bookkeeping of the three solvers
    assert '#include "sf_p2p_device.h"' in device and '#include "sf_align_step.h"' in shared and "sfa_step_core(" in shared
    assert "LDL" not in device + shared and "atomicAdd(float" not in device + shared
    sources = device + open(os.path.join(csrc, "sf_hip_register.hip")).read()
    # the insert kernel is the voxel table's
    assert "compare_exchange" not in sources and '#include "sf_voxel_table.h"' in device and "sf_join.h" not in device and "sfj_insert_kernel<true>" in sources
    assert "compare_exchange" in open(os.path.join(csrc, "sf_voxel_table.h")).read() and "compare_exchange" not in open(os.path.join(csrc, "sf_join.h")).read()


def test_the_oracle_binding_is_refused(ora):
    from staticfusion_amd import SfError, register

    with pytest.raises(SfError):
        register._bind(ora)


def test_struct_sizes_and_layouts():
    from staticfusion_amd import register

    b = register._product()
    assert b.params_bytes() == C.sizeof(register.SfgParams) == 32
    assert b.system_bytes() == register.SYSTEM_DTYPE.itemsize == 256 and register.SYSTEM_DTYPE == rr.SYSTEM_DTYPE
    assert b.result_bytes() == register.RESULT_DTYPE.itemsize == 128
    param_names = ("cell", "dist_max", "min_cos", "min_confidence", "damping", "iterations", "stride", "min_pairs")
    assert [getattr(register.SfgParams, k).offset for k in param_names] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert list(param_names) == [k for k, _ in register.SfgParams._fields_]
    layouts = {"sfg_params": (param_names, None),
               "sfg_system": (("n", "ss", "g", "H", "reserved"), (register.SYSTEM_DTYPE, [0, 8, 16, 64, 232])),
               "sfg_result": (("T", "status", "iterations_done", "n_first", "ss_first", "n_last", "ss_last", "n_sampled", "n_outside", "reserved"),
                              (register.RESULT_DTYPE, [0, 64, 68, 72, 80, 88, 96, 104, 108, 112]))}
    txt = open(HEADER).read()
    for struct, (names, dtype) in layouts.items():
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), txt, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body) == list(names), struct
        if dtype:
            assert list(dtype[0].names) == list(names) and [dtype[0].fields[k][1] for k in names] == dtype[1], struct


def test_defaults_are_the_headers_and_pass_the_checks():
    from staticfusion_amd import register

    p = register.default_params()
    keys = ("cell", "dist_max", "min_cos", "min_confidence", "damping", "iterations", "stride", "min_pairs")
    assert tuple(getattr(p, k) for k in keys) == (np.float32(0.1), np.float32(0.05), 0.5, 0.0, 0.0, 10, 1, 64)
    assert bytes(p) == bytes(register.Params()) == bytes(rc.as_product(rr.Params()))
    assert sorted(rr.DEFAULTS) == sorted(keys) and all(np.float32(getattr(p, k)) == np.float32(rr.DEFAULTS[k]) for k in keys)
    register.check_params(p)
    assert register._product().default_params(None) == -1
    txt = open(HEADER).read()
    assert len(re.findall(r"parameter defaults, NOT tuned values", txt)) == 1
    assert "cell 0.1, dist_max 0.05, min_cos 0.5, min_confidence 0, damping 0, iterations 10, stride 1, min_pairs 64." in txt


def test_a_shell_call_without_a_gpu_refuses_nulls():
    from staticfusion_amd import register

    b = register._product()
    res = np.full(128, 0xAB, np.uint8)
    assert b.register_maps(None, 1, None, None, None, None, res.ctypes.data, None, None) == -1 and (res == 0xAB).all()  # a null registrar
    assert b.registrar_create(None, None) == -1
    b.registrar_destroy(None)
