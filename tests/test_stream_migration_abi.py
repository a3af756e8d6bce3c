"""Stream migration (include/sf_migrate.h), the checks that need no GPU: the header, the ctypes table of
staticfusion_amd/streams.py and the library's exports name the same functions -- none of them part of include/sf.h --, the
blob size is the sum of the documented segments, and the host arithmetic (blob layout, ring rotation) holds in a stand-alone
C++ program under the address and undefined-behaviour sanitizers (a child process: nothing is loaded into python)."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "sf_migrate.h")


def declared():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)  # declarations only: the comments name the functions too
    return sorted(set(re.findall(r"\b(sfm_\w+)\s*\(", txt)))


def test_header_table_and_exports_name_the_same_functions():
    import staticfusion_amd as sf
    from staticfusion_amd import capi, streams

    names = declared()
    assert len(names) == 7 and "sfm_copy_streams" in names
    assert names == sorted(streams.SIGNATURES.keys())
    out = subprocess.check_output(["nm", "-D", "--defined-only", sf.LIB]).decode()
    assert sorted(set(re.findall(r" T (sfm_\w+)", out))) == names
    # a companion of the ABI, not a part of it: sf.h declares none of them, its table has none, the version stands
    sf_h = open(os.path.join(ROOT, "include", "sf.h")).read()
    assert "sfm_" not in sf_h and "SF_FN" not in open(HEADER).read()
    assert not any(k.startswith("sfm") or ("sfm_" + k) in names for k in capi.SIGNATURES)
    # the precise and reference-order libraries link the same host objects
    for other in ("libsf_hip_precise.so", "libsf_hip_reforder.so"):
        path = os.path.join(os.path.dirname(sf.LIB), other)
        if os.path.exists(path):
            o = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
            assert sorted(set(re.findall(r" T (sfm_\w+)", o))) == names, other
    # both bindings share one loaded copy of the library
    assert streams._product().api.lib is sf.load().lib
    assert streams.version() == 1


def documented_blob_bytes(rows, cols, levels, with_input):
    """include/sf_migrate.h, BLOB: header, then the segments, each padded to a multiple of 16 bytes"""
    import staticfusion_amd as sf

    pad = lambda b: (b + 15) // 16 * 16
    n0 = rows * cols
    n_tot = sum((rows >> L) * (cols >> L) for L in range(levels))
    segs = [347 * 4, ctypes.sizeof(sf.SfFrameStats)] + [4 * n_tot] * 4 + [n_tot, 4 * n0] + [4 * n0] * 5 + [4 * n0] * 5
    if with_input:
        segs += [2 * n0, 2 * n0, 4 * n0, 3 * n0]
    return 64 + sum(pad(b) for b in segs)


@pytest.mark.parametrize("rows,cols,levels,with_input", [(60, 80, 3, 0), (60, 80, 3, 1), (40, 42, 3, 0), (18, 22, 1, 0)])
def test_blob_bytes_is_the_sum_of_the_documented_segments(rows, cols, levels, with_input):
    from staticfusion_amd import streams

    assert streams.blob_bytes(rows, cols, levels, with_input) == documented_blob_bytes(rows, cols, levels, with_input)
    assert streams.blob_bytes(rows, cols, levels, with_input) % 16 == 0


def test_blob_bytes_of_no_geometry_is_zero():
    from staticfusion_amd import streams

    assert streams.blob_bytes(4, 4, 1, 0) == 0 and streams.blob_bytes(60, 80, 0, 0) == 0 and streams.blob_bytes(60, 80, 9, 1) == 0


def test_layout_and_ring_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "migrate_layout")
    # (the sanitizer runtimes linked statically: the program then is the same in whatever environment it is started)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "migrate_layout.cpp"), "-o", exe])
    needed = subprocess.check_output(["readelf", "-d", exe]).decode()
    assert "amdhip" not in needed and "libsf_hip" not in needed  # stand-alone: no HIP runtime, no product library
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode())
    assert re.match(r"ok \d+\n", r.stdout.decode()) and not r.stderr
