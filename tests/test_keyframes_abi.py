"""Place recognition (include/sf_keyframes.h), the checks that need no GPU: the header, the ctypes table of
staticfusion_amd/keyframes.py and the exports of the three libraries name the same functions -- none of them part of
include/sf.h, whose version has not moved, like those of the other companions --, the three structs have the documented
sizes, the default ferns are the reference's generator, and the pure-host fern check refuses every case of the header's list."""
import os
import re
import subprocess

import numpy as np
import pytest

import keyframe_ref as kr
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "sf_keyframes.h")


def declared():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)  # declarations only: the comments name the functions too
    return sorted(set(re.findall(r"\b(sfk_\w+)\s*\(", txt)))


def test_header_table_and_exports_name_the_same_functions():
    import staticfusion_amd as sf
    from staticfusion_amd import capi, keyframes, map_window, score, streams, view

    names = declared()
    assert len(names) == 19 and "sfk_query_streams" in names and "sfk_encode_images_device" in names and "sfk_db_set" in names
    assert names == sorted(keyframes.SIGNATURES.keys())
    for lib in ("libsf_hip.so", "libsf_hip_precise.so", "libsf_hip_reforder.so"):  # the three link the same host objects
        path = os.path.join(os.path.dirname(sf.LIB), lib)
        assert os.path.exists(path), lib
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert sorted(set(re.findall(r" T (sfk_\w+)", out))) == names, lib
        assert "orphan_keyframe_dbs" not in out, "what sf_destroy calls is not exported"
        # ... nor what does that work now: the base of the parts with its hook, the handle's list of them, the shared destroy and refusals
        assert not re.search(r"SfPart|shelled|orphan_all|part_destroy|check_part|check_live_handle|_ZT[VIS]\d+sfk_db", out), lib
    # a companion of the ABI, not a part of it
    sf_h = open(os.path.join(ROOT, "include", "sf.h")).read()
    assert "sfk_" not in sf_h and "SF_FN" not in open(HEADER).read()
    assert re.search(r"#define\s+SF_ABI_VERSION\s+5\b", sf_h)
    assert not any(k.startswith("sfk") or "keyframe" in k or "fern" in k for k in capi.SIGNATURES)  # (its keys are the names of sf.h without "sf_")
    for other in (view, score, map_window, streams):
        assert not any(k.startswith("sfk_") for k in other.SIGNATURES)
        assert other.version() == 1
    assert keyframes.version() == 1 == keyframes.VERSION
    assert keyframes._product().api.lib is sf.load().lib and keyframes._product().api.lib is score._product().api.lib  # one loaded copy


def test_the_oracle_binding_is_refused(ora):
    from staticfusion_amd import SfError, keyframes

    with pytest.raises(SfError):
        keyframes._bind(ora)


def test_struct_sizes():
    from staticfusion_amd import keyframes

    b = keyframes._product()
    assert b.fern_bytes() == keyframes.FERN_DTYPE.itemsize == 16
    assert b.match_bytes() == keyframes.MATCH_DTYPE.itemsize == 8
    assert b.info_bytes() == keyframes.INFO_DTYPE.itemsize == 48
    assert keyframes.INFO_DTYPE.names[:9] == keyframes.INFO_FIELDS and all(keyframes.INFO_DTYPE.fields[k][1] == 4 * q for q, k in enumerate(keyframes.INFO_FIELDS))


@pytest.mark.parametrize("n_ferns", [1, 8, 9, 513])
def test_default_ferns_equal_the_reference_generator(n_ferns):
    from staticfusion_amd import keyframes

    for seed, n_cells in ((20261020, 192), (0, 1), ((1 << 64) - 1, 4096), (7, 35)):
        got = keyframes.default_ferns(n_ferns, seed, n_cells)
        want = kr.default_ferns(n_ferns, seed, n_cells)
        assert got.shape == (n_ferns,) and got.tobytes() == want.tobytes(), (seed, n_cells)
        keyframes.check_ferns(got, n_cells)  # what the generator makes is in range


def test_default_ferns_write_exactly_n_records_and_refuse_bad_counts():
    from staticfusion_amd import keyframes

    b = keyframes._product()
    buf = np.full(10, -77, keyframes.FERN_DTYPE)
    assert b.default_ferns(9, 5, 12, buf.ctypes.data) == 0
    assert buf[:9].tobytes() == kr.default_ferns(9, 5, 12).tobytes() and buf[9].tolist() == (-77, -77, -77, -77)
    before = buf.tobytes()
    for args in ((0, 5, 12), (-1, 5, 12), (4097, 5, 12), (9, 5, 0), (9, 5, -3), (9, 5, 4097)):
        assert b.default_ferns(args[0], args[1], args[2], buf.ctypes.data) == -1, args
    assert b.default_ferns(9, 5, 12, None) == -1 and buf.tobytes() == before


def test_check_ferns_without_a_gpu():
    from staticfusion_amd import SfError, keyframes

    good = kr.default_ferns(9, 3, 12)
    keyframes.check_ferns(good, 12)
    edge = good.copy()
    edge[0] = (11, 4096, 32768, 123)  # the bounds themselves are legal; reserved is not read
    edge[1] = (0, 0, 0, -1)
    keyframes.check_ferns(edge, 12)
    b = keyframes._product()
    for field, value in (("cell", -1), ("cell", 12), ("t_grey", -1), ("t_grey", 4097), ("t_depth", -1), ("t_depth", 32769)):
        for at in (0, 8):
            bad = good.copy()
            bad[field][at] = value
            with pytest.raises(SfError, match="failed with -1"):
                keyframes.check_ferns(bad, 12)
    assert b.check_ferns(None, 9, 12) == -1  # null: SF_ERR_ARG
    for n_ferns, n_cells in ((0, 12), (-1, 12), (4097, 12), (9, 0), (9, -1), (9, 4097)):
        big = np.zeros(max(n_ferns, 1), keyframes.FERN_DTYPE)
        assert b.check_ferns(big.ctypes.data, n_ferns, n_cells) == -1, (n_ferns, n_cells)
    assert b.check_ferns(np.zeros(4096, keyframes.FERN_DTYPE).ctypes.data, 4096, 4096) == 0
