"""The index arithmetic of the region kernels (staticfusion_amd/csrc/sf_region_walk.h), a check that needs no GPU: a
stand-alone C++ program includes the real header and holds tiles, border items and the lanes' pixel counters to the plain
divisions they replace, for every shape of the GPU tests and the extremes of the legal range, under the address and
undefined-behaviour sanitizers (a child process: nothing is loaded into python). Every address the kernels form comes from
these values."""
import os
import re
import subprocess

from conftest import ROOT
from staticfusion_amd import regions


def test_tiles_border_items_and_runs_equal_the_divisions(tmp_path):
    assert regions.VERSION == 1
    exe = str(tmp_path / "region_walk_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "region_walk_host.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode())
    m = re.match(r"ok (\d+)\n", r.stdout.decode())
    assert m and int(m.group(1)) > 10 ** 6 and not r.stderr
