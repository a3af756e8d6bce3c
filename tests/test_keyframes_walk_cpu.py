"""The item walk of the keyframe encode kernel (staticfusion_amd/csrc/sf_keyframe_walk.h), a check that needs no GPU: a
stand-alone C++ program includes the real header and holds the walk to the divisions it replaces, for every geometry of the
GPU tests and the extremes of the legal range, under the address and undefined-behaviour sanitizers (a child process: nothing
is loaded into python). Every address the kernel loads from comes from this walk."""
import os
import re
import subprocess

from conftest import ROOT
from staticfusion_amd import keyframes


def test_the_walk_visits_exactly_the_items_the_divisions_give(tmp_path):
    assert keyframes.VERSION == 1
    exe = str(tmp_path / "keyframe_walk_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "keyframe_walk_host.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode())
    m = re.match(r"ok (\d+)\n", r.stdout.decode())
    assert m and int(m.group(1)) > 10 ** 7 and not r.stderr
