"""The greedy assignment of the region tracks (staticfusion_amd/csrc/sf_track_assign.h), a check that needs no GPU: a
stand-alone C++ program includes the real header -- the text the assign kernel and the pure-host sft_assign compile -- and runs
it on the hand tables of include/sf_tracks.h, on every K_prev, K in {0, 1, 2, 255, 256} and on 3000 random tables against a plain
statement of the rule, counting the rounds, under the address and undefined-behaviour sanitizers (a child process: nothing is
loaded into python)."""
import os
import re
import subprocess

from conftest import ROOT
from staticfusion_amd import tracks


def test_the_assignment_on_the_host_under_the_sanitizers(tmp_path):
    assert tracks.VERSION == 1
    exe = str(tmp_path / "track_assign_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall",
                           "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "track_assign_host.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode())
    m = re.match(r"ok (\d+)\n", r.stdout.decode())
    assert m and int(m.group(1)) > 9000 and not r.stderr
