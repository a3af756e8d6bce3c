"""The key, the rank and the hash of the joined maps (staticfusion_amd/csrc/sf_join_key.h), a check that needs no GPU: a
stand-alone C++ program includes the real header -- the text the kernels and the pure-host functions compile -- and runs it on
the special values of include/sf_join.h, on keys at both ends of the range and on 200 000 random positions, under the address and
undefined-behaviour sanitizers (a child process: nothing is loaded into python)."""
import os
import re
import subprocess

from conftest import ROOT
from staticfusion_amd import join


def test_the_key_on_the_host_under_the_sanitizers(tmp_path):
    assert join.VERSION == 1
    exe = str(tmp_path / "join_key_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "join_key_host.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode())
    m = re.match(r"ok (\d+)\n", r.stdout.decode())
    assert m and int(m.group(1)) > 200000 and not r.stderr
