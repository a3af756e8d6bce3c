"""The world motion of the region motions (staticfusion_amd/csrc/sf_body_world.h), a check that needs no GPU: a stand-alone C++
program includes the real header -- the text the step kernel and the pure-host sfb_world_motion compile -- and runs it on hand
cases and on 2000 random rigid triples against a plain matrix product, with guards behind the output arrays, under the address
and undefined-behaviour sanitizers (a child process: nothing is loaded into python)."""
import os
import re
import subprocess

from conftest import ROOT
from staticfusion_amd import bodies


def test_the_world_motion_on_the_host_under_the_sanitizers(tmp_path):
    assert bodies.VERSION == 1
    exe = str(tmp_path / "body_world_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "body_world_host.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode())
    m = re.match(r"ok (\d+)\n", r.stdout.decode())
    assert m and int(m.group(1)) > 8000 and not r.stderr
