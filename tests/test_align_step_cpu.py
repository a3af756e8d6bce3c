"""The step of the pose refinement (staticfusion_amd/csrc/sf_align_step.h), a check that needs no GPU: a stand-alone C++
program includes the real header -- the text the step kernel and sfa_step compile -- and runs it on an empty system, on sums at
their bounds, on every refusal and on 2000 random systems whose solves it holds to their residual, under the address and
undefined-behaviour sanitizers (a child process: nothing is loaded into python)."""
import os
import re
import subprocess

from conftest import ROOT
from staticfusion_amd import align


def test_the_step_on_the_host_under_the_sanitizers(tmp_path):
    assert align.VERSION == 1
    exe = str(tmp_path / "align_step_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "align_step_host.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode())
    m = re.match(r"ok (\d+)\n", r.stdout.decode())
    assert m and int(m.group(1)) > 6000 and not r.stderr
