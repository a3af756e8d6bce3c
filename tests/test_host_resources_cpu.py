"""The owner of the host side's device blocks, pinned blocks, events and streams (staticfusion_amd/csrc/sf_resources.h), the
checks that need no GPU: a stand-alone C++ program includes the real header, defines the HIP functions it calls itself
(malloc-backed, a set of live pointers, a log of calls, "fail the k-th acquiring call") and plays groups, growth, both rings,
a call-local owner and the release through under the address and undefined-behaviour sanitizers -- once clean, then once for
every acquiring call failing (a child process: nothing is loaded into python)."""
import os
import re
import subprocess

from conftest import ROOT


def test_owner_growth_and_rings_under_sanitizers(tmp_path):
    exe = str(tmp_path / "resources_host")
    # (the sanitizer runtimes linked statically: the program then is the same in whatever environment it is started)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "resources_host.cpp"), "-o", exe])
    needed = subprocess.check_output(["readelf", "-d", exe]).decode()
    assert "amdhip" not in needed and "libsf_hip" not in needed  # stand-alone: no HIP runtime, no product library
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode())
    m = re.match(r"ok (\d+)\n", r.stdout.decode())
    assert m and int(m.group(1)) > 40 and not r.stderr  # the clean run and one run per acquiring call of it


def test_the_host_sources_acquire_and_release_in_one_place():
    """outside sf_resources.h only the caller-owned pinned blocks and the process-wide cluster events name HIP's calls"""
    csrc = os.path.join(ROOT, "staticfusion_amd", "csrc")
    pat = re.compile(r"hip(Malloc|Free|HostMalloc|HostFree|EventCreate|EventDestroy|StreamCreate|StreamDestroy)")
    hits = []
    for name in sorted(os.listdir(csrc)):
        if name.endswith(".hip") or name == "sf_host.h":
            for line in open(os.path.join(csrc, name)):
                if pat.search(line):
                    hits.append((name, line.strip()))
    assert [n for n, _ in hits] == ["sf_hip.hip", "sf_hip_solver.hip", "sf_hip_solver.hip"], hits
    assert "hipEventCreateWithFlags(&ev, hipEventDisableTiming)" in hits[0][1]  # launch(): the event of g_cluster_done[device]
    assert "hipHostMalloc(out" in hits[1][1] and "hipHostFree(p)" in hits[2][1]  # sf_alloc_pinned, sf_free_pinned
