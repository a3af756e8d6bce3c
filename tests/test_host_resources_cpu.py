"""The owner of the host side's device blocks, pinned blocks, events and streams (staticfusion_amd/csrc/sf_resources.h), the
per-call block of the companion interfaces (sf_call_block.h) and the lifetime of what is created from a handle (sf_parts.h),
the checks that need no GPU: a stand-alone C++ program includes the real headers, defines the HIP functions they call itself
(malloc-backed, a set of live pointers, a log of calls, "fail the k-th acquiring call") and plays groups, growth, both rings,
the layout rule, a call block reused at three sizes with its two cleared ranges, a call-local owner, the release, and the parts
of two handles -- the handle first, the part first, a part never entered, a rebind, the shells destroyed -- through under the
address and undefined-behaviour sanitizers -- once clean, then once for every acquiring call failing (a child process: nothing
is loaded into python)."""
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
    assert m and int(m.group(1)) > 80 and not r.stderr  # the clean run and one run per acquiring call of it (61 before the parts)


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


def test_the_companion_host_sources_state_layout_block_and_refusals_once():
    """the 256-byte layout rule, the scratch block with its host copies and the shared refusals live in sf_call_block.h and
    sf_host.h: no companion file restates them, and the kernels of the stable partition are compiled into one object"""
    csrc = os.path.join(ROOT, "staticfusion_amd", "csrc")
    read = lambda name: open(os.path.join(csrc, name)).read()
    hips = [n for n in sorted(os.listdir(csrc)) if n.endswith(".hip")]
    for name in hips:
        src = read(name)
        assert not re.search(r"\btake\s*\(\s*size_t", src), name  # no struct with a take( member of its own
        assert not re.search(r"^\s*(static\s+|inline\s+)*[\w:<>]+[\s*&]+(finite_all|check_camera|indices_moved)\s*\([^;]*\)\s*\{", src, re.M), name
        assert not re.search(r"^enum\s+\w+\s*\{\s*FORM_STREAMS", src, re.M), name
        assert "namespace sfj_window" not in src and "sfj_window::" not in src and "sfp_window::" not in src, name
    for name in ("sf_join.h", "sf_body_maps.h"):
        assert "sf_map_window.h\"" not in read(name) and "sf_window_args.h\"" in read(name), name
    assert len(re.findall(r"\btake\s*\(\s*size_t", read("sf_call_block.h") + read("sf_host.h"))) == 1
    host = read("sf_host.h")
    body = host[host.index("struct sf_handle {"):host.index("// the surfel map")]
    members = re.findall(r"(\w+)\s*(?:=[^;,]*|\{\}|\[[^\]]*\])*\s*[;,]", re.sub(r"//.*", "", body))
    assert "seq_ring" in members and "view_counters_off" in members and len(members) > 60, members
    assert not [m for m in members if m.endswith("_scratch") or m.endswith("_args_host") or m.endswith("_tab_host")], members
    # (the two that remain are the solver's own: the shared argument table of sf_hip_model.hip and the staging of sf_hip_migrate.hip)
    assert sorted(m for m in members if m.endswith("_bytes")) == ["mig_stage_bytes", "tab_bytes"], members
    assert len(re.findall(r"\bSfCallBlock\s+\w+;", body)) == 7
    # the header is host only and includes nothing of the product but sf_resources.h
    assert re.findall(r'#include\s+"([^"]+)"', read("sf_call_block.h")) == ["sf_resources.h"]


def test_the_point_to_plane_system_the_wave_sum_and_the_voxel_table_are_stated_once():
    """the quantised row of the three point-to-plane solvers (sf_p2p_system.h), the shuffle sum over a wave (sf_device_common.h)
    and the voxel table (sf_voxel_table.h) have one statement each, in the product and in the restatements of tests/"""
    csrc = os.path.join(ROOT, "staticfusion_amd", "csrc")
    read = lambda name: open(os.path.join(csrc, name)).read()
    sources = [n for n in sorted(os.listdir(csrc)) if n.endswith((".hip", ".h", ".cpp"))]
    other_quantities = ("sf_score.h", "sf_regions.h", "sf_keyframes.h")  # grey, b and gradient sums at the same scales
    scales = [n for n in sources if n not in other_quantities and re.search(r"\b(4096|65536)\.0?f\b", read(n))]
    assert scales == ["sf_p2p_system.h", "sf_splat.h"], scales  # (sf_splat.h: the reciprocal of a division by multiplication)
    assert not re.search(r"rintf", read("sf_splat.h")) and len(re.findall(r"\b(?:4096|65536)\.0?f\b", read("sf_p2p_system.h"))) == 2
    assert [n for n in sources if re.search(r"\+=\s*__shfl_xor\(", read(n))] == ["sf_device_common.h"]
    for name in sources:  # no header is included inside a namespace: every #include stands outside all braces
        src = re.sub(r"//.*|\"(?:[^\"\\\n]|\\.)*\"", "", read(name))
        for m in re.finditer(r"^\s*#\s*include\b", src, re.M):
            assert src[:m.start()].count("{") == src[:m.start()].count("}"), name
    assert "sf_join.h" not in read("sf_register.h") and '#include "sf_voxel_table.h"' in read("sf_register.h")
    assert '#include "sf_voxel_table.h"' in read("sf_join.h")
    tests = os.path.join(ROOT, "tests")
    refs = [n for n in sorted(os.listdir(tests)) if n.endswith("_ref.py") and re.search(r"np\.rint\([^\n]*4096", open(os.path.join(tests, n)).read())]
    assert refs == ["align_ref.py", "keyframe_ref.py", "region_ref.py"], refs  # (the last two: the restatements of sf_keyframes.h and sf_regions.h)


def test_the_host_sources_state_the_lifetime_of_a_handles_parts_once():
    """what is created from a handle (maps, keyframe databases, trackers, deformation graphs, closure builders) is entered in
    one list of the handle and orphaned, destroyed and refused by one piece of code each (sf_parts.h, sf_host.h)"""
    csrc = os.path.join(ROOT, "staticfusion_amd", "csrc")
    read = lambda name: open(os.path.join(csrc, name)).read()
    sources = [n for n in sorted(os.listdir(csrc)) if n.endswith((".hip", ".h", ".cpp"))]
    for name in sources:
        if name.endswith(".hip"):  # no part has an orphan function of its own
            assert not re.search(r"^[\w\s*&:<>]*\borphan_\w*\s*\([^;{]*\)\s*(const\s*)?\{", read(name), re.M), name
    host = read("sf_host.h")
    body = host[host.index("struct sf_handle {"):host.index("// the surfel map")]
    members = re.findall(r"(\w+)\s*(?:=[^;,]*|\{\}|\[[^\]]*\])*\s*[;,]", re.sub(r"//.*", "", body))
    assert re.findall(r"\bSfParts\s+(\w+);", body) == ["parts"] and "parts" in members
    assert not [m for m in members if m in ("maps", "keyframe_dbs", "trackers", "graphs", "builders")], members
    assert not re.search(r"std::vector<\s*(struct\s+)?(sf_map|sfk_db|sft_tracker|sfd_graph|sfc_builder)\s*\*", body)
    # the two refusals of a part and the refusal of a handle that is gone are made in check_part and check_live_handle alone
    text = "has been destroyed"
    for fn, count in (("check_part", 1), ("check_live_handle", 1)):
        m = re.search(r"static inline int %s\(.*?\n}\n" % fn, host, re.S)
        assert m and m.group(0).count(text) == count, fn
        host = host.replace(m.group(0), "")
    for name in sources:
        assert text not in (host if name == "sf_host.h" else read(name)), name
    # the header is host only and includes nothing of the product but sf_call_block.h / sf_resources.h
    assert set(re.findall(r'#include\s+"([^"]+)"', read("sf_parts.h"))) <= {"sf_call_block.h", "sf_resources.h"}
    assert not re.search(r"__global__|__device__|hip_runtime\.h", read("sf_parts.h"))
