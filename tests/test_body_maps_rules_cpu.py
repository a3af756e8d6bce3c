"""The per-surfel rules of the body maps (staticfusion_amd/csrc/sf_body_map_rules.h), checks that need no GPU. A stand-alone C++
program includes the real header -- the text the kernels and the pure-host sfp_pixel_surfel / sfp_merge_surfel compile -- and runs
it on hand cases and random cases with guards behind the outputs, under the address and undefined-behaviour sanitizers (a child
process: nothing is loaded into python). And the two pure-host functions of the library agree with tests/body_map_ref.py bit
for bit, NaN and inf depths and normal_dz met and one ulp beyond included."""
import os
import re
import subprocess

import numpy as np

import body_map_cases as pc
import body_map_ref as pr
from conftest import ROOT

F = np.float32


def test_the_rules_on_the_host_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "body_map_rules_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "body_map_rules_host.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode())
    m = re.match(r"ok (\d+)\n", r.stdout.decode())
    assert m and int(m.group(1)) > 20000 and not r.stderr


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a, F), np.asarray(b, F)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def lib_camera(cam):
    from staticfusion_amd import body_maps

    return body_maps.Camera(cam["pose"], cam["cx"], cam["cy"], cam["fx"], cam["fy"])


def test_pixel_surfel_equals_the_restatement_bit_for_bit():
    from staticfusion_amd import body_maps

    rng = np.random.default_rng(11)
    T = pc.bc.pose((0.3, -0.2, 0.5), (0.4, -0.1, 0.2))
    cams = [pc.cam(60, 80), pc.cam(120, 160, T)]
    cams[1]["fy"] = F(-131.5)  # a mirrored axis is a camera too
    n_has = 0
    for it in range(600):
        cam = cams[it % 2]
        p = pr.params(z_max=float(rng.uniform(2, 9)), normal_dz=float(rng.choice([0.05, 0.01, 0.25])), conf_new=float(rng.uniform(0, 1)))
        z = F(rng.uniform(0.3, 8.0))
        d = np.array([z] + [z + F(rng.uniform(-1.2, 1.2) * p["normal_dz"]) for _ in range(4)], F)
        v, u = int(rng.integers(1, 200)), int(rng.integers(1, 300))
        colour = None if it % 3 == 0 else rng.integers(0, 256, 3)
        time = float(rng.integers(1, 100))
        want = pr.pixel_surfel(d, v, u, cam, colour, p, time)
        got = body_maps.pixel_surfel(d, v, u, lib_camera(cam), colour, body_maps.Params(**p), time)
        assert same(got, want), (it, d, got, want)
        n_has += want is not None
    assert 100 < n_has < 500
    # special depths in every position; normal_dz met exactly and one ulp beyond, on both sides
    cam, lc = cams[0], lib_camera(cams[0])
    p = pr.params(normal_dz=0.25)
    lp = body_maps.Params(**p)
    base = np.array([2.0, 2.25, 1.75, 2.25, 1.75], F)
    assert pr.pixel_surfel(base, 30, 40, cam, None, p, 1.0) is not None and same(body_maps.pixel_surfel(base, 30, 40, lc, None, lp, 1.0), pr.pixel_surfel(base, 30, 40, cam, None, p, 1.0))
    for k in range(5):
        for bad in (np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, 8.0, np.nextafter(F(8), F(9)), 1e-30):
            d = base.copy()
            d[k] = bad
            want = pr.pixel_surfel(d, 30, 40, cam, None, p, 1.0)
            assert same(body_maps.pixel_surfel(d, 30, 40, lc, None, lp, 1.0), want), (k, bad)
            assert want is None, (k, bad)  # not a valid depth, or valid and further than normal_dz from its neighbours
    for k in range(1, 5):
        for beyond, expect in ((np.nextafter(base[k], F(2)), True), (base[k], True), (np.nextafter(base[k], F(2) + (base[k] - F(2)) * 4), False)):
            d = base.copy()
            d[k] = beyond
            want = pr.pixel_surfel(d, 30, 40, cam, None, p, 1.0)
            assert (want is not None) == expect, (k, beyond)
            assert same(body_maps.pixel_surfel(d, 30, 40, lc, None, lp, 1.0), want)
    # every byte of a colour
    d = np.full(5, 2.0, F)
    for b in range(256):
        got = body_maps.pixel_surfel(d, 30, 40, lc, (b, 255 - b, (b * 7) % 256), lp, 1.0)
        assert got[4] == (b << 16) + ((255 - b) << 8) + (b * 7) % 256 and same(got, pr.pixel_surfel(d, 30, 40, cam, (b, 255 - b, (b * 7) % 256), p, 1.0))


def test_merge_surfel_equals_the_restatement_bit_for_bit():
    from staticfusion_amd import body_maps

    surf, _ = pc.first_map(12, 14)
    assert surf.shape[0] > 50
    rng = np.random.default_rng(12)
    special = pc.special_map(surf)
    for it in range(400):
        s = (special if it % 2 else surf)[int(rng.integers(0, surf.shape[0]))].copy()
        q = surf[int(rng.integers(0, surf.shape[0]))].copy()
        if it % 2 == 0:
            s[5] = F(rng.integers(1, 60))
            s[3] = F(rng.uniform(0, 1))
            s[8:11] += rng.normal(0, 0.2, 3).astype(F)
        if it % 7 == 0:
            q[8:11] = -s[8:11]  # the blend cancels when the weight is 1
            s[5] = F(1)
        p = pr.params(gain=float(rng.uniform(0.01, 1.0)), max_weight=float(rng.choice([1.0, 3.0, 32.0])))
        time = float(rng.integers(1, 50))
        want = pr.merge_surfel(s, q, p, time)
        got = body_maps.merge_surfel(s, q, body_maps.Params(**p), time)
        assert same(got, want), (it, s, q, got, want)
