"""Parity of the HIP path (libsf_hip.so, through the C ABI) against the CPU oracle and the golden
fixtures, on MI355X.  Bars (BASELINE.json north_star):
  * pyramids, K-means centres, cluster labels of every level, connectivity: BIT-EXACT
  * pose vs the CPU solver: <= 1e-4 rad and <= 1e-4 m per frame (measured ~1e-7)
  * b values <= 1e-4; the per-pixel static/dynamic decision (b > 0.5) identical
  * iteration counts (outer, IRLS, K-means) identical
Cross-pixel sums are accumulated in a different (parallel, fp64 / fixed-point) order on the GPU,
so reduced quantities agree to rounding, not bitwise; the image warp quantises projections to
centi-pixels, so a last-bit difference in T can move single pixels of the Warped images.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, config2_params, driver_params, hip_runtime, make_solver, trace_array
from staticfusion_amd import capi
from staticfusion_amd.synth import DEFAULT_XI, Scene, pose_delta, quantise_and_decimate, se3_exp

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4  # rad and m, north_star


def solve_both(hip, ora, rows, cols, mk_params, pr, seg_image=True):
    out = []
    for api in (hip, ora):
        s = make_solver(api, rows, cols, mk_params(api), pr)
        s.build_pyramid(True)
        s.run_solver(True)
        if seg_image:
            s.build_segm_image()
        out.append(s)
    return out


def assert_traces_match(sg, so, tol_twist=2e-6, tol_b=1e-4, rtol_aver=2e-4, n_valid_slack=0):
    """n_valid_slack: valid pixels by which an outer iteration may differ. The warp quantises target positions to centi-pixels
    (FrontEnd.cpp:819-820), so a last-bit difference of T can move a source pixel's taps to the neighbouring cells and a cell at the
    edge of the warped image in or out of validPixels; 0 everywhere except on scenes built to have thousands of such edges."""
    a, b = sg.stats(), so.stats()
    assert (a.n_outer, a.n_irls, a.kmeans_iters, a.status) == (b.n_outer, b.n_irls, b.kmeans_iters, b.status)
    assert abs(a.pixel_iters - b.pixel_iters) <= n_valid_slack * a.n_irls
    for f in ("level", "k", "irls_iters"):
        assert np.array_equal(trace_array(a, f), trace_array(b, f)), f
    assert np.abs(trace_array(a, "n_valid") - trace_array(b, "n_valid")).max() <= n_valid_slack
    assert np.allclose(trace_array(a, "aver_res"), trace_array(b, "aver_res"), rtol=rtol_aver, atol=1e-7)
    assert np.abs(trace_array(a, "var") - trace_array(b, "var")).max() < tol_twist
    assert np.abs(trace_array(a, "twist_level") - trace_array(b, "twist_level")).max() < tol_twist
    assert np.abs(trace_array(a, "T") - trace_array(b, "T")).max() < tol_twist
    assert np.abs(trace_array(a, "b_segm") - trace_array(b, "b_segm")).max() < tol_b


def assert_planes_close(g, o, frac=0.98, tol=5e-5, hard=0.2):
    """centi-pixel quantisation of the warp can move isolated pixels: all but 2 % within tol."""
    d = np.abs(g.astype(np.float64) - o.astype(np.float64))
    assert np.isfinite(d).all()
    assert (d <= tol).mean() >= frac, ((d <= tol).mean(), d.max())
    assert d.max() <= hard


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,sphere,seed", [(240, 320, True, 1234), (240, 320, False, 99), (120, 160, True, 7), (60, 80, False, 3)])
def test_pyramid_kmeans_labels_bit_exact(hip, ora, pair, rows, cols, sphere, seed):
    pr = pair(seed=seed, sphere=sphere, rows=rows, cols=cols)
    d_new = pr["new"][0].copy()
    d_new[rows // 3: rows // 2, cols // 2: cols // 2 + cols // 6] = 0  # invalid region: label 24, zero-centre branch
    d_new[::17, ::13] = 0                                                 # isolated holes
    prm = {"new": (d_new, pr["new"][1]), "old": pr["old"]}
    sg, so = solve_both(hip, ora, rows, cols, lambda a: driver_params(a), prm)
    for L in range(sg.levels):
        for pset in (capi.SET_NEW, capi.SET_PRED):
            for ch in range(4):
                assert np.array_equal(sg.plane(pset, ch, L), so.plane(pset, ch, L)), (L, pset, ch)
        assert np.array_equal(sg.labels(L), so.labels(L)), L
    assert np.array_equal(sg.kmeans_centres(), so.kmeans_centres())
    assert np.array_equal(sg.connectivity(), so.connectivity())
    assert sg.stats().kmeans_iters == so.stats().kmeans_iters


def test_config1_static_pair_qvga(hip, ora, pair):
    """BASELINE.json configs[1]: static pair, QVGA, 3 levels, segmentation disabled."""
    pr = pair(seed=1234, rows=240, cols=320)
    sg, so = solve_both(hip, ora, 240, 320, lambda a: config2_params(a, levels=3), pr)
    assert_traces_match(sg, so)
    rot, trans = pose_delta(so.T(), sg.T())
    assert rot <= POSE_TOL and trans <= POSE_TOL
    rot, trans = pose_delta(pr["T_gt"], sg.T())
    assert rot < 1.5e-3 and trans < 4e-3
    assert np.array_equal(sg.b(), so.b()) and np.all(sg.b_image() == 1.0)


@pytest.mark.parametrize("seed", [1234, 1235, 1240])
def test_config2_moving_sphere_full_solver(hip, ora, pair, seed):
    """BASELINE.json configs[2]: moving sphere, K-means(24) + b-field, driver parameters."""
    pr = pair(seed=seed, sphere=True, rows=240, cols=320)
    sg, so = solve_both(hip, ora, 240, 320, lambda a: driver_params(a), pr)
    assert_traces_match(sg, so)
    rot, trans = pose_delta(so.T(), sg.T())
    assert rot <= POSE_TOL and trans <= POSE_TOL
    for L in range(5):
        assert np.array_equal(sg.labels(L), so.labels(L))
    assert np.abs(sg.b() - so.b()).max() < 1e-4
    bg, bo = sg.b_image(), so.b_image()
    assert np.array_equal(bg > 0.5, bo > 0.5)  # the decision the map uses (reference Shaders/data.vert:180)
    assert np.abs(bg - bo).max() < 1e-4
    assert (bg < 0.5).mean() > 1e-3  # the sphere is flagged dynamic


def test_linearisation_and_warp_planes(hip, ora, pair):
    pr = pair(seed=11, sphere=True, rows=240, cols=320)
    sg, so = solve_both(hip, ora, 240, 320, lambda a: driver_params(a, debug_planes=1), pr)
    for which in range(capi.LIN_NULL):
        g, o = sg.lin_plane(which), so.lin_plane(which)
        if which in (capi.LIN_WC, capi.LIN_WD):
            # the pre-weights are normalised by their maximum 1/sqrt(eps + k |derivatives|) over the image
            # (reference FrontEnd.cpp:494-509), which is ill-conditioned in the best pixel's ddt = dn - dw:
            # a 1e-7 difference in T moves the common scale by a few per cent. Compare shape and scale apart.
            mg, mo = np.median(g[g > 0]), np.median(o[o > 0])
            assert abs(mg / mo - 1.0) < 0.1
            # ... and per pixel w = 1/sqrt(0.01 + 200 |ddt| + ...) moves by 1e-3 for a 1e-7 m change of dw
            assert_planes_close(g * (mo / mg), o, tol=2e-3)
            continue
        assert_planes_close(g, o)
    ng, no = sg.lin_plane(capi.LIN_NULL), so.lin_plane(capi.LIN_NULL)
    assert (ng != no).mean() < 1e-3
    for L in range(5):
        for pset in (capi.SET_WARPED, capi.SET_INTER):
            for ch in range(4):
                assert_planes_close(sg.plane(pset, ch, L), so.plane(pset, ch, L))
    # the coarsest level's first iteration uses Warped := Pred: exact
    for ch in range(4):
        assert np.array_equal(sg.plane(capi.SET_WARPED, ch, 4), so.plane(capi.SET_WARPED, ch, 4))


def test_golden_fixtures_on_the_hip_path(hip):
    import test_golden

    test_golden.check_pyramid(hip)
    test_golden.check_linearise_and_first_irls(hip)
    # the HIP path expands A from its factored rows (another association, FMA) and its IRLS weights use the hardware rsq
    test_golden.check_lin_planes_single_level(hip, tol_rows=5e-6, tol_ata=5e-6)
    test_golden.check_kmeans(hip)
    test_golden.check_full_solve(hip, tol=5e-6, tol_b=2e-4, tol_prior=2e-5)  # the HIP path's IRLS weights use the hardware rsq / rcp
    test_golden.check_history_residuals(hip, tol=2e-5)
    g = np.load(os.path.join(GOLDEN, "segm_image_160x120.npz"))
    s = make_solver(hip, 120, 160, driver_params(hip))
    s.set_segm_state(0, g["labels0"], g["b_segm"], g["cluster_res"])
    s.build_segm_image()
    assert np.array_equal(s.b_image(), g["b_image"])


def test_frame_sequence_with_history(hip, ora):
    """8 frames through sf_process_frame: carried state (twist_old, b_segm, 5-frame ring), the
    residual check from frame 5 on, per-frame pose parity."""
    scene = Scene(seed=77, sphere=True)
    xi = np.array(DEFAULT_XI) * 0.6
    frames, T = [], np.eye(4)
    for k in range(9):
        frames.append(quantise_and_decimate(*scene.render(T, 640, 480, sphere_offset=(0.02 * k, 0, 0))))
        T = T @ se3_exp(xi)
    solvers = [make_solver(api, 240, 320, driver_params(api, kb=1.5)) for api in (hip, ora)]
    for s in solvers:
        s.set_current(0, *frames[0])
        s.current_to_prediction()
        s.push_history(0)
    for k in range(1, 9):
        for s in solvers:
            s.set_prediction(0, *frames[k - 1])
            s.set_current(0, *frames[k])
            s.process_frame(k)
        sg, so = solvers
        rot, trans = pose_delta(so.T(), sg.T())
        assert rot <= POSE_TOL and trans <= POSE_TOL, (k, rot, trans)
        assert np.abs(sg.twist_old() - so.twist_old()).max() < 1e-5
        assert np.array_equal(sg.labels(0), so.labels(0))
        cg, co = sg.cluster_residuals(), so.cluster_residuals()
        assert np.array_equal(np.isnan(cg), np.isnan(co))
        # 1e-3: measured 1.2e-4 ... 6.5e-4 over three sequences and all builds (tools/diag/residual_dev.py, profiles/r03f_residual_dev.txt)
        # -- and the oracle against ITSELF with these sums in fp64 instead of its sequential float (3200 terms per cluster) differs by
        # 1.4e-4 ... 6.2e-4: the reference's own summation error, not the port's (the HIP sums are exact Q32.32 integers); single
        # pixels of the 5-frame warp that land on the other side of a centi-pixel account for the rest (2e-4 ... 3.7e-4 against fp64 sums)
        assert np.allclose(cg[~np.isnan(cg)], co[~np.isnan(co)], rtol=1e-3, atol=1e-6)
        bg, bo = sg.b_image(), so.b_image()
        assert np.array_equal(bg > 0.5, bo > 0.5), k  # the static / dynamic decision the map uses (Shaders/data.vert:180)
        assert np.abs(bg - bo).max() < 1e-4, k
        a, b = sg.stats(), so.stats()
        assert (a.n_outer, a.n_irls) == (b.n_outer, b.n_irls), k


def test_warp_with_targets_outside_the_tile_windows(hip, ora, pair):
    """A patch of picket fence (3-pixel bands at a third of the depth) in the predicted depth image, under a sideways
    motion: neighbouring source pixels of the patch move by very different amounts, so the targets of its tiles do not fit
    their accumulation windows. The one-workgroup builds then take the replay path of the splat (the accumulator columns
    are zeroed lazily there, sf_splat.h) -- the counter in slot 24 of the stage profile says that they really did
    -- and the warped images still equal the oracle's. (The rest of the image keeps the estimate well conditioned.)"""
    pr = pair(seed=21, rows=240, cols=320, xi=(0.05, 0.0, 0.0, 0.0, 0.0, 0.0))
    d_old = pr["old"][0].copy()
    patch = np.zeros((240, 320), bool)
    patch[90:150, 130:190] = True
    patch &= ((np.arange(320) // 3) % 2 == 0)[None, :]
    d_old[patch] *= 0.3
    fence = {"new": pr["new"], "old": (d_old, pr["old"][1])}
    sg, so = solve_both(hip, ora, 240, 320, lambda a: driver_params(a, debug_planes=1), fence)
    # The fence has 1200 depth edges: a last-bit difference of T can put a tap on the other side of a centi-pixel boundary there and
    # a cell or two in or out of validPixels. The bounds depend on whether that HAPPENED (one blanket tolerance would
    # hide a regression of the ordered splat's list path). Measured, profiles/r05b_fence_measured.txt: no such pixel in the latency
    # and cluster builds (b 1.2e-5, mean residual 2.7e-5 relative), two in the throughput build (b 6.9e-3 -- the UNCLAMPED b of the
    # cluster they belong to, 1.924 against 1.921 --, mean residual 1.2e-3).
    a, b = sg.stats(), so.stats()
    flipped = int(np.abs(trace_array(a, "n_valid") - trace_array(b, "n_valid")).max())
    assert flipped <= 4
    if flipped:
        assert_traces_match(sg, so, tol_twist=3e-6, tol_b=1e-2, n_valid_slack=4, rtol_aver=3e-3)
        assert np.abs(sg.b_image() - so.b_image()).max() < 1e-2
    else:
        assert_traces_match(sg, so, tol_twist=2e-6, tol_b=1e-4, rtol_aver=2e-4)
        assert np.abs(sg.b_image() - so.b_image()).max() < 1e-4
    assert np.array_equal(sg.b_image() > 0.5, so.b_image() > 0.5)
    for L in range(4):  # level 4 is warped once: Warped := Pred
        o0 = so.plane(capi.SET_WARPED, 0, L).astype(np.float64)
        pad = np.pad(o0, 1, mode="edge")
        nb = np.stack([pad[1 + dv:pad.shape[0] - 1 + dv, 1 + du:pad.shape[1] - 1 + du] for dv in (-1, 0, 1) for du in (-1, 0, 1)])
        smooth = (nb.max(0) - nb.min(0)) < 0.1  # cells whose 3 x 3 neighbourhood of the oracle's warped depth holds no depth edge
        for ch in range(2):
            d = np.abs(sg.plane(capi.SET_WARPED, ch, L).astype(np.float64) - so.plane(capi.SET_WARPED, ch, L).astype(np.float64))
            assert np.isfinite(d).all()
            if L >= 2:
                # the coarse levels: the fence is gone (3-pixel bands at level 0) and levels 3 / 4 take the reference's ordered float
                # sums -- every cell to rounding (measured 4.8e-7)
                assert d.max() <= 5e-6, (L, ch, d.max())
                continue
            # away from the depth edges the old tight bounds hold (measured: >= 0.9955 of those cells within 5e-5, worst 4.2e-3) ...
            assert (d[smooth] <= 5e-5).mean() >= 0.99 and d[smooth].max() <= 1.5e-2, (L, ch, (d[smooth] <= 5e-5).mean(), d[smooth].max())
            # ... at an edge a tap on the other side of a centi-pixel mixes depths 1.9 m apart (0.88 m measured at level 0, 1.1e-2 at 1)
            assert (d <= 5e-5).mean() >= 0.99 and d.max() <= (1.0 if L == 0 else 0.05), (L, ch, (d <= 5e-5).mean(), d.max())
    rot, trans = pose_delta(so.T(), sg.T())
    assert rot <= POSE_TOL and trans <= POSE_TOL
    assert np.array_equal(sg.labels(0), so.labels(0))
    if hip.default_variant != "cluster":  # a cluster zeroes the cells up front and sends such targets straight to them
        assert sg.splat_replays() > 0, "the scene did not exercise the replay path"


def test_throughput_build_picks_its_kernel_by_configuration(hip, pair):
    """The throughput build launches the 4-per-CU compilation of the frame kernel for pure odometry and the 5-per-CU one
    for the full solver (sf_get_resident_workgroups says which); both are covered by the parity tests above, which run with
    and without segmentation. The same stream must give the same answer whichever of the two runs it."""
    if hip.default_variant != "throughput":
        pytest.skip("one compilation per build")
    pr = pair(seed=5, sphere=True, rows=120, cols=160)
    seg = make_solver(hip, 120, 160, driver_params(hip), pr, batch=2000)
    odo = make_solver(hip, 120, 160, driver_params(hip, segmentation_enabled=0, ctf_levels=3), pr, batch=2000)
    assert seg.resident_workgroups()[0] == 5 and odo.resident_workgroups()[0] == 4
    assert seg.resident_workgroups()[1] == 5 * odo.resident_workgroups()[1] // 4  # 2000 streams exceed both grids
    out = {}
    for n in ("4", "5"):
        os.environ["SF_THROUGHPUT_WG_PER_CU"] = n
        try:
            s = make_solver(hip, 120, 160, driver_params(hip), pr)
            assert s.resident_workgroups()[0] == int(n)
            s.build_pyramid(True)
            s.run_solver(True)
            s.build_segm_image()
            out[n] = (s.T().copy(), s.b_image().copy(), s.labels(0).copy(), s.stats().n_irls)
        finally:
            del os.environ["SF_THROUGHPUT_WG_PER_CU"]
    assert np.array_equal(out["4"][2], out["5"][2]) and out["4"][3] == out["5"][3]
    assert np.array_equal(out["4"][0], out["5"][0]) and np.array_equal(out["4"][1], out["5"][1])


def test_edge_cases(hip, ora, pair):
    z = np.zeros((60, 80), np.float32)
    for api in (hip, ora):
        s = make_solver(api, 60, 80, driver_params(api), {"new": (z, z), "old": (z, z)})
        s.build_pyramid(True)
        s.run_solver(True)
        s.build_segm_image()
        assert s.stats().status & capi.STATUS_EMPTY_LEVEL
        assert np.array_equal(s.T(), np.eye(4, dtype=np.float32))
        assert np.all(s.labels(0) == 24) and np.all(s.b_image() == 1.0)
    # identical images: zero motion on both
    pr = pair(seed=3, rows=60, cols=80)
    same = {"new": pr["new"], "old": pr["new"]}
    sg, so = solve_both(hip, ora, 60, 80, lambda a: driver_params(a), same)
    assert np.abs(sg.T() - np.eye(4)).max() < 1e-6
    assert_traces_match(sg, so)
    # half of the new image invalid + large motion (3 outer iterations per level possible)
    big = pair(seed=8, rows=120, cols=160, xi=tuple(4 * np.array(DEFAULT_XI)))
    d = big["new"][0].copy()
    d[:, :70] = 0
    sg, so = solve_both(hip, ora, 120, 160, lambda a: driver_params(a), {"new": (d, big["new"][1]), "old": big["old"]})
    assert_traces_match(sg, so, tol_twist=1e-5, tol_b=3e-4)  # stress case: large motion, half the image invalid
    rot, trans = pose_delta(so.T(), sg.T())
    assert rot <= POSE_TOL and trans <= POSE_TOL


def test_batch_streams_are_independent_and_deterministic(hip, pair):
    """Full-size property check: 96 streams (3 distinct pairs tiled) in one launch; equal inputs give
    bit-equal outputs wherever they sit in the batch, run to run, and equal the single-stream result."""
    prs = [pair(seed=s, sphere=True, rows=240, cols=320) for s in (1234, 1235, 1240)]
    B = 96
    p = driver_params(hip)
    results = []
    for _ in range(2):
        s = make_solver(hip, 240, 320, p, batch=B)
        for b in range(B):
            s.set_current(b, *prs[b % 3]["new"])
            s.set_prediction(b, *prs[b % 3]["old"])
        s.process_frame(0)
        T, n_irls, n_outer, pix = s.batch_results()
        bimg = [s.b_image(b) for b in (0, 1, 2, 93, 94, 95)]
        results.append((T, n_irls, n_outer, pix, bimg))
        s.close()
    T, n_irls, n_outer, pix, bimg = results[0]
    for b in range(B):
        assert np.array_equal(T[b], T[b % 3]) and n_irls[b] == n_irls[b % 3] and pix[b] == pix[b % 3]
    assert np.array_equal(results[0][0], results[1][0])  # run-to-run determinism (order-independent sums)
    for i in range(3):
        assert np.array_equal(bimg[i], bimg[3 + i])
    single = make_solver(hip, 240, 320, p, prs[1])
    single.process_frame(0)
    if hip.default_variant == "cluster":  # the number of workgroups per stream (the partition of the sums) depends on the batch
        assert np.abs(single.T(0) - T[1]).max() < 2e-6
    else:
        assert np.array_equal(single.T(0), T[1])
    for b in range(3):  # rigid transforms
        R = T[b][:3, :3].astype(np.float64)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-5 and abs(np.linalg.det(R) - 1) < 1e-5


@pytest.mark.parametrize("config", ["configs1_static", "configs2_sphere"])
def test_bench_size_batch_against_the_oracle(hip, ora, pair, config):
    """The shape bench.py times -- >= 1024 QVGA streams in ONE launch of the frame kernel, on the build the fixture names
    (`[throughput]` = sf_frame_kernel_nt256, the one behind the headline number) -- with 8 DISTINCT pairs tiled over the
    batch; 16 streams spread over the batch (the 8 distinct pairs at both ends of the work queue) are compared with the
    CPU oracle: labels of every level and iteration counts exactly, pose <= 1e-4, b <= 1e-4, (b > 0.5) identical.
    Loop under test: reference FrontEnd.cpp:1071-1146 (runSolver), driven as StaticFusion-datasets.cpp:171-184."""
    sphere = config == "configs2_sphere"
    mk = (lambda a: driver_params(a)) if sphere else (lambda a: config2_params(a, levels=3))
    prs = [pair(seed=4321 + 7 * q, sphere=sphere, rows=240, cols=320) for q in range(8)]
    B = 1024
    s = make_solver(hip, 240, 320, mk(hip), batch=B)
    name, threads, per_stream = s.variant()
    assert name == hip.default_variant and threads == {"throughput": 256, "latency": 1024}.get(name, threads)
    for b in range(B):
        s.set_current(b, *prs[b % 8]["new"])
        s.set_prediction(b, *prs[b % 8]["old"])
    s.process_frame(0)
    T, n_irls, n_outer, pix = s.batch_results()
    o = make_solver(ora, 240, 320, mk(ora), batch=8)
    for q in range(8):
        o.set_current(q, *prs[q]["new"])
        o.set_prediction(q, *prs[q]["old"])
    o.process_frame(0)
    To, n_irls_o, n_outer_o, pix_o = o.batch_results()
    for b in range(B):  # every stream: counts exactly, pose within the bar
        q = b % 8
        assert (n_irls[b], n_outer[b], pix[b]) == (n_irls_o[q], n_outer_o[q], pix_o[q]), b
        rot, trans = pose_delta(To[q], T[b])
        assert rot <= POSE_TOL and trans <= POSE_TOL, (b, rot, trans)
    assert len({T[q].tobytes() for q in range(8)}) == 8  # the streams really differ
    for b in list(range(8)) + list(range(B - 8, B)):  # field-level comparison on 16 of them
        q = b % 8
        a, c = s.stats(b), o.stats(q)
        assert (a.n_outer, a.n_irls, a.kmeans_iters, a.status) == (c.n_outer, c.n_irls, c.kmeans_iters, c.status)
        assert np.abs(trace_array(a, "twist_level") - trace_array(c, "twist_level")).max() < 5e-6
        assert np.abs(s.b(b) - o.b(q)).max() < 1e-4
        if sphere:
            for L in range(s.levels):
                assert np.array_equal(s.labels(L, b), o.labels(L, q)), (b, L)
            assert np.array_equal(s.kmeans_centres(b), o.kmeans_centres(q))
            bg, bo = s.b_image(b), o.b_image(q)
            assert np.array_equal(bg > 0.5, bo > 0.5) and np.abs(bg - bo).max() < 1e-4
            assert (bg < 0.5).mean() > 1e-3


def test_device_resident_inputs_and_counters(hip, pair):
    """set_*_device (inputs already in HBM) + the device-side counters used by bench.py."""
    import ctypes

    pr = pair(seed=5, rows=120, cols=160)
    B = 4
    s = make_solver(hip, 120, 160, config2_params(hip, levels=3), pr, batch=B)
    s.process_frame(0)
    T_host, n_irls, _, _ = s.batch_results()
    hiprt = hip_runtime()
    n = 120 * 160
    col = lambda a: np.ascontiguousarray(np.tile(np.asarray(a, np.float32).T.ravel(), B))
    bufs = []
    for arr in (pr["new"][0], pr["new"][1], pr["old"][0], pr["old"][1]):
        ptr = ctypes.c_void_p()
        assert hiprt.hipMalloc(ctypes.byref(ptr), ctypes.c_size_t(4 * n * B)) == 0
        h = col(arr)
        assert hiprt.hipMemcpy(ptr, h.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(h.nbytes), 1) == 0
        bufs.append(ptr)
    s2 = make_solver(hip, 120, 160, config2_params(hip, levels=3), batch=B)
    hip.check(hip.set_current_device(s2.h, bufs[0], bufs[1]))
    hip.check(hip.set_prediction_device(s2.h, bufs[2], bufs[3]))
    s2.process_frame(0)
    T_dev, n_irls2, _, _ = s2.batch_results()
    assert np.array_equal(T_host, T_dev) and np.array_equal(n_irls, n_irls2)
    frames, irls, outer, pix = s2.counters()
    assert frames == B and irls == int(n_irls2.sum()) and outer == 3 * B and pix > 0
    for ptr in bufs:
        hiprt.hipFree(ptr)


def test_vga_resolution_six_levels(hip, ora):
    """res_factor 1 of the reference constructor: 480x640, ctf_levels = log2(640/40) + 2 = 6 (maximum size)."""
    from staticfusion_amd.synth import make_pair

    pr = make_pair(seed=5, sphere=True, out_rows=480, out_cols=640)
    sg, so = solve_both(hip, ora, 480, 640, lambda a: driver_params(a), pr)
    assert sg.levels == 6 and sg.level_shape(5) == (15, 20)
    for L in range(6):
        assert np.array_equal(sg.labels(L), so.labels(L)), L
        assert np.array_equal(sg.plane(capi.SET_NEW, capi.CH_DEPTH, L), so.plane(capi.SET_NEW, capi.CH_DEPTH, L))
    assert np.array_equal(sg.kmeans_centres(), so.kmeans_centres())
    # the oracle sums 600k residuals sequentially in float32 (reference FrontEnd.cpp:655-664): ~1e-3 relative
    assert_traces_match(sg, so, tol_twist=5e-6, rtol_aver=2e-3, tol_b=1e-3)
    rot, trans = pose_delta(so.T(), sg.T())
    assert rot <= POSE_TOL and trans <= POSE_TOL
    assert np.array_equal(sg.b_image() > 0.5, so.b_image() > 0.5)


@pytest.mark.parametrize("seed", range(2000, 2012))
def test_many_seeds_small(hip, ora, pair, seed):
    """A dozen random scenes/motions at 160x120: labels identical, iteration counts identical, pose <= 1e-4."""
    from staticfusion_amd.synth import LCG64

    g = LCG64(seed)
    xi = tuple(np.array(DEFAULT_XI) * np.array([g.uniform(-2.5, 2.5) for _ in range(6)]))
    pr = pair(seed=seed, sphere=(seed % 2 == 0), rows=120, cols=160, xi=xi)
    sg, so = solve_both(hip, ora, 120, 160, lambda a: driver_params(a, kb=1.5 if seed % 3 else 1.05), pr)
    a, b = sg.stats(), so.stats()
    assert (a.n_outer, a.n_irls, a.kmeans_iters) == (b.n_outer, b.n_irls, b.kmeans_iters)
    for L in range(sg.levels):
        assert np.array_equal(sg.labels(L), so.labels(L))
    rot, trans = pose_delta(so.T(), sg.T())
    assert rot <= POSE_TOL and trans <= POSE_TOL
    assert np.abs(sg.b() - so.b()).max() < 2e-4


# sizes whose level 0 ends in a PARTLY filled wave: n0 % 64 = 16 (fewer active lanes than labels) or 48; odd rows / columns from
# level 1 on (level 0 itself must be even with segmentation: KMeans.cpp:267 reads labels_lowres(v/2, u/2))
PARTIAL_WAVE_SIZES = [(40, 42, 3), (36, 116, 2), (20, 52, 2), (26, 104, 3), (34, 72, 4), (20, 44, 2)]


def partial_wave_pair(pair, rows, cols, seed=5):
    pr = pair(seed=seed, sphere=True, rows=rows, cols=cols)
    d_new = pr["new"][0].copy()
    d_new[-3:, -1] = 0  # pixels of the last, partly filled wave that belong to no cluster (label 24: b image 1.0)
    return {"new": (d_new, pr["new"][1]), "old": pr["old"]}


@pytest.mark.parametrize("rows,cols,levels", PARTIAL_WAVE_SIZES)
def test_last_wave_partly_filled(hip, ora, pair, rows, cols, levels):
    """Images whose pixel count is not a multiple of the wave size (sf_create_ex only asks for a multiple of 4 per level): the
    cross-lane code -- ds_bpermute in stage_segm_image, the DPP neighbours of the strip linearisation, the ballots of K-means --
    meets a last wave with 16 (or 48) active pixels, fewer than there are labels. Round 5's segm image gave such pixels b = 0
    when their label was >= the number of active lanes (a lane that has left the loop returns 0 to ds_bpermute)."""
    assert (rows * cols) % 64 in (16, 48)
    pr = partial_wave_pair(pair, rows, cols)
    solvers = []
    for api in (hip, ora):
        s = make_solver(api, rows, cols, driver_params(api, kb=1.5, ctf_levels=levels), pr)
        s.build_pyramid(True)
        s.run_solver(True)
        s.build_segm_image()
        solvers.append(s)
    sg, so = solvers
    assert_traces_match(sg, so, tol_twist=5e-6, rtol_aver=2e-3, tol_b=1e-3)
    for L in range(levels):
        assert np.array_equal(sg.labels(L), so.labels(L)), L
    bg, bo = sg.b_image(), so.b_image()
    assert np.all(bg[sg.labels(0) == 24] == 1.0) and (sg.labels(0) == 24).any()
    assert np.array_equal(bg > 0.5, bo > 0.5)
    assert np.abs(bg - bo).max() < 1e-3
    # the value of a pixel is a function of its label alone: the last wave's pixels carry the values of the full waves' pixels
    lab = sg.labels(0)
    for l in np.unique(lab):
        assert np.unique(bg[lab == l]).size == 1, l
    rot, trans = pose_delta(so.T(), sg.T())
    assert rot <= POSE_TOL and trans <= POSE_TOL


@pytest.mark.parametrize("rows,cols,levels", PARTIAL_WAVE_SIZES[:2])
def test_last_wave_partly_filled_frame_sequence(hip, ora, pair, rows, cols, levels):
    """... and through sf_process_frame with the five-frame residuals (the 0.017 rule of buildSegmImage switched on by history)."""
    scene = Scene(seed=21, sphere=True, sphere_seed=77)
    T = np.eye(4)
    frames = []
    for k in range(8):
        d, i = scene.render(T, 2 * cols, 2 * rows, sphere_offset=(0.03 * k, 0, 0))
        d, i = quantise_and_decimate(d, i)
        d[-3:, -1] = 0
        frames.append((d, i))
        T = T @ se3_exp(DEFAULT_XI)
    solvers = [make_solver(api, rows, cols, driver_params(api, kb=1.5, ctf_levels=levels)) for api in (hip, ora)]
    for s in solvers:
        s.set_current(0, *frames[0])
        s.current_to_prediction()
        s.push_history(0)
    for k in range(1, 8):
        for s in solvers:
            s.set_prediction(0, *frames[k - 1])
            s.set_current(0, *frames[k])
            s.process_frame(k)
        sg, so = solvers
        bg, bo = sg.b_image(), so.b_image()
        assert np.array_equal(sg.labels(0), so.labels(0)), k
        assert np.array_equal(bg > 0.5, bo > 0.5), k
        assert np.abs(bg - bo).max() < 1e-3, k
        assert np.all(bg[sg.labels(0) == 24] == 1.0), k
        rot, trans = pose_delta(so.T(), sg.T())
        assert rot <= POSE_TOL and trans <= POSE_TOL, k


@pytest.mark.parametrize("rows,cols,levels", [(48, 43, 2), (45, 48, 2), (36, 117, 1)])
def test_odd_image_sizes_pure_odometry(hip, ora, pair, rows, cols, levels):
    """Odd rows / columns at level 0 exist for the pure odometry of configs[1] only (K-means refuses them on both sides:
    KMeans.cpp:267 reads outside its label matrix). 48 x 43: n0 % 64 = 16; 45 x 48: 48; 36 x 117: 52 (one level)."""
    pr = pair(seed=6, rows=rows, cols=cols)
    sg, so = solve_both(hip, ora, rows, cols, lambda a: config2_params(a, levels=levels), pr)
    assert_traces_match(sg, so, tol_twist=5e-6, rtol_aver=2e-3)
    rot, trans = pose_delta(so.T(), sg.T())
    assert rot <= POSE_TOL and trans <= POSE_TOL
    assert np.all(sg.b_image() == 1.0) and np.array_equal(sg.b(), so.b())
    for L in range(levels):
        for ch in range(4):
            assert np.array_equal(sg.plane(capi.SET_NEW, ch, L), so.plane(capi.SET_NEW, ch, L)), (L, ch)
