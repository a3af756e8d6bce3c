"""calculateCoord, calculateDerivatives, computeWeights, the Jacobian rows and computeSegPrior against EXACT fp64 references
(tests/exact_ref.py, section D) -- the stages between the warped planes (test_exact_references.py: warp_checks) and the rows
that test's irls_inputs takes as given. Each stage is recomputed from the planes the implementation itself gave it (NEW and
WARPED -> Inter / Null / dct / ddt; Inter -> gradients; derivative planes -> weights; derivative planes + depths + exact weights
-> rows; depths + labels -> prior) and held to a bound that is a COUNT of float roundings times u = 2^-24 on the magnitude of
the terms that can cancel (the counts stand next to the constants in exact_ref.py). The planes are those of the last outer
iteration of a solve.

CPU part: the oracle meets every bound on the suite's scenes, on two scenes made for the prior's branches and for points behind
the camera, on a first iteration (Warped := Pred) and on the strip-edge geometries; four perturbations of oracle outputs that the
suite's older bars accept are rejected.
GPU part (marked one by one): the three product builds and libsf_hip_reforder.so on the same checks, the geometry sweep of
solve_linearise_strips (level-0 sizes around the 62-row strips and with short / uneven column segments; on the cluster build the
same sizes walk the LDS tiles of solve_linearise), the global maxima, debug_planes = 0 against = 1, and a batch of eight
streams. Every test prints max |got - exact| / bound per stage: coord (bound: 1/2 ulp), gradients, weights, rows A, rows B, prior.

Rules for a pixel warped BEHIND the camera (exact_ref.coord_reference): the product builds and the oracle with
sfo_test_set_hip_behind_camera_rule leave it out of validPixels; the oracle without it and the reference-order build keep it.
The rows of such a kept pixel are not compared: d = (dn + dw) / 2 cancels there, which the row count does not cover.
"""
import ctypes
import os

import numpy as np
import pytest

import exact_ref as E
from conftest import config2_params, driver_params, make_solver
from staticfusion_amd import _capi as capi
from staticfusion_amd.synth import make_pair
from test_exact_references import SCENES, irls_solver, solve, tan_half_fovh

PRODUCT = ("throughput", "latency", "cluster")
LS_ROWS = 62  # rows of a register strip (sf_solve_shared.h)
LIN = dict(dcu=capi.LIN_DCU, dcv=capi.LIN_DCV, dct=capi.LIN_DCT, ddu=capi.LIN_DDU, ddv=capi.LIN_DDV, ddt=capi.LIN_DDT, wc=capi.LIN_WC,
           wd=capi.LIN_WD)
STAGES = ("coord", "gradients", "weights", "rows_A", "rows_B", "prior")


def where(v, u):
    """a pixel in the terms of solve_linearise_strips: (v, u), its strip and the lane that owns it"""
    return "(v, u) = (%d, %d): strip %d, lane %d" % (v, u, v // LS_ROWS, v % LS_ROWS + 1)


def last_iteration(s, stream=0):
    st = s.stats(stream)
    j = st.n_outer - 1
    tr = st.outer[j]
    return st, tr, s.levels - 1 - tr.level, (tr.level == 0 and tr.k == 0)


def linearisation_checks(s, kind, stream=0, expect_first=False, prior_path=None):
    """Every stage of the last outer iteration of `stream` against its exact reference. kind: "oracle", "oracle+rule" (the
    oracle with the product's behind-the-camera rule), one of PRODUCT, or "reforder". -> dict: the ratios of STAGES, the exact
    references, and what the scene exercised (n_behind, starved / full clusters, min_e_c, min_e_d)."""
    product = kind in PRODUCT
    rule_valid = "product" if product or kind == "oracle+rule" else "reference"
    rule_planes = "product" if product else "reference"  # (the oracle's ddt plane is dn - dw whatever its rule)
    st, tr, L, first = last_iteration(s, stream)
    assert first == expect_first, "the last outer iteration (level %d, k %d) %s on Warped := Pred" % (tr.level, tr.k, "ran" if first else "did not run")
    new = [s.plane(capi.SET_NEW, ch, L, stream) for ch in (capi.CH_DEPTH, capi.CH_INTENSITY)]
    wrp = [s.plane(capi.SET_WARPED, ch, L, stream) for ch in (capi.CH_DEPTH, capi.CH_INTENSITY)]
    inter = [s.plane(capi.SET_INTER, ch, L, stream) for ch in (capi.CH_DEPTH, capi.CH_INTENSITY)]
    lin = {k: s.lin_plane(w, stream) for k, w in LIN.items()}
    null = s.lin_plane(capi.LIN_NULL, stream) != 0
    out = {}

    # -- calculateCoord + the temporal derivatives: exact sets, one rounding per value
    ref = E.coord_reference(*new, *wrp, behind_camera=rule_valid)
    valid = ref["valid"]
    planes = ref if rule_planes == rule_valid else E.coord_reference(*new, *wrp, behind_camera=rule_planes)
    assert np.array_equal(null, ref["null"]), ("Null", kind, where(*np.argwhere(null != ref["null"])[0]))
    assert int(valid.sum()) == tr.n_valid, ("validPixels", kind, int(valid.sum()), tr.n_valid)
    everywhere = np.ones(null.shape, bool)
    r = [E.check_planes(got, planes[k], everywhere) for got, k in ((inter[0], "depth"), (inter[1], "intensity"), (lin["dct"], "dct"), (lin["ddt"], "ddt"))]
    out["coord"] = max(x[0] for x in r)
    assert out["coord"] <= 1.0, ("coord", kind, [(x[0], where(*x[1])) for x in r])

    # -- the edge-aware gradients from the implementation's Inter planes; exactly 0 where the implementation defines none
    defined = valid if product else (~null & E._inner(null.shape))
    g = E.gradient_reference(*inter, null)
    r = {k: E.check_planes(lin[k], g[k], defined, c=E.C_GRADIENT, mag=g["m_" + k]) for k in ("dcu", "dcv", "ddu", "ddv")}
    out["gradients"] = max(x[0] for x in r.values())
    assert all(x[2] for x in r.values()), ("a gradient plane is not 0 outside its pixels", kind, {k: x[2] for k, x in r.items()})
    assert out["gradients"] <= 1.0, ("gradients", kind, {k: (x[0], where(*x[1])) for k, x in r.items()})

    # -- computeWeights from the implementation's derivative planes: IEEE planes, maximum 1 within 2 ulp, 0 outside validPixels
    w = E.weights_reference(*(lin[k] for k in ("dcu", "dcv", "dct", "ddu", "ddv", "ddt")), valid)
    r = {k: E.check_planes(lin[k], w[k], valid, c=E.C_WEIGHT, relative=True, half_ulp=False) for k in ("wc", "wd")}
    out["weights"] = max(x[0] for x in r.values())
    assert all(x[2] for x in r.values()), ("a weight plane is not 0 outside validPixels", kind)
    assert out["weights"] <= 1.0, ("weights", kind, {k: (x[0], where(*x[1])) for k, x in r.items()})
    if valid.any():
        for k in ("wc", "wd"):
            assert abs(float(lin[k][valid].max()) - 1.0) <= 2 * 2.0 ** -23, ("max " + k, kind, float(lin[k][valid].max()))
    out["min_e_c"], out["min_e_d"] = w["min_e_c"], w["min_e_d"]

    # -- the rows, with the EXACT weights: the kernels' own pre-weights are in here and nowhere else
    A, B = s.jacobian_rows(stream)
    Ar, Br, xyd = E.rows_reference(*(lin[k] for k in ("dcu", "dcv", "dct", "ddu", "ddv")), new[0], wrp[0], w["wc"], w["wd"], valid,
                                   tan_half_fovh(s), s.params.k_photometric_res)
    assert A.shape == Ar.shape, (A.shape, Ar.shape)
    keep = np.repeat((wrp[0].T.ravel()[valid.T.ravel()] > 0), 2)  # (see the module docstring: kept pixels behind the camera)
    rA, rB, at = E.check_rows(A[keep], B[keep], Ar[keep], Br[keep], [q[keep[::2]] for q in xyd])
    out["rows_A"], out["rows_B"] = rA, rB
    if rA > 1.0 or rB > 1.0:
        px = np.argwhere(valid.T & (wrp[0].T > 0))[at[0] // 2]  # (u, v) in validPixels order
        raise AssertionError(("rows", kind, rA, rB, "row %d entry %d" % at, where(int(px[1]), int(px[0]))))

    # -- computeSegPrior
    out.update(prior=0.0, n_behind=ref["n_behind"], ref=ref, weights_ref=w, rows_ref=(Ar, Br, xyd), lin=lin, valid=valid, trace=tr, level=L)
    if s.params.segmentation_enabled:
        p = E.seg_prior_reference(new[0], wrp[0], s.labels(L, stream), s.params.kz, behind_camera=rule_valid)
        lam = np.array(tr.lambda_t_w, np.float32)
        assert np.array_equal(lam.view(np.uint32), p["lambda_t_w"].view(np.uint32)), ("lambda_t_w", kind, lam, p["lambda_t_w"])
        path = prior_path or ("integer" if product else "float")
        bp = np.array(tr.b_prior, np.float64)
        out["prior"] = float((np.abs(bp - p["b_prior"]) / (p["bound"][path] + 0.5 * E.ulp32(p["b_prior"]))).max())
        assert out["prior"] <= 1.0, ("b_prior", kind, path, out["prior"], int(np.argmax(np.abs(bp - p["b_prior"]) / (p["bound"][path] + 1e-30))))
        out["prior_ref"] = p
    return out


def report(tag, kind, out):
    print("linearisation %s %s: max |got - exact| / bound " % (tag, kind) + ", ".join("%s %.3g" % (k, out[k]) for k in STAGES))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
#  scenes of this file
# ------------------------------------------------------------------------------------------------------------------------------
def _starved_pair():
    """depth holes in the new frame (invalid labels, as in test_gpu_parity.py::test_pyramid_kmeans_labels_bit_exact) and the
    left part of the old frame zeroed: the clusters there find (almost) no warped depth -- the prior's `ratio < 0.1` branch"""
    pr = make_pair(seed=1234, sphere=True, out_rows=240, out_cols=320)
    d_new = pr["new"][0].copy()
    d_new[80:120, 160:213] = 0
    d_new[::17, ::13] = 0
    d_old = pr["old"][0].copy()
    d_old[:, :110] = 0
    return {"new": (d_new, pr["new"][1]), "old": (d_old, pr["old"][1])}


def _flat_patch_pair():
    """the same frame twice, with a patch of constant depth and intensity: T stays the identity, the warp reproduces the patch
    exactly (weighted means of equal values, 2.0 and 0.5, are exact in either summation), so the smallest error_l is exactly 0
    for both weights -- the extreme of lin_finish's bit trick 0x7f7fffff - bits"""
    pr = make_pair(seed=77, sphere=False, out_rows=120, out_cols=160)
    d, i = pr["new"][0].copy(), pr["new"][1].copy()
    d[40:80, 60:110] = 2.0
    i[40:80, 60:110] = 0.5
    return {"new": (d, i), "old": (d.copy(), i.copy())}


def _near_patch_pair():
    from test_gpu_edge_rules import _near_patch_pair as f

    return f()


SWEEP_XI = (0.05, -0.03, 0.04, 0.015, -0.02, 0.02)  # |xi| = 0.08: the first iteration's twist passes the 0.04 stop, a warp follows
# (rows, cols) of level 0. Heights on both sides of the strip edges (62, 124, 186 rows); widths that leave the column segments
# n_seg = min(cols, SF_NW / gcd(strips, SF_NW)), SF_NW = 4 / 16, uneven or shorter than the sweep's three-column loop.
# The ABI wants rows, cols >= 8 and a pixel count that is a multiple of 4: 62 x 5 became 62 x 8 (segments of 2 columns and of 1),
# 63 x 41 became 63 x 44 (two strips, the second of one row; 44 = 4 x 11 = 8 x 5 + 4: uneven on the latency build).
SWEEP = [(15, 20), (30, 40), (61, 20), (62, 8), (62, 20), (63, 44), (64, 12), (124, 9), (125, 96), (126, 10), (187, 12)]


def sweep_solver(api, rows, cols, iters=3):
    pr = make_pair(seed=1000 * rows + cols, sphere=False, out_rows=rows, out_cols=cols, xi=SWEEP_XI)
    s = make_solver(api, rows, cols, config2_params(api, levels=1, max_iter_per_level=iters, debug_planes=1), pr)
    s.build_pyramid(True)
    s.run_solver(True)
    return s


def solve_pair(api, rows, cols, params, pr, prepare=None):
    s = make_solver(api, rows, cols, params, pr)
    if prepare is not None:
        prepare(s)
    s.build_pyramid(True)
    s.run_solver(True)
    return s


def _hook(ora, name, value):
    fn = getattr(ora.lib, name)
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int]

    def prepare(s):
        assert fn(s.h, value) == 0

    return prepare


# ------------------------------------------------------------------------------------------------------------------------------
#  CPU part: the oracle inside every bound
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_oracle_linearisation_meets_the_bounds(ora, name):
    report(name, "oracle", linearisation_checks(solve(ora, name), "oracle"))


@pytest.mark.parametrize("seg", [False, True])
def test_oracle_linearisation_of_the_irls_scene(ora, seg):
    report("irls_solver seg=%d" % seg, "oracle", linearisation_checks(irls_solver(ora, seg, True), "oracle"))


def starved_checks(api, kind):
    s = solve_pair(api, 240, 320, driver_params(api, debug_planes=1), _starved_pair())
    out = linearisation_checks(s, kind)
    p = out["prior_ref"]
    assert (s.labels(out["level"]) == capi.NUM_CLUSTERS).any(), "no invalid label"
    assert p["starved"].any() and p["full"].any(), ("both branches of the prior", p["size"], p["nonnull"])
    assert (p["starved"] & (p["nonnull"] > 0)).any(), "no starved cluster with a non-Null pixel: the ratio is not between 0 and 0.1"
    return report("starved", kind, out)


def test_oracle_prior_takes_both_branches(ora):
    starved_checks(ora, "oracle")


@pytest.mark.parametrize("rule", [0, 1])
def test_oracle_points_behind_the_camera(ora, rule):
    """test_gpu_edge_rules.py's scene under both settings of the oracle's switch; the pixels in question exist in the LAST outer
    iteration (n_behind: inner, non-Null, warped depth < 0) and are in validPixels exactly without the product's rule"""
    s = solve_pair(ora, 120, 160, driver_params(ora, debug_planes=1), _near_patch_pair(), _hook(ora, "sfo_test_set_hip_behind_camera_rule", rule))
    kind = "oracle+rule" if rule else "oracle"
    out = report("behind_camera", kind, linearisation_checks(s, kind))
    assert out["n_behind"] > 0, "the last outer iteration has no pixel behind the camera"
    behind = ~out["ref"]["null"] & E._inner(out["valid"].shape) & (s.plane(capi.SET_WARPED, capi.CH_DEPTH, out["level"]) < 0)
    assert out["valid"][behind].all() == (rule == 0) and out["valid"][behind].any() == (rule == 0)


def test_oracle_first_iteration(ora):
    """Warped := Pred (FIRST is a template parameter of the product's sweep): one level, one outer iteration. Pure odometry: with
    segmentation the ABI wants two levels, and the last outer iteration -- the one whose planes can be read -- is then a warped one."""
    pr = make_pair(seed=9, sphere=True, out_rows=120, out_cols=160)
    s = solve_pair(ora, 120, 160, config2_params(ora, levels=1, max_iter_per_level=1, debug_planes=1), pr)
    report("first", "oracle", linearisation_checks(s, "oracle", expect_first=True))


@pytest.mark.parametrize("rows,cols", SWEEP)
def test_oracle_strip_edge_geometries(ora, rows, cols):
    report("%dx%d" % (rows, cols), "oracle", linearisation_checks(sweep_solver(ora, rows, cols), "oracle"))


def flat_patch_checks(api, kind):
    s = solve_pair(api, 120, 160, driver_params(api, debug_planes=1), _flat_patch_pair())
    out = report("flat_patch", kind, linearisation_checks(s, kind))
    assert out["min_e_c"] == 0.0 and out["min_e_d"] == 0.0, ("the patch does not reach error_l = 0", out["min_e_c"], out["min_e_d"])
    assert float(out["lin"]["wc"].max()) == 1.0  # sqrt(1 / (1 + 0)) and its reciprocal are exact


def test_oracle_global_maxima_with_a_zero_linearisation_error(ora):
    flat_patch_checks(ora, "oracle")


# ------------------------------------------------------------------------------------------------------------------------------
#  the checks reject what the older bars accept
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def qvga(ora):
    s = irls_solver(ora, True, True)
    return s, linearisation_checks(s, "oracle")


def test_rejects_a_halo_lane_slip(qvga):
    """(a) image row 62 of dcv -- the first row of the second strip, whose upper neighbour comes from a halo lane -- recomputed with
    the row two above in place of the row above: test_gpu_parity.py's assert_planes_close accepts the plane (one row is 0.4 % of
    it), the gradient check does not"""
    from test_gpu_parity import assert_planes_close

    s, out = qvga
    L = out["level"]
    null = out["ref"]["null"]
    inter = [s.plane(capi.SET_INTER, ch, L) for ch in (capi.CH_DEPTH, capi.CH_INTENSITY)]
    v0 = LS_ROWS
    slipped = [p.copy() for p in inter]
    nul2 = null.copy()
    for p in slipped:
        p[v0 - 1] = p[v0 - 2]
    nul2[v0 - 1] = null[v0 - 2]
    bad_row = E.gradient_reference(*slipped, nul2)["dcv"][v0]
    defined = ~null & E._inner(null.shape)
    bad = out["lin"]["dcv"].copy()
    bad[v0] = np.where(defined[v0], bad_row, 0.0).astype(np.float32)
    assert (bad[v0] != out["lin"]["dcv"][v0]).mean() > 0.5
    assert_planes_close(bad, out["lin"]["dcv"])
    g = E.gradient_reference(*inter, null)
    ratio, at, _ = E.check_planes(bad, g["dcv"], defined, c=E.C_GRADIENT, mag=g["m_dcv"])
    assert ratio > 100 and at[0] == v0, (ratio, at)


def test_rejects_a_wrong_global_maximum(qvga):
    """(b) WC scaled by 1.03: the median / rescaled-plane comparison of test_linearisation_and_warp_planes accepts it"""
    from test_gpu_parity import assert_planes_close

    s, out = qvga
    o = out["lin"]["wc"]
    bad = (o * np.float32(1.03)).astype(np.float32)
    mg, mo = np.median(bad[bad > 0]), np.median(o[o > 0])
    assert abs(mg / mo - 1.0) < 0.1
    assert_planes_close(bad * (mo / mg), o, tol=2e-3)
    ratio, _, _ = E.check_planes(bad, out["weights_ref"]["wc"], out["valid"], c=E.C_WEIGHT, relative=True, half_ulp=False)
    assert ratio > 1000, ratio
    assert abs(float(bad[out["valid"]].max()) - 1.0) > 2 * 2.0 ** -23


def test_rejects_a_row_entry_inside_the_golden_bar(qvga):
    """(c) one entry of A moved by 1e-6 of its column's largest entry: inside the 5e-6 of test_golden.check_lin_planes_single_level,
    beyond C_ROW_A u of the entry's own terms. The entry is the one of median magnitude in column 3; the share of all entries
    for which the same move is rejected is printed."""
    s, out = qvga
    Ar, Br, xyd = out["rows_ref"]
    A, B = s.jacobian_rows()
    colmax = np.abs(A).max(0)
    r = int(np.argsort(np.abs(A[:, 3]))[A.shape[0] // 2])
    bad = A.astype(np.float64).copy()
    bad[r, 3] += 1e-6 * colmax[3]
    assert np.abs(bad - A).max(0)[3] <= 5e-6 * colmax[3]
    rA, _, at = E.check_rows(bad, B, Ar, Br, xyd)
    assert rA > 1.0 and at == (r, 3), (rA, at)
    bound = E.SECOND_ORDER * E.C_ROW_A * E.U32 * E.row_term_magnitudes(Ar, *xyd)
    print("share of A entries for which a move of 1e-6 of the column maximum leaves the bound: %.3f" % float((1e-6 * colmax[None, :] > 2 * bound).mean()))


def test_prior_check_and_a_dropped_pixel(ora):
    """(d) one non-Null pixel dropped from one cluster's prior (sum and count), chosen so that b_prior moves by less than the 2e-5
    of test_golden's tol_prior. With sums that are exact up to their final rounding (the oracle's exact_sums hook; the product's
    Q32.32 sums have the same order of bound) the check rejects it. With the reference's FLOAT sums it cannot: gamma_n sum |t| / n
    of a cluster of n ~ 4000 pixels is ~ 2e-4, ten times the move -- the float-order bound (the oracle as the reference runs it,
    ro_seg_prior) does not see one pixel, and this test asserts that it does not pretend to."""
    s = solve_pair(ora, 240, 320, driver_params(ora, debug_planes=1, max_iter_irls=1), SCENES["qvga_sphere"][3](), _hook(ora, "sfo_test_set_exact_sums", 1))
    out = report("qvga exact_sums", "oracle", linearisation_checks(s, "oracle", prior_path="fp64"))
    p = out["prior_ref"]
    l = int(np.argmax(np.where(p["full"], p["nonnull"], 0)))
    t = p["terms"][p["term_labels"] == l]
    n = t.size
    moved = (p["sum"][l] - t) / (n - 1) - p["sum"][l] / n  # b_prior's move for each candidate pixel
    ok = np.abs(moved) < 2e-5
    k = int(np.argmax(np.where(ok, np.abs(moved), 0.0)))
    assert ok[k] and -1.0 < p["b_prior"][l] < 2.0
    bad = float(np.float32(p["sum"][l] - t[k]) / np.float32(n - 1))
    d = abs(bad - p["b_prior"][l])
    assert d < 2e-5
    print("cluster %d, %d pixels: dropped pixel moves b_prior by %.3g; bounds fp64 %.3g, integer %.3g, float order %.3g"
          % (l, n, d, p["bound"]["fp64"][l], p["bound"]["integer"][l], p["bound"]["float"][l]))
    assert d > p["bound"]["fp64"][l] + 0.5 * E.ulp32(p["b_prior"][l]) and d > p["bound"]["integer"][l] + 0.5 * E.ulp32(p["b_prior"][l])
    assert d < p["bound"]["float"][l], "the float-order bound now rejects a dropped pixel: update the docstring"


# ------------------------------------------------------------------------------------------------------------------------------
#  GPU part
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["throughput", "latency"])
def ro(request):
    import staticfusion_amd as sf

    lib = os.path.join(os.path.dirname(sf.LIB), "libsf_hip_reforder.so")
    api = sf.Api(lib, "sf_").with_variant(request.param)
    assert api.backend_name() == "hip:gfx950:reference-order"
    return api


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_hip_linearisation_against_exact_references(hip, name):
    report(name, hip.default_variant, linearisation_checks(solve(hip, name), hip.default_variant))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_reference_order_linearisation_against_exact_references(ro, name):
    report(name, "reforder", linearisation_checks(solve(ro, name), "reforder"))


@pytest.mark.gpu
@pytest.mark.parametrize("seg", [False, True])
def test_hip_linearisation_of_the_irls_scene(hip, seg):
    report("irls_solver seg=%d" % seg, hip.default_variant, linearisation_checks(irls_solver(hip, seg, True), hip.default_variant))


@pytest.mark.gpu
def test_hip_prior_takes_both_branches(hip):
    starved_checks(hip, hip.default_variant)


@pytest.mark.gpu
def test_reference_order_prior_takes_both_branches(ro):
    starved_checks(ro, "reforder")


@pytest.mark.gpu
def test_hip_points_behind_the_camera(hip):
    s = solve_pair(hip, 120, 160, driver_params(hip, debug_planes=1), _near_patch_pair())
    out = report("behind_camera", hip.default_variant, linearisation_checks(s, hip.default_variant))
    assert out["n_behind"] > 0, "the last outer iteration has no pixel behind the camera"


@pytest.mark.gpu
def test_reference_order_points_behind_the_camera(ro):
    s = solve_pair(ro, 120, 160, driver_params(ro, debug_planes=1), _near_patch_pair())
    out = report("behind_camera", "reforder", linearisation_checks(s, "reforder"))
    assert out["n_behind"] > 0, "the last outer iteration has no pixel behind the camera"


@pytest.mark.gpu
def test_hip_first_iteration(hip):
    pr = make_pair(seed=9, sphere=True, out_rows=120, out_cols=160)
    s = solve_pair(hip, 120, 160, config2_params(hip, levels=1, max_iter_per_level=1, debug_planes=1), pr)
    report("first", hip.default_variant, linearisation_checks(s, hip.default_variant, expect_first=True))


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", SWEEP)
def test_hip_strip_edge_geometries(hip, rows, cols):
    """solve_linearise_strips<true, false, false> at level-0 sizes around its strip edges and with short / uneven column segments
    (cluster build: the LDS tiles of solve_linearise; every size but 125 x 96 is at or below SF_CLUSTER_SOLO_PIXELS = 8192, where
    each workgroup of the cluster runs the level on its own). The whole sweep takes about a second per build: nothing is thinned."""
    report("%dx%d" % (rows, cols), hip.default_variant, linearisation_checks(sweep_solver(hip, rows, cols), hip.default_variant))


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", SWEEP)
def test_reference_order_strip_edge_geometries(ro, rows, cols):
    report("%dx%d" % (rows, cols), "reforder", linearisation_checks(sweep_solver(ro, rows, cols), "reforder"))


@pytest.mark.gpu
def test_hip_global_maxima_with_a_zero_linearisation_error(hip):
    flat_patch_checks(hip, hip.default_variant)


@pytest.mark.gpu
def test_reference_order_global_maxima_with_a_zero_linearisation_error(ro):
    flat_patch_checks(ro, "reforder")


def _trace_bytes(st):
    return [bytes(st.outer[i]) for i in range(st.n_outer)]


def debug_planes_off_against_on(api, rows, cols, params_of, pr):
    """the shipping instantiation (debug_planes = 0: no Null / Warped / Inter stores, dct = 0 outside validPixels) against the one
    every plane test runs, on the same input: everything either of them computes must be identical"""
    runs = []
    for dbg in (1, 0):
        s = solve_pair(api, rows, cols, params_of(api, dbg), pr)
        s.build_segm_image()
        runs.append(s)
    on, off = runs
    st_on, st_off = on.stats(), off.stats()
    assert (st_on.n_outer, st_on.n_irls, st_on.status) == (st_off.n_outer, st_off.n_irls, st_off.status)
    assert _trace_bytes(st_on) == _trace_bytes(st_off)
    assert np.array_equal(on.T(), off.T()) and np.array_equal(on.twist(), off.twist())
    assert np.array_equal(on.b(), off.b()) and np.array_equal(on.b_image(), off.b_image())
    lin_on, lin_off = ({k: s.lin_plane(w) for k, w in LIN.items()} for s in runs)
    # ddt = dn - |stored dw| (the magnitude, dn being the same plane), wd > 0 <=> stored dw > 0 (the sign: validPixels)
    for k in ("dcu", "dcv", "ddu", "ddv", "ddt", "wc", "wd"):
        assert np.array_equal(lin_on[k], lin_off[k]), k
    valid = lin_on["wd"] > 0
    assert int(valid.sum()) == st_on.outer[st_on.n_outer - 1].n_valid
    assert np.array_equal(lin_on["dct"][valid], lin_off["dct"][valid])
    assert np.all(lin_off["dct"][~valid] == 0.0) and np.any(lin_on["dct"][~valid] != 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["qvga_seg", "qvga_odometry", "first_126x10"])
def test_hip_debug_planes_off_against_on(hip, case):
    if case == "qvga_seg":
        debug_planes_off_against_on(hip, 240, 320, lambda a, d: driver_params(a, debug_planes=d), SCENES["qvga_sphere"][3]())
    elif case == "qvga_odometry":
        debug_planes_off_against_on(hip, 240, 320, lambda a, d: config2_params(a, levels=3, debug_planes=d), SCENES["qvga_sphere"][3]())
    else:
        pr = make_pair(seed=126010, sphere=False, out_rows=126, out_cols=10, xi=SWEEP_XI)
        debug_planes_off_against_on(hip, 126, 10, lambda a, d: config2_params(a, levels=1, max_iter_per_level=1, debug_planes=d), pr)


@pytest.mark.gpu
def test_reference_order_debug_planes_off_against_on(ro):
    debug_planes_off_against_on(ro, 240, 320, lambda a, d: driver_params(a, debug_planes=d), SCENES["qvga_sphere"][3]())


@pytest.mark.gpu
def test_hip_batch_of_eight_streams(hip):
    """eight different pairs in one handle, every stream checked. The one-workgroup builds give stream b the record slot b
    (sf_frame_kernels.hip: cluster_init(..., b, b, ...)) and the cluster build the shared slot b or a private one recorded in
    last_slot, so every stream's records survive the launch at any batch size; eight stays inside the cluster build's limit."""
    rows, cols = 120, 160
    pairs = [make_pair(seed=300 + b, sphere=bool(b % 2), out_rows=rows, out_cols=cols) for b in range(8)]
    s = make_solver(hip, rows, cols, driver_params(hip, debug_planes=1), None, batch=8)
    for b, pr in enumerate(pairs):
        s.set_current(b, *pr["new"])
        s.set_prediction(b, *pr["old"])
    s.build_pyramid(True)
    s.run_solver(True)
    for b in range(8):
        report("batch stream %d" % b, hip.default_variant, linearisation_checks(s, hip.default_variant, stream=b))
    assert len({bytes(s.stats(b).outer[0]) for b in range(8)}) == 8, "the streams did not get different inputs"
