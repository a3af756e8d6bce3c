"""The warp splat, the IRLS normal equations, the 6 x 6 solve, the velocity filter, the SE(3) update and the b-solve against EXACT
fp64 references (tests/exact_ref.py), each stage recomputed from the inputs the implementation gave it, each held to the rounding
bound a correct float implementation must meet -- not to the distance from the float oracle.

CPU part: the oracle (liboracle.so) meets every bound, which validates references and tolerances; the same checks reject
perturbed oracle outputs that the suite's loose plane comparison (`assert_planes_close`) accepts.
GPU part (marked one by one: the CPU part shares the file): every build of the frame kernel (`hip` fixture) and the
reference-order build libsf_hip_reforder.so.

Summation paths of the warp (exact_ref.warp_bounds): the product sums levels of more than SF_ORDERED_SPLAT_MAX_PIXELS = 2048
pixels in exact fixed point and the smaller ones in the reference's float order (every build: the cluster build runs such levels
on one workgroup); the reference-order build and the oracle take the float order everywhere.
"""
import os

import numpy as np
import pytest

import exact_ref as E
from conftest import config2_params, driver_params, make_solver
from staticfusion_amd import _capi as capi
from staticfusion_amd.synth import Scene, make_pair, quantise_and_decimate, se3_exp

ORDERED_MAX_PIXELS = 2048  # SF_ORDERED_SPLAT_MAX_PIXELS (staticfusion_amd/csrc/sf_reforder.h)


# ------------------------------------------------------------------------------------------------------------------------------
#  scenes (the suite's recipes)
# ------------------------------------------------------------------------------------------------------------------------------
def _pair_scene(seed, rows, cols, sphere=True, xi=None):
    kw = {} if xi is None else {"xi": xi}
    return make_pair(seed=seed, sphere=sphere, out_rows=rows, out_cols=cols, **kw)


def _fence():
    """test_gpu_parity.py::test_warp_with_targets_outside_the_tile_windows"""
    pr = _pair_scene(21, 240, 320, sphere=False, xi=(0.05, 0.0, 0.0, 0.0, 0.0, 0.0))
    d_old = pr["old"][0].copy()
    patch = np.zeros((240, 320), bool)
    patch[90:150, 130:190] = True
    patch &= ((np.arange(320) // 3) % 2 == 0)[None, :]
    d_old[patch] *= 0.3
    return {"new": pr["new"], "old": (d_old, pr["old"][1])}


def _first_touch():
    """test_gpu_edge_rules.py::test_first_touch_splat_on_odd_geometry: frames 0 -> 1 of its sequence"""
    rows, cols = 200, 264
    scene = Scene(seed=31, sphere=True)
    xi = np.array((0.010, -0.005, 0.008, 0.03, -0.006, 0.003))
    frames, T = [], np.eye(4)
    for k in range(2):
        d, i = quantise_and_decimate(*scene.render(T, 2 * cols, 2 * rows, sphere_offset=(0.02 * k, 0, 0)))
        d = d.copy()
        d[:, 96:144] = 0
        d[0:120, 208:232] = 0
        frames.append((d, i))
        T = T @ se3_exp(xi)
    return {"new": frames[1], "old": frames[0]}


def _partial_wave(rows, cols):
    """test_gpu_parity.py::partial_wave_pair"""
    pr = _pair_scene(5, rows, cols)
    d_new = pr["new"][0].copy()
    d_new[-3:, -1] = 0
    return {"new": (d_new, pr["new"][1]), "old": pr["old"]}


def _tiny():
    """test_gpu_edge_rules.py::test_tiny_images_take_the_ordered_splat_at_every_level: frames 0 -> 1"""
    rows, cols = 32, 48
    scene = Scene(seed=41, sphere=True)
    xi = np.array((0.006, -0.004, 0.005, 0.01, -0.004, 0.003))
    f0 = quantise_and_decimate(*scene.render(np.eye(4), 2 * cols, 2 * rows))
    f1 = quantise_and_decimate(*scene.render(se3_exp(xi), 2 * cols, 2 * rows, sphere_offset=(0.02, 0, 0)))
    return {"new": f1, "old": f0}


# name -> (rows, cols, params(api), pair factory, checked levels, minimum coverage per checked level). The coverage floors sit
# a few per cent under what the oracle reaches (it depends on the geometry only: which sources land near a centi-pixel edge).
SCENES = {
    "qvga_sphere": (240, 320, lambda a: driver_params(a, debug_planes=1), lambda: _pair_scene(11, 240, 320), range(4),
                    (0.84, 0.91, 0.92, 0.94)),
    "picket_fence": (240, 320, lambda a: driver_params(a, debug_planes=1), _fence, range(4), (0.86, 0.9, 0.93, 0.96)),
    "roll_0.3": (240, 320, lambda a: driver_params(a, debug_planes=1), lambda: _pair_scene(17, 240, 320, xi=(0, 0, 0, 0, 0, 0.3)),
                 range(4), (0.84, 0.9, 0.93, 0.93)),
    "first_touch_200x264": (200, 264, lambda a: driver_params(a, kb=1.5, ctf_levels=3, debug_planes=1), _first_touch, range(2),
                            (0.85, 0.91)),
    "wave_40x42": (40, 42, lambda a: driver_params(a, kb=1.5, ctf_levels=3, debug_planes=1), lambda: _partial_wave(40, 42),
                   range(2), (0.94, 0.94)),
    "wave_20x52": (20, 52, lambda a: driver_params(a, kb=1.5, ctf_levels=2, debug_planes=1), lambda: _partial_wave(20, 52),
                   range(1), (0.96,)),
    "odd_48x43": (48, 43, lambda a: config2_params(a, levels=2, debug_planes=1), lambda: _pair_scene(6, 48, 43, sphere=False),
                  range(1), (0.95,)),
    "vga_6_levels": (480, 640, lambda a: driver_params(a, debug_planes=1), lambda: _pair_scene(5, 480, 640), range(5),
                     (0.73, 0.84, 0.9, 0.94, 0.96)),
    "tiny_32x48": (32, 48, lambda a: driver_params(a, kb=1.5, ctf_levels=2, debug_planes=1), _tiny, range(1), (0.95,)),
}
_scene_cache = {}


def scene_pair(name):
    if name not in _scene_cache:
        _scene_cache[name] = SCENES[name][3]()
    return _scene_cache[name]


def solve(api, name, batch=1):
    rows, cols, mk, _, _, _ = SCENES[name]
    s = make_solver(api, rows, cols, mk(api), scene_pair(name), batch=batch)
    s.build_pyramid(True)
    s.run_solver(True)
    return s


def tan_half_fovh(s):
    return float(np.tan(np.float32(0.5) * np.float32(s.params.fovh)))


def ordered_levels(kind, s):
    """image levels whose splat sums in the reference's float order: all of them for the oracle / reference-order build"""
    return {L for L in range(s.levels) if kind in ("oracle", "reforder") or np.prod(s.level_shape(L)) <= ORDERED_MAX_PIXELS}


def warp_checks(s, kind, name, stream=0):
    """(level, exact reference, failures, stats) of every checked level: the reference warps the PRED planes with the T_odometry
    that solve_warp read -- the trace's T of the outer iteration before the level's last one (sf_warp.h: solve_warp)."""
    _, _, _, _, levels, _ = SCENES[name]
    st = s.stats(stream)
    lv = np.array([st.outer[i].level for i in range(st.n_outer)])
    ordered = ordered_levels(kind, s)
    out = []
    for L in levels:
        j = int(np.nonzero(lv == s.levels - 1 - L)[0][-1])
        assert j > 0, "level %d's last iteration ran on Warped := Pred: choose another level" % L
        T = E.cm_to_mat(st.outer[j - 1].T)
        src = [s.plane(capi.SET_PRED, ch, L, stream) for ch in range(4)]
        ref = E.warp_reference(*src, T, tan_half_fovh(s))
        # preconditions of the bounds (the fixed-point conversions clamp depth to +-1000 and intensity to +-4)
        assert ref["min_depth_w_margin"] > 0 and ref["max_depth_w"] < 1000.0, (L, ref["min_depth_w_margin"], ref["max_depth_w"])
        assert 0.0 <= ref["min_intensity"] and ref["max_intensity"] <= 1.0, L
        fails, stats = E.check_warp(ref, s.plane(capi.SET_WARPED, capi.CH_DEPTH, L, stream),
                                    s.plane(capi.SET_WARPED, capi.CH_INTENSITY, L, stream), ordered=L in ordered)
        stats["ordered"] = L in ordered
        out.append((L, ref, fails, stats))
    return out


def assert_warps_exact(s, kind, name, stream=0):
    floors = SCENES[name][5]
    report = []
    for (L, ref, fails, stats), floor in zip(warp_checks(s, kind, name, stream), floors):
        report.append((L, round(stats["coverage"], 4), round(max(stats["ratio_depth"], stats["ratio_intensity"]), 3), stats["max_count"]))
        assert not fails, (name, kind, L, stats, fails)
        assert stats["coverage"] >= floor, ("coverage", name, L, stats)
    print("warp %s %s: (level, coverage, max |got - exact| / bound, max contributions)" % (name, kind), report)
    return report


# ------------------------------------------------------------------------------------------------------------------------------
#  B / C: one IRLS iteration per outer iteration, every stage from the implementation's own inputs
# ------------------------------------------------------------------------------------------------------------------------------
TWIST_OLD = np.array([0.004, -0.003, 0.002, 0.001, -0.002, 0.0015], np.float32)


def _plane_texture_pair(rows=120, cols=160):
    """a fronto-parallel plane at 2 m with a texture that varies along u only: the normal equations are near-singular"""
    u = np.arange(cols)[None, :].repeat(rows, 0).astype(np.float64)
    d = np.full((rows, cols), 2.0, np.float32)
    i_new = (0.5 + 0.3 * np.sin(u * 0.3)).astype(np.float32)
    i_old = (0.5 + 0.3 * np.sin((u + 0.4) * 0.3)).astype(np.float32)
    return {"new": (d, i_new), "old": (d.copy(), i_old)}


def irls_solver(api, seg, motion_filter, texture=False):
    if texture:
        rows, cols, pr = 120, 160, _plane_texture_pair()
    else:
        rows, cols, pr = 240, 320, _pair_scene(11, 240, 320)
    p = driver_params(api, debug_planes=1, max_iter_irls=1, segmentation_enabled=int(seg), use_motion_filter=int(motion_filter))
    s = make_solver(api, rows, cols, p, pr)
    s.set_twist_old(0, TWIST_OLD)
    s.build_pyramid(True)
    s.run_solver(True)
    return s


def irls_inputs(s):
    """the last outer iteration's rows, valid pixels, labels and the b its single IRLS iteration weighted with"""
    st = s.stats()
    j = st.n_outer - 1
    tr = st.outer[j]
    L = s.levels - 1 - tr.level
    A, B = s.jacobian_rows()
    nul = s.lin_plane(capi.LIN_NULL)
    inner = np.zeros(nul.shape, bool)
    inner[1:-1, 1:-1] = True  # validPixels: Null == 0 off the image border (reference FrontEnd.cpp:526-545)
    valid = ((nul == 0) & inner).T.ravel()
    assert valid.sum() == tr.n_valid and A.shape[0] == 2 * tr.n_valid, (valid.sum(), tr.n_valid, A.shape)
    seg = s.params.segmentation_enabled != 0
    lab = s.labels(L).T.ravel()[valid] if seg else np.zeros(int(valid.sum()), np.int64)
    if not seg:
        b = np.ones(24)
    elif tr.level == 0:  # the coarsest level starts every outer iteration from the prior (reference FrontEnd.cpp:603-604)
        b = np.array(tr.b_prior, np.float64)
    else:
        b = np.array(st.outer[j - 1].b_segm, np.float64)
    xyd = [s.plane(capi.SET_INTER, ch, L).T.ravel()[valid] for ch in (capi.CH_XX, capi.CH_YY, capi.CH_DEPTH)]
    T_prev = E.cm_to_mat(st.outer[j - 1].T) if j > 0 else np.eye(4)
    return dict(st=st, j=j, tr=tr, A=A.astype(np.float64), B=B.astype(np.float64), lab=lab, b=b, xyd=xyd, T_prev=T_prev)


def check_normal_equations(s, inp, perturb=None):
    """-> (max ratio over AtA, max ratio over AtB); perturb(AtA, AtB, bound) may edit copies of the implementation's values"""
    w, aver = E.irls_weights(inp["B"], np.repeat(inp["b"][inp["lab"]], 2), s.params.kc_Cauchy)
    sm = E.row_term_magnitudes(inp["A"], *inp["xyd"])
    AtA, AtB, bA, bB = E.normal_equations(inp["A"], inp["B"], w, sm)
    gA = np.array(inp["tr"].AtA, np.float64).reshape(6, 6)
    gB = np.array(inp["tr"].AtB, np.float64)
    if perturb is not None:
        perturb(gA, gB, AtA, bA)
    return float((np.abs(gA - AtA) / bA).max()), float((np.abs(gB - AtB) / bB).max()), aver


def filter_reference(s, inp):
    """twist_level of the last outer iteration from the implementation's AtA, var and rows, with the bound on it: the filter's
    inputs carry the float evaluation of ||A var - B||^2 (per row c u (sum |a_k var_k| + |B|)) and the implementation's inverse of
    AtA (double, from the float AtA: c u kappa); the output is float (1 ulp)."""
    tr = inp["tr"]
    var = np.array(tr.var, np.float64)
    res = inp["A"] @ var - inp["B"]
    e_r = 32 * E.U32 * (np.abs(inp["A"]) @ np.abs(var) + np.abs(inp["B"]))
    sq = res @ res
    e_sq = 2 * np.abs(res) @ e_r + e_r @ e_r + E.gamma(64) * sq
    if not s.params.use_motion_filter:
        tl, tol = var, np.zeros(6)
    else:
        tl, info = E.velocity_filter(tr.AtA, sq, var, TWIST_OLD, inp["T_prev"], tr.level, s.params.previous_speed_eig_weight,
                                     s.params.previous_speed_const_weight)
        # dW = cf dC, |dC| <= |C| (e_sq / sq + 64 u kappa); d tl = (I + W)^-1 dW (old - tl)
        dC = np.linalg.norm(info["C"], 2) * (e_sq / sq + 64 * E.U32 * info["cond"])
        M = np.linalg.inv(np.eye(6) + info["W"])
        tol = np.linalg.norm(M, 2) * info["cf"] * dC * np.linalg.norm(info["old"] - tl) + 64 * E.U32 * (
            np.abs(M) @ (np.abs(var) + np.abs(info["W"]) @ np.abs(info["old"])))
    return tl, tol + E.ulp32(tl) + 1e-15


def update_checks(s, inp):
    """-> (|twist_level - exact| / bound, |T - exp(twist_level) T_prev| / bound, |twist - log T| / bound): maxima"""
    tr = inp["tr"]
    tl, tol = filter_reference(s, inp)
    r_tl = float((np.abs(np.array(tr.twist_level, np.float64) - tl) / tol).max())
    Eexp = E.se3_exp(np.array(tr.twist_level, np.float64))
    T = Eexp @ inp["T_prev"]
    # float E (rounded from double) times float T_prev with float sums of 4 products: gamma_5 |E| |T_prev| entrywise
    bT = E.gamma(5) * (np.abs(Eexp) @ np.abs(inp["T_prev"])) + 1e-15
    r_T = float((np.abs(E.cm_to_mat(tr.T) - T) / bT).max())
    Tf = s.T().astype(np.float64)
    tw = E.se3_log(Tf)
    r_tw = float((np.abs(s.twist().astype(np.float64) - tw) / (E.ulp32(tw) + 1e-12 + 16 * E.U32 * 1e-6)).max())
    return r_tl, r_T, r_tw


def b_solve_check(s, inp):
    """the b-solve of the last outer iteration from the implementation's own rows and solution: -> (exact b, bound, got b)"""
    tr = inp["tr"]
    var = np.array(tr.var, np.float64)
    A, B = inp["A"], inp["B"]
    r = A @ var - B
    e_r = 32 * E.U32 * (np.abs(A) @ np.abs(var) + np.abs(B))
    pair_abs = np.abs(r[0::2]) + np.abs(r[1::2])
    means, counts = E.label_means(pair_abs, inp["lab"])
    e_means = np.bincount(inp["lab"], weights=e_r[0::2] + e_r[1::2], minlength=24)[:24] / (2.0 * (counts + 1))
    e_means += E.gamma(64) * means  # the float (or fixed-point) per-label sums
    aro = np.abs(B).sum() / B.size  # aver_res before the iteration (reference :590)
    p = s.params
    args = (np.array(tr.b_prior, np.float64), np.array(tr.lambda_t_w, np.float64), s.connectivity(), p.kb, p.kc_Cauchy, p.lambda_prior,
            p.lambda_reg)
    b, x = E.b_solve(means, aro, *args)
    # d b / d (label means, aver_res_old) by central differences of the reference (the clamp is 1-Lipschitz)
    tol = np.zeros(24)
    for l in range(25):
        h = 1e-6 * max(abs(means[l]) if l < 24 else aro, 1e-9)
        mp, mm, ap, am = means.copy(), means.copy(), aro, aro
        if l < 24:
            mp[l] += h
            mm[l] -= h
            e = e_means[l]
        else:
            ap, am = aro + h, aro - h
            e = E.gamma(8) * aro
        dx = (E.b_solve(mp, ap, *args)[1] - E.b_solve(mm, am, *args)[1]) / (2 * h)
        tol += np.abs(dx) * e
    # the float system itself: the data term's logs and products and a float LDL^T of the 24 x 24 system, c u (|x| + 1)
    tol += 64 * E.U32 * (np.abs(x) + 1.0) + E.ulp32(b)
    return b, tol, np.array(tr.b_segm, np.float64)


# ------------------------------------------------------------------------------------------------------------------------------
#  CPU part: the oracle meets every bound; the checks reject what the loose comparisons accept
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_oracle_warp_meets_the_exact_sums(ora, name):
    s = solve(ora, name)
    assert_warps_exact(s, "oracle", name)


@pytest.mark.parametrize("seg,mf", [(False, True), (True, True), (True, False)])
def test_oracle_irls_stages_meet_the_exact_references(ora, seg, mf):
    s = irls_solver(ora, seg, mf)
    inp = irls_inputs(s)
    rA, rB, _ = check_normal_equations(s, inp)
    r, bound = E.solve_residual(inp["tr"].AtA, inp["tr"].AtB, inp["tr"].var)
    r_tl, r_T, r_tw = update_checks(s, inp)
    assert max(rA, rB, r / bound, r_tl, r_T, r_tw) <= 1.0, (rA, rB, r / bound, r_tl, r_T, r_tw)
    if seg:
        b, tol, got = b_solve_check(s, inp)
        assert np.all(np.abs(got - b) <= tol), (np.abs(got - b) / tol).max()


def test_oracle_near_singular_solve(ora):
    s = irls_solver(ora, False, False, texture=True)
    tr = s.stats().outer[s.stats().n_outer - 1]
    assert np.all(np.isfinite(tr.var))
    assert np.linalg.cond(np.array(tr.AtA, np.float64).reshape(6, 6)) > 1e4, "the texture scene is not near-singular"
    r, bound = E.solve_residual(tr.AtA, tr.AtB, tr.var)
    assert r <= bound, (r, bound)


def _assert_planes_close_accepts(g, o):
    from test_gpu_parity import assert_planes_close

    assert_planes_close(g, o)


def test_warp_check_rejects_what_the_plane_comparison_accepts(ora):
    """one contribution removed from one warped cell / one tap weight off by one: the existing tolerance passes both, the exact
    check fails both"""
    s = solve(ora, "qvga_sphere")
    L = 0
    (_, ref, fails, _), = [c for c in warp_checks(s, "oracle", "qvga_sphere") if c[0] == L]
    assert not fails
    got_d = s.plane(capi.SET_WARPED, capi.CH_DEPTH, L)
    got_i = s.plane(capi.SET_WARPED, capi.CH_INTENSITY, L)
    # the contributions of every checked cell, through the reference's own taps
    st = s.stats()
    lv = np.array([st.outer[i].level for i in range(st.n_outer)])
    j = int(np.nonzero(lv == s.levels - 1 - L)[0][-1])
    T = E.cm_to_mat(st.outer[j - 1].T)
    src = [s.plane(capi.SET_PRED, ch, L) for ch in range(4)]
    one = E.warp_reference(*src, T, tan_half_fovh(s))
    W, SD = one["w"].astype(np.float64), one["depth"] * one["w"]
    bd, _ = E.warp_bounds(ref, ordered=True)
    # candidate perturbations of single cells: mean without one contributor of weight w and value d, mean with weight w + 1
    rows, cols = W.shape
    f, du, dv = E.warp_geometry(rows, cols, tan_half_fovh(s))
    depth = got_d.astype(np.float64)
    cand_removed = []
    Ti = np.linalg.inv(T).astype(np.float32).astype(np.float64)
    for u in range(1, cols - 1, 3):
        for v in range(1, rows - 1, 3):
            if not ref["checked"][v, u] or ref["count"][v, u] < 2:
                continue
            # one source near (v, u) that contributes to this cell: search the sources whose taps hit it
            cand_removed.append((v, u))
            if len(cand_removed) > 400:
                break
        if len(cand_removed) > 400:
            break
    # contributions: recompute taps of all sources and keep those that hit the candidate cells
    z = src[0].T.ravel().astype(np.float64)
    sel = z != 0
    pts = np.stack([src[2].T.ravel()[sel], src[3].T.ravel()[sel], z[sel], np.ones(int(sel.sum()))]).astype(np.float64)
    X, Y, D = (Ti[r] @ pts for r in range(3))
    uw = np.trunc(100 * (f * X / D + du)).astype(np.int64)
    vw = np.trunc(100 * (f * Y / D + dv)).astype(np.int64)
    ok = (uw >= 0) & (uw < 100 * (cols - 1)) & (vw >= 0) & (vw < 100 * (rows - 1))
    tv, tu, tw = E._taps(uw[ok], vw[ok])
    Dk = D[ok]
    want = set(cand_removed)
    best_rm, best_w = None, None
    for t in range(4):
        for k in np.nonzero(tw[t] > 0)[0]:
            cell = (int(tv[t][k]), int(tu[t][k]))
            if cell not in want:
                continue
            w, d = float(tw[t][k]), float(Dk[k])
            mean_rm = (SD[cell] - w * d) / (W[cell] - w)
            mean_w1 = (SD[cell] + d) / (W[cell] + 1)
            for val, best in ((mean_rm, "rm"), (mean_w1, "w1")):
                delta = abs(val - ref["depth"][cell])
                if delta > 0.2:
                    continue
                score = delta / bd[cell]
                if best == "rm" and (best_rm is None or score > best_rm[0]):
                    best_rm = (score, cell, val)
                if best == "w1" and (best_w is None or score > best_w[0]):
                    best_w = (score, cell, val)
    for score, cell, val in (best_rm, best_w):
        assert score > 10, (score, cell)
        bad = depth.copy()
        bad[cell] = val
        _assert_planes_close_accepts(bad.astype(np.float32), got_d)
        fails, _ = E.check_warp(ref, bad, got_i, ordered=True)
        assert fails, cell


def test_normal_equation_check_rejects_a_small_AtA_error(ora):
    """AtA[0, 3] moved by 1e-5 sqrt(a00 a33) -- inside the suite's twist bars -- is rejected"""
    s = irls_solver(ora, True, True)
    inp = irls_inputs(s)

    def nudge(gA, gB, AtA, bA):
        d = 1e-5 * np.sqrt(AtA[0, 0] * AtA[3, 3])
        gA[0, 3] += d
        gA[3, 0] += d

    rA, _, _ = check_normal_equations(s, inp, nudge)
    assert rA > 1.0, rA


def test_b_solve_check_rejects_a_moved_b(ora):
    """one b value moved by ten times its bound, or by 1e-4 if that is smaller, is rejected"""
    s = irls_solver(ora, True, True)
    inp = irls_inputs(s)
    b, tol, got = b_solve_check(s, inp)
    assert np.all(np.abs(got - b) <= tol)
    l = int(np.argmax(inp["tr"].lambda_t_w))
    moved = got.copy()
    moved[l] += min(10 * tol[l], 1e-4)
    assert tol[l] < 1e-4, "the b bound (%g) exceeds the suite's 1e-4 bar" % tol[l]
    assert np.abs(moved[l] - b[l]) > tol[l]
    print("b bounds: max %.3g, median %.3g" % (tol.max(), np.median(tol)))


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


GPU_SCENES = [n for n in sorted(SCENES) if n != "tiny_32x48"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_SCENES)
def test_hip_warp_against_exact_sums(hip, name):
    s = solve(hip, name)
    assert_warps_exact(s, hip.default_variant, name)
    if name == "picket_fence" and hip.default_variant != "cluster":
        assert s.splat_replays() > 0, "the scene did not exercise the replay path"
    if name == "roll_0.3" and hip.default_variant == "throughput":
        assert s.ordered_fallbacks() > 0, "no coarse level left its tile windows"


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_SCENES)
def test_reference_order_warp_against_exact_sums(ro, name):
    s = solve(ro, name)
    assert_warps_exact(s, "reforder", name)


@pytest.mark.gpu
def test_hip_warp_of_many_streams(hip_auto):
    """3000 streams of 32 x 48 on the throughput build (more than its resident workgroups: per-workgroup scratch of the ordered
    splat): the first, the last and a seeded sample of streams against the exact sums"""
    s = solve(hip_auto.with_variant("throughput"), "tiny_32x48", batch=3000)
    rng = np.random.default_rng(3000)
    for b in [0, 2999] + sorted(rng.choice(np.arange(1, 2999), 6, replace=False).tolist()):
        assert_warps_exact(s, "throughput", "tiny_32x48", stream=b)


@pytest.mark.gpu
@pytest.mark.parametrize("seg,mf", [(False, True), (True, True), (True, False)])
def test_hip_irls_stages_against_exact_references(hip, ora, seg, mf):
    s = irls_solver(hip, seg, mf)
    inp = irls_inputs(s)
    rA, rB, _ = check_normal_equations(s, inp)
    r, bound = E.solve_residual(inp["tr"].AtA, inp["tr"].AtB, inp["tr"].var)
    r_tl, r_T, r_tw = update_checks(s, inp)
    print("irls seg=%d mf=%d %s: |got - exact| / bound AtA %.3g AtB %.3g solve %.3g twist_level %.3g T %.3g twist %.3g"
          % (seg, mf, hip.default_variant, rA, rB, r / bound, r_tl, r_T, r_tw))
    assert max(rA, rB, r / bound, r_tl, r_T, r_tw) <= 1.0, (rA, rB, r / bound, r_tl, r_T, r_tw)
    if seg:
        b, tol, got = b_solve_check(s, inp)
        bo = irls_solver(ora, seg, mf).b()
        d_ho = np.abs(s.b().astype(np.float64) - bo)
        inside = float((d_ho <= tol).mean())
        msg = ("b: max |got - exact| / bound %.3g; HIP - oracle distance %.3g, share of labels whose HIP - oracle distance lies inside the "
               "float-evaluation bound: %.3f" % ((np.abs(got - b) / tol).max(), d_ho.max(), inside))
        print(msg)
        assert np.all(np.abs(got - b) <= tol), msg


@pytest.mark.gpu
def test_hip_near_singular_solve(hip):
    s = irls_solver(hip, False, False, texture=True)
    tr = s.stats().outer[s.stats().n_outer - 1]
    assert np.all(np.isfinite(tr.var))
    r, bound = E.solve_residual(tr.AtA, tr.AtB, tr.var)
    assert r <= bound, (r, bound)
