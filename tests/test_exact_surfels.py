"""The surfel drawing (staticfusion_amd/csrc/sf_surfel_geom.h: prediction, views, scores, alignment) and the prediction's
composition against EXACT fp64 references derived from the shaders (tests/surfel_ref.py, sections F and G) -- not against
another copy of the kernel's float arithmetic.

CPU part: the oracle's prediction and tests/view_ref.py meet F and G on every scene (tests/surfel_cases.py), every scene meets
its caps (the check must DECIDE: few pixels with several admissible winners, few open fragments), and F and G reject what the
restatements cannot see of themselves: view_ref.py with one line changed at a time.
GPU part (marked one by one; `hip_auto`: the drawing does not depend on the build of the frame kernel): sfv_render_surfels,
sfv_render_maps and sf_predict_from_model on the same scenes.

The caps: at most 1 drawn pixel in 20 with more than one admissible winner and at most 1 square fragment in 50 open; the grazing
and plane-crossing scenes state their own in surfel_cases.py (1 in 200 and 1 in 500: F decides nearly every fragment of theirs too)
and must still leave half of their certainly drawn pixels with a single admissible winner.
"""
import functools

import numpy as np
import pytest

import surfel_cases as sc
import surfel_ref as S
import view_cases as vc
import view_ref
from conftest import driver_params, make_solver
from staticfusion_amd import _capi as capi
from staticfusion_amd import view as sfview

MOVED = dict(vc.poses())["moved"]


# ------------------------------------------------------------------------------------------------------------------------------
#  scenes
# ------------------------------------------------------------------------------------------------------------------------------
def handle_intrinsics(api, rows, cols):
    s = make_solver(api, rows, cols, driver_params(api))
    mp = s.default_model_params()
    s.close()
    return mp


def frame_case(api, rows, cols, which):
    """view_cases.frame_surfels (a wavy wall, a nearer box: an occlusion edge, a hole) from the `moved` pose. The surfels of the
    box are coplanar to within the rounding of their positions (1e-7 m), less than any float evaluation of z can resolve: where
    several of them cover a pixel, each is an admissible winner. The confidences are uniform in [0, 0.6]; at a threshold of 0.35
    (0.25 in test_view_reference_cpu.py) few enough discs overlap for the scene to meet the cap of 1 ambiguous pixel in 20."""
    mp = handle_intrinsics(api, rows, cols)
    intr = dict(cx=mp.cx, cy=mp.cy, fx=mp.fx, fy=mp.fy)
    if which == "other":
        intr = vc.other_intrinsics(mp)
    elif which == "flipped":  # fy < 0, as VIEWS[1] of test_gpu_view.py
        intr = dict(cx=mp.cx + 1.75, cy=rows - mp.cy + 2.25, fx=mp.fx * 0.9, fy=-mp.fy * 1.1)
    return sc.Case("frame-%dx%d-%s" % (cols, rows, which), vc.frame_surfels(rows, cols, mp), rows, cols, pose=MOVED, min_confidence=0.35, tick=3, **intr)


FRAME_IDS = [(r, c, w) for r, c in vc.SIZES for w in ("default", "other", "flipped")]
PLAIN = {
    **{"tilts-%d-%s" % (n, "ordered" if o else "shuffled"): functools.partial(sc.tilts, n, o) for n in (511, 512, 513, 5003) for o in (True, False)},
    "crossing": sc.crossing, "crossing-32x32": sc.crossing_small, "large-in-front": functools.partial(sc.large_sprite, "in front"),
    "large-behind": functools.partial(sc.large_sprite, "behind"), "cull-thresholds": sc.cull_thresholds, "image-border": sc.image_border,
    "tiny-1x1": sc.tiny_image, "duplicates": sc.duplicates,
}
# the scenes a prediction draws too (sf_predict_splat_kernel: two targets, its own LDS tile and fallback): a handle of the
# scene's size, primed so that nothing is filled in. Not the 1 x 1, 32 x 32 and 64 x 32 images: no handle is that small.
HANDLE_SIZED = sorted(n for n in PLAIN if n.startswith(("tilts", "large", "duplicates"))) + ["crossing", "cull-thresholds"]


@functools.lru_cache(maxsize=None)
def plain_case(name):
    return PLAIN[name]()


_frame_cases = {}


def get_frame_case(api, rows, cols, which):
    if (rows, cols, which) not in _frame_cases:
        _frame_cases[rows, cols, which] = frame_case(api, rows, cols, which)
    return _frame_cases[rows, cols, which]


_refs = {}


def view_reference(case):
    """section F for the case drawn as a view (the age test of include/sf_view.h) -- computed once, never changed"""
    if case.name not in _refs:
        _refs[case.name] = S.draw_reference(case.surfels, case.pose, case.cx, case.cy, case.fx, case.fy, case.rows, case.cols, case.max_depth,
                                            case.min_confidence, time=case.tick, time_delta=case.max_age if case.max_age >= 0 else None, nan_age_culls=True)
    return _refs[case.name]


def prediction_reference(case, mp):
    """section F for the case drawn by one target of the prediction (the age tests of splat.vert:57)"""
    key = case.name + "/prediction"
    if key not in _refs:
        _refs[key] = S.draw_reference(case.surfels, case.pose, case.cx, case.cy, case.fx, case.fy, case.rows, case.cols, mp.max_depth, mp.conf_high,
                                      time=mp.time, time_delta=mp.time_delta, max_time=mp.max_time)
    return _refs[key]


def view_of(case, **over):
    kw = dict(pose=case.pose, cx=case.cx, cy=case.cy, fx=case.fx, fy=case.fy, rows=case.rows, cols=case.cols, min_confidence=case.min_confidence,
              max_depth=case.max_depth, max_age=case.max_age)
    kw.update(over)
    return sfview.View(**kw)


def pure_params(s, case):
    mp = vc.pure_render_params(s, dict(cx=case.cx, cy=case.cy, fx=case.fx, fy=case.fy), case.min_confidence, case.max_depth, time=case.tick)
    if case.max_age >= 0:
        mp.time_delta = case.max_age
    assert mp.time_delta >= 0
    return mp


RECORD = {}  # (scene, implementation) -> the figures of the last check (run with -s to see them; tests/README.md quotes a run)


def check_caps(case, ref, stats, who):
    """the caps of the issue, per scene; and the floors: the scene draws, and decides"""
    RECORD[(case.name, who)] = stats
    print("%-28s %-10s drawn %5d  |got - exact| / bound %.3f  ambiguous %5d (%.4f, cap %.4f)  open %6d of %7d (%.4f, cap %.4f)" % (
        case.name, who, stats["drawn"], stats["ratio"], stats["ambiguous"], stats["ambiguous"] / max(stats["drawn"], 1), case.ambiguous_cap,
        stats["open_fragments"], stats["square_fragments"], stats["open_fragments"] / max(stats["square_fragments"], 1), case.open_cap))
    assert stats["drawn"] > 0
    assert stats["ambiguous"] <= case.ambiguous_cap * stats["drawn"], "ambiguous pixels"
    assert stats["open_fragments"] <= case.open_cap * stats["square_fragments"], "open fragments"
    assert 2 * stats["single_certain"] >= stats["certain_pixels"] > 0
    if case.kind == "grazing" and case.surfels.shape[0] > 5000:  # the grazing scene proper (surfel_cases.TILT_CAPS says why)
        assert stats["open_fragments"] > 0


def check_floors(case, ref, index):
    """what the scene is there for"""
    won = np.unique(index[index >= 0])
    if case.kind == "crossing":
        # every crossing disc has a corner at or behind the camera plane, and F certainly draws pixels outside the bounding
        # rectangle of its projected corners (as sf_surfel_geom.h widens it)
        for b in case.big:
            assert (ref.corner_z[b] - ref.corner_z_err[b] <= 0).any() and (ref.corner_z[b] + ref.corner_z_err[b] <= 0).any(), b
            xlo, xhi, ylo, yhi = (float(r.v[b]) for r in ref.corner_box)
            mine = ref.certain & (ref.s == b)
            i, j = ref.pix[mine] % ref.cols, ref.pix[mine] // ref.cols
            outside = (i < np.floor(xlo - 1.5)) | (i > np.ceil(xhi + 0.5)) | (j < np.floor(ylo - 1.5)) | (j > np.ceil(yhi + 0.5))
            assert outside.sum() > 0, b
        assert np.isin(case.big, won).all() and (~np.isin(won, case.big)).any()
    if case.name.startswith("large"):
        assert np.isin(case.big, won).all() and (~np.isin(won, case.big)).any() == (case.name == "large-behind")
    if case.name == "duplicates":
        assert (ref.first_of != np.arange(ref.n)).sum() == 128 and (np.bincount(ref.first_of[won], minlength=ref.n)[won] == 1).all()
        copies = np.flatnonzero(np.bincount(ref.first_of, minlength=ref.n) == 3)
        assert np.isin(copies, won).sum() >= 16  # the lowest copies do win pixels
    if case.name == "cull-thresholds":
        for k, exp in enumerate(case.expect):
            if exp is not None:
                assert ref.surfel_certain[k] == exp and ref.surfel_alive[k] == exp, k
        got = [bool((index[v - 1: v + 2, u - 1: u + 2] >= 0).any()) for u, v in case.spots]
        certain = [k for k, e in enumerate(case.expect) if e is not None and k not in case.open_by_nature]
        assert [got[k] for k in certain] == [case.expect[k] for k in certain]
        assert not ref.certain[np.isin(ref.s, case.open_by_nature)].any() and np.isin(case.open_by_nature, ref.s).all()
    if case.name == "image-border":
        assert list(ref.surfel_certain) == case.expect and list(ref.surfel_alive) == case.expect  # ndc is exact here: nothing open
        assert sorted(won) == [k for k, e in enumerate(case.expect) if e]
    if case.name == "tiny-1x1":
        assert index.shape == (1, 1) and index[0, 0] == 1  # the nearer, tilted one


# ------------------------------------------------------------------------------------------------------------------------------
#  CPU: view_ref and the oracle meet F
# ------------------------------------------------------------------------------------------------------------------------------
def _check_view_ref(case):
    ref = view_reference(case)
    got = view_ref.render(case.surfels, view_of(case), tick=case.tick)
    stats = S.check_drawing(ref, got["index"], got["depth"])
    check_caps(case, ref, stats, "view_ref")
    check_floors(case, ref, got["index"])
    return ref, got


@pytest.mark.parametrize("name", sorted(PLAIN))
def test_view_ref_meets_the_exact_drawing(name):
    _check_view_ref(plain_case(name))


def test_a_centre_one_ulp_outside_that_rounds_onto_the_border_is_open():
    ref = S.draw_reference(sc.border_ties(), np.eye(4), max_depth=20.0, conf_threshold=0.0, **sc.BORDER_VIEW)
    assert not ref.surfel_certain.any() and ref.surfel_alive.all() and ref.open_fragments > 0 and not ref.certain.any()
    got = view_ref.render(sc.border_ties(), sfview.View(np.eye(4), min_confidence=0.0, **sc.BORDER_VIEW), tick=sc.TICK)
    assert (got["index"] >= 0).any()  # the float ndc is 1: drawn
    S.check_drawing(ref, got["index"], got["depth"])
    S.check_drawing(ref, np.full((32, 64), -1), np.zeros((32, 64), np.float32))  # and not drawing it passes as well


@pytest.mark.parametrize("name", ["tilts-5003-shuffled", "crossing", "cull-thresholds", "large-behind"])
def test_the_tracker_stays_within_the_hand_counts(name):
    """the margins come from a running error bound; the counts written next to C_H, C_NV / C_NORMAL, C_RAY, C_NDC and C_DEPTH
    in surfel_ref.py bound it (C_PLANE and C_DISC are not held here)"""
    case = plain_case(name)
    ref = view_reference(case)
    u, slack, floor = S.U32, 1 + 1e-4, 16 * S.TINY
    with np.errstate(all="ignore"):
        ok = np.isfinite(ref.h_err).all(1) & np.isfinite(ref.h_mags).all(1)
        t_col = ref.t_err[12:15]  # the translation's own margin comes on top of the count
        assert np.all(ref.h_err[ok] <= (S.C_H * u * ref.h_mags[ok] + t_col) * slack + floor)
        if name == "cull-thresholds":
            assert not ref.h_err.any()  # the identity pose: h is exact
        # the normal
        q = ref.surfels
        Tm = np.abs(S.inverse_f32(case.pose).astype(np.float64))
        m = np.stack([Tm[i] * np.abs(q[:, 8]) + Tm[4 + i] * np.abs(q[:, 9]) + Tm[8 + i] * np.abs(q[:, 10]) for i in range(3)], 1)
        okn = np.isfinite(ref.nrm).all(1) & np.isfinite(ref.nrm_err).all(1)
        assert okn.sum() > 0.9 * len(okn) and np.all(ref.nv_err[okn] <= S.C_NV * u * m[okn] * slack + floor)
        norm = np.linalg.norm(ref.nv, axis=1, keepdims=True)
        bound = S.C_NV * u * m / norm + np.abs(ref.nrm) * (S.C_NV * u * (np.abs(ref.nv) * m).sum(1, keepdims=True) / norm ** 2 + 3.5 * u)
        assert np.all(ref.nrm_err[okn] <= bound[okn] * slack + floor)
        # the view ray
        assert np.all(ref.ray_err <= S.C_RAY * u * np.abs(ref.ray) * slack + floor)
        # ndc: five roundings on |f h.x / h.z| + |c| + w / 2, and what h brings
        for k, (f, c, w) in enumerate(((case.fx, case.cx, case.cols), (case.fy, case.cy, case.rows))):
            qk = np.abs(f * ref.h[:, k] / ref.h[:, 2])
            den = np.abs(ref.h[:, 2]) - ref.h_err[:, 2]
            from_h = (abs(f) * ref.h_err[:, k] + qk * ref.h_err[:, 2]) / den
            bound = (S.C_NDC * u * (qk + abs(c) + w / 2) + from_h * (1 + 8 * u)) / (w / 2)
            okk = ok & (den > 0) & np.isfinite(bound)
            assert okk.sum() > 0.9 * len(okk) and np.all(ref.ndc_err[okk, k] <= bound[okk] * slack + floor)
    zq = np.abs(ref.z) / (2 * ref.max_depth)
    assert np.all(ref.depth_err <= (ref.z_err / (2 * ref.max_depth) + S.C_DEPTH * u * (zq + np.abs(ref.depth))) * slack + floor)


def _check_prediction(s, case, who):
    mp = pure_params(s, case)
    ref = prediction_reference(case, mp)
    s.predict_from_model(0, case.surfels, case.pose, mp)
    d, inten = s.prediction()
    stats = S.check_prediction(ref, d, inten, mp.extract_max_depth)
    assert stats["drawn"] > 0
    RECORD[(case.name, who + " prediction")] = stats
    print("%-28s %-18s drawn %5d  |got - exact| / bound %.3f" % (case.name, who + " prediction", stats["drawn"], stats["ratio"]))
    return mp, ref, d, inten


@pytest.mark.parametrize("rows,cols,which", FRAME_IDS)
def test_frame_models_meet_the_exact_drawing_and_composition(ora, rows, cols, which):
    case = get_frame_case(ora, rows, cols, which)
    ref, drawn = _check_view_ref(case)
    assert (drawn["index"] >= 0).mean() > 0.5
    s = make_solver(ora, rows, cols, driver_params(ora))
    vc.prime_pure_render(s, rows, cols)
    mp, _, d, inten = _check_prediction(s, case, "oracle")
    # G on one target: nothing is filled in from the black previous frame, but its branch and its clip run
    dense, dg, ig = S.compose(drawn["index"], drawn["depth"], drawn["index"], drawn["depth"], case.surfels, s.input_image(capi.IN_DEPTH_FILTERED_MM),
                              s.input_image(capi.IN_COLOR), s.b_image(), mp.extract_max_depth)
    assert np.array_equal(dg, d) and np.array_equal(ig, inten) and dense == s.prediction_dense()
    s.close()


@pytest.mark.parametrize("name", HANDLE_SIZED)
def test_the_oracles_prediction_meets_the_exact_drawing(ora, name):
    case = plain_case(name)
    s = make_solver(ora, case.rows, case.cols, driver_params(ora))
    vc.prime_pure_render(s, case.rows, case.cols)
    _check_prediction(s, case, "oracle")
    s.close()


# ------------------------------------------------------------------------------------------------------------------------------
#  the composition (section G)
# ------------------------------------------------------------------------------------------------------------------------------
COMPOSITIONS = [  # rows, cols, surfels on sampled pixels, one more with a zero channel, dense
    (120, 160, 3, False, False), (120, 160, 4, False, True), (120, 160, 3, True, False), (60, 80, 0, False, False), (60, 80, 1, False, True),
    (60, 80, 0, True, False), (30, 40, 0, False, False)]
B_VALUES = np.array([0.1, np.nextafter(np.float32(0.6), np.float32(0)), 0.6, np.nextafter(np.float32(0.6), np.float32(1)), 0.9], np.float32)


def prime_composition(s, rows, cols):
    """a previous frame with every case of the fill-in: depths of 0, below and above extract_max_depth = 2 m, colours, and a b
    image with values on both sides of 0.6 and at it"""
    rng = np.random.default_rng(rows)
    mm = rng.integers(800, 3200, (rows, cols)).astype(np.uint16)
    mm[rng.random((rows, cols)) < 0.2] = 0
    rgb = rng.integers(1, 256, (rows, cols, 3)).astype(np.uint8)
    s.load_frame(0, np.repeat(np.repeat(rgb, 2, 0), 2, 1), np.repeat(np.repeat(mm, 2, 0), 2, 1), 2)
    s.filter_depth()
    labels = rng.integers(0, 24, (rows, cols)).astype(np.int32)
    s.set_segm_state(0, labels, np.resize(B_VALUES, 24), np.ones(24, np.float32))
    s.build_segm_image()


def composition_case(s, rows, cols, on_samples, zero_channel):
    mp = s.default_model_params()
    mp.time = mp.max_time = sc.TICK
    mp.extract_max_depth = 2.0
    assert mp.conf_low < 0.2 < mp.conf_high < 0.5 and mp.time_delta >= 0
    surf = sc.composition(rows, cols, mp, on_samples, S.sample_positions(120, 160) if rows < 40 else S.sample_positions(rows, cols), zero_channel)
    return mp, surf


def check_composition(s, mp, surf, targets, expect_dense):
    """targets: (index, depth) of the low and the high target, each already checked against F"""
    rows, cols = s.rows, s.cols
    (il, zl), (ih, zh) = targets
    filt, rgb, b = s.input_image(capi.IN_DEPTH_FILTERED_MM), s.input_image(capi.IN_COLOR), s.b_image()
    six = np.float32(0.6)
    assert (b < six).any() and (b == six).any() and (b > six).any() and (filt == 0).any() and (filt > 2000).any() and ((filt > 0) & (filt < 2000)).any()
    dense, dg, ig = S.compose(il, zl, ih, zh, surf, filt, rgb, b, mp.extract_max_depth)
    assert dense == expect_dense
    s.predict_from_model(0, surf, np.eye(4, dtype=np.float32), mp)
    d, inten = s.prediction()
    assert s.prediction_dense() == dense
    assert np.array_equal(d, dg) and np.array_equal(inten, ig)
    # what the scene is there for: black winners keep their depth, and take another colour
    black = S.decode_colour(surf[:, 4]).astype(int).sum(1) == 0
    bh, bl = (ih >= 0) & black[np.maximum(ih, 0)], (ih < 0) & (il >= 0) & black[np.maximum(il, 0)]
    assert bh.sum() >= 2 and bl.sum() >= 1 and np.all(d[bh] == zh[bh]) and np.all(d[bl] == zl[bl])
    over = (ih >= 0) & (il >= 0) & (ih != il) & bh  # a black high-confidence winner over a coloured low-confidence one
    assert over.any()
    low_col = S.grey_f32(S.decode_colour(surf[np.maximum(il, 0), 4]))
    prev_col = S.grey_f32(rgb)
    if dense:
        assert np.all(inten[over] == low_col[over]) and np.all(inten[bl] == 0)
    else:
        assert np.all(inten[over] == low_col[over]) and np.all(inten[bh & ~over] == prev_col[bh & ~over]) and np.all(inten[bl] == prev_col[bl])
        empty = (il < 0) & (ih < 0)
        fill = empty & (b > six) & (filt > 0) & (filt <= 2000)
        assert fill.any() and np.all(d[fill] > 0) and not d[empty & ~(b > six)].any() and not d[empty & (filt > 2000)].any()
    assert (zh > np.float32(2.0)).any() and not d[zh > np.float32(2.0)].any()  # the extraction clip on a drawn pixel
    return dense, dg, ig


def composition_targets(case_views, render):
    """both targets from a renderer of views, each checked against F"""
    out = []
    for case in case_views:
        got = render(case)
        S.check_drawing(view_reference(case), got["index"], got["depth"])
        out.append((got["index"], got["depth"]))
    return out


def composition_views(mp, surf, rows, cols, tag):
    kw = dict(rows=rows, cols=cols, cx=mp.cx, cy=mp.cy, fx=mp.fx, fy=mp.fy, max_depth=mp.max_depth, max_age=mp.time_delta, tick=mp.time)
    return [sc.Case("composition-%s-%s" % (tag, lvl), surf, min_confidence=c, **kw) for lvl, c in (("low", mp.conf_low), ("high", mp.conf_high))]


@pytest.mark.parametrize("rows,cols,on_samples,zero_channel,expect_dense", COMPOSITIONS)
def test_the_oracles_composition_is_exact(ora, rows, cols, on_samples, zero_channel, expect_dense):
    s = make_solver(ora, rows, cols, driver_params(ora))
    prime_composition(s, rows, cols)
    mp, surf = composition_case(s, rows, cols, on_samples, zero_channel)
    views = composition_views(mp, surf, rows, cols, "%dx%d-%d%s" % (cols, rows, on_samples, "z" if zero_channel else ""))
    targets = composition_targets(views, lambda c: view_ref.render(c.surfels, view_of(c), tick=c.tick))
    dense, dg, ig = check_composition(s, mp, surf, targets, expect_dense)
    total = S.dense_enough(np.where((targets[0][0] >= 0)[..., None], S.decode_colour(surf[np.maximum(targets[0][0], 0), 4]), 0).astype(np.uint8))[1]
    assert total == on_samples and S.sample_positions(rows, cols).shape[0] == (cols // 40) * (rows // 40)
    # ---- rejections: compositions that misread the reference in one place (surfel_ref.WRONG), run on the same inputs and held
    # against the oracle's output as G is: np.array_equal fails where the scene can tell, and only there ----
    filt, rgb, b = s.input_image(capi.IN_DEPTH_FILTERED_MM), s.input_image(capi.IN_COLOR), s.b_image()
    (il, zl), (ih, zh) = targets
    d, inten = s.prediction()
    seen = {}
    for w in S.WRONG:
        _, dw, iw = S.compose(il, zl, ih, zh, surf, filt, rgb, b, mp.extract_max_depth, wrong=(w,))
        seen[w] = not (np.array_equal(dw, d) and np.array_equal(iw, inten))
    print("%d x %d, %d on samples%s: %s" % (cols, rows, on_samples, " + zero channel" if zero_channel else "", seen))
    assert seen[S.WRONG[0]] == (rows == 120 and on_samples == 3)  # the quotient is 0.25 itself at 3 of 12, nowhere else
    assert seen[S.WRONG[1]] == expect_dense  # texel i * 40 sees none of the surfels on the samples: "not dense" always
    assert seen[S.WRONG[2]]  # every scene has black winners with z != 0 and undrawn pixels next to coloured ones
    s.close()


# ------------------------------------------------------------------------------------------------------------------------------
#  rejections: view_ref.py with one line changed at a time (CPU)
# ------------------------------------------------------------------------------------------------------------------------------
def _render(case):
    return view_ref.render(case.surfels, view_of(case), tick=case.tick)


def _rejected(case):
    got = _render(case)
    try:
        S.check_drawing(view_reference(case), got["index"], got["depth"])
    except S.DrawingMismatch as e:
        return str(e)
    return None


def test_the_corner_rectangle_of_before_is_rejected_on_the_crossing_scene(monkeypatch):
    for name in ("crossing", "crossing-32x32"):
        case = plain_case(name)
        good = _render(case)
        monkeypatch.setattr(view_ref, "_corner_rectangle_applies", lambda corners: True)
        why = _rejected(case)
        lost = int(((good["index"] >= 0) & (_render(case)["index"] < 0)).sum())
        monkeypatch.undo()
        print("%s: the unconditional corner rectangle loses %d pixels: %s" % (name, lost, why))
        assert why is not None and "certainly drawn pixel is empty" in why and lost > 0
        assert _rejected(case) is None
    # every other scene keeps its pixel set with or without the rule: no surfel of theirs has a corner behind the camera
    for name in ("tilts-513-ordered", "large-in-front", "duplicates"):
        case = plain_case(name)
        good = _render(case)
        monkeypatch.setattr(view_ref, "_corner_rectangle_applies", lambda corners: True)
        same = all(np.array_equal(good[k], _render(case)[k]) for k in good)
        monkeypatch.undo()
        assert same, name


REJECTIONS = {  # change -> (scene, attribute, value, seen)
    "sqrt2 dropped from x1": ("tilts-513-ordered", "SQRT2", np.float32(1.0), True),
    "pixel centres without + 0.5": ("tilts-513-ordered", "PIXEL_CENTRE", np.float32(0.0), True),
    # dot(diff, diff) == rad^2 exactly lies inside the margin of the disc test: F calls such a fragment open, and says so
    "> turned into >= in the disc test": ("tilts-5003-shuffled", "_discarded", lambda dd, r2: dd >= r2, False),
    "dot(l, n) with the unnormalised ray": ("tilts-513-ordered", "_rays_of_the_dot", lambda normalised, unnormalised: unnormalised, True),
}


@pytest.mark.parametrize("change", sorted(REJECTIONS))
def test_one_changed_line_of_view_ref(monkeypatch, change):
    name, attr, value, seen = REJECTIONS[change]
    case = plain_case(name)
    assert _rejected(case) is None
    monkeypatch.setattr(view_ref, attr, value)
    why = _rejected(case)
    print("%s on %s: %s" % (change, name, why))
    assert (why is not None) == seen
    if not seen:  # not even on the large and the duplicated discs
        assert _rejected(plain_case("duplicates")) is None and _rejected(plain_case("large-behind")) is None


def test_a_tie_that_goes_to_the_higher_index_is_rejected(monkeypatch):
    case = plain_case("duplicates")
    top = np.uint64(0xFFFFFFFF)
    monkeypatch.setattr(view_ref, "_key", lambda depth, s: (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (top - np.uint64(s)))
    monkeypatch.setattr(view_ref, "_index_of", lambda keys: top - (keys & top))
    why = _rejected(case)
    assert why is not None and "lower-indexed copy" in why


# ------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ------------------------------------------------------------------------------------------------------------------------------
def small_solver(api, rows, cols):
    p = driver_params(api)
    p.ctf_levels = 2
    return make_solver(api, rows, cols, p)


@pytest.fixture(scope="module")
def box(hip_auto):
    s = small_solver(hip_auto, 60, 80)
    yield s
    s.close()


def _check_hip_views(box, case, min_large=None):
    from staticfusion_amd import SurfelMap

    ref = view_reference(case)
    v = view_of(case)
    loose = sfview.render_surfels(box, case.surfels, v, tick=case.tick)
    stats = S.check_drawing(ref, loose["index"], loose["depth"])
    check_caps(case, ref, stats, "hip")
    check_floors(case, ref, loose["index"])
    m = SurfelMap(box, max(case.surfels.shape[0], box.rows * box.cols))
    m.upload(case.surfels, np.eye(4, dtype=np.float32), case.tick)
    mapped = sfview.render([m], [v])[0]
    large = sfview.last_large_sprites(box, 1)[0]
    m.close()
    S.check_drawing(ref, mapped["index"], mapped["depth"])
    assert np.array_equal(mapped["index"], loose["index"])
    return loose, large


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PLAIN))
def test_hip_views_meet_the_exact_drawing(box, name):
    case = plain_case(name)
    got, large = _check_hip_views(box, case)
    if case.kind == "crossing" or case.name.startswith("large"):
        # both kernels' paths won pixels: the crossing discs of the 80 x 60 scene and the large sprite go to the large-sprite
        # kernel, the 500 small ones do not; in the 32 x 32 image a whole-image sprite is still the small-sprite kernel's
        assert large == (0 if case.name == "crossing-32x32" else len(case.big))
    elif case.kind == "grazing":
        assert large == 0


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,which", FRAME_IDS)
def test_hip_frame_models_meet_the_exact_drawing(hip_auto, ora, box, rows, cols, which):
    case = get_frame_case(ora, rows, cols, which)
    got, _ = _check_hip_views(box, case)
    assert (got["index"] >= 0).mean() > 0.5
    s = small_solver(hip_auto, rows, cols)
    vc.prime_pure_render(s, rows, cols)
    _check_prediction(s, case, "hip")
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", HANDLE_SIZED)
def test_hip_prediction_meets_the_exact_drawing(hip_auto, name):
    case = plain_case(name)
    s = small_solver(hip_auto, case.rows, case.cols)
    vc.prime_pure_render(s, case.rows, case.cols)
    _check_prediction(s, case, "hip")
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,on_samples,zero_channel,expect_dense", COMPOSITIONS)
def test_hip_composition_is_exact(hip_auto, rows, cols, on_samples, zero_channel, expect_dense):
    s = small_solver(hip_auto, rows, cols)
    prime_composition(s, rows, cols)
    mp, surf = composition_case(s, rows, cols, on_samples, zero_channel)
    views = composition_views(mp, surf, rows, cols, "%dx%d-%d%s" % (cols, rows, on_samples, "z" if zero_channel else ""))
    targets = composition_targets(views, lambda c: sfview.render_surfels(s, c.surfels, view_of(c), tick=c.tick))
    check_composition(s, mp, surf, targets, expect_dense)
    s.close()
