"""Properties of tests/score_ref.py, the NumPy statement of include/sf_score.h that the GPU tests compare with (no GPU here):
the seven class codes partition the pixels and reproduce the counts, hand cases at and one ulp beyond the tolerance and with
NaN / inf / 0 / negative inputs, and the premise of the GPU ranking test -- the true pose strictly has the most inliers among
thirteen poses -- from the reference alone."""
import numpy as np

import score_cases as sc
import score_ref
from staticfusion_amd import score, view

F = np.float32


def one_surfel_view():
    """a 5 x 5 view at identity whose centre pixel looks along the optical axis, and one surfel at 2 m that covers it all"""
    s = np.zeros((1, 12), np.float32)
    s[0, :4] = (0.0, 0.0, 2.0, 0.5)
    s[0, 4] = (200 << 16) + (100 << 8) + 50
    s[0, 8:11] = (0, 0, -1)
    s[0, 11] = 1.0
    v = view.View(np.eye(4), 2.5, 2.5, 10.0, 10.0, 5, 5, min_confidence=0.0)
    return s, v


def test_class_codes_partition_the_pixels_and_reproduce_the_counts():
    rng = np.random.default_rng(12)
    rows, cols = 37, 53
    v = view.View(np.eye(4), 25.25, 19.5, 47.0, -44.0, rows, cols, min_confidence=0.0)
    n = 400
    z = rng.uniform(0.8, 3.0, n)
    s = np.zeros((n, 12), np.float32)
    s[:, 0], s[:, 1], s[:, 2] = (rng.uniform(0, cols, n) - v.cx) * z / v.fx, (rng.uniform(0, rows, n) - v.cy) * z / v.fy, z
    s[:, 3] = 0.5
    s[:, 4] = (rng.integers(1, 256, n) << 16) + (rng.integers(1, 256, n) << 8) + rng.integers(1, 256, n)
    s[:, 8:11] = (0, 0, -1)
    s[:, 11] = z / 47.0 * rng.uniform(1.0, 3.0, n)
    depth = rng.uniform(0.7, 3.1, (rows, cols)).astype(np.float32)
    depth[rng.random((rows, cols)) < 0.15] = 0
    depth[3, 4], depth[5, 6], depth[7, 8] = np.nan, np.inf, -1.0
    grey = rng.random((rows, cols)).astype(np.float32)
    b = rng.random((rows, cols)).astype(np.float32)
    b[9, 10] = np.nan
    for p in (score.Params(tol_abs=0.3, tol_rel=0.05), score.Params(tol_abs=0.3, use_b=False, use_grey=False), score.Params(tol_abs=0.0, tol_rel=0.0)):
        got, cls = score_ref.score(s, v, depth, grey, b, p, tick=1)
        hist = np.bincount(cls.ravel(), minlength=7)
        assert hist.sum() == rows * cols and len(hist) == 7
        assert hist[3] == got["n_inlier"] and hist[4] == got["n_front"] and hist[5] == got["n_behind"] and hist[6] == got["n_masked"]
        assert hist[3] + hist[4] + hist[5] == got["n_both"] and hist[1] + got["n_both"] == got["n_frame"]
        assert hist[2] + got["n_both"] <= got["n_map"] <= hist[2] + got["n_both"] + hist[6]  # a masked pixel may be drawn or not
        assert got["n_map"] > 200 and got["n_front"] > 0 and got["n_behind"] > 0
        assert (got["n_masked"] > 0) == bool(p.use_b) and (got["sum_grey"] > 0) == bool(p.use_grey and p.tol_abs > 0)
        assert (got["n_inlier"] > 0) == (p.tol_abs > 0)
        assert got["sum_abs"] <= got["n_both"] * 8 * 16384 and got["sum_sq"] >= got["sum_abs"] ** 2 // max(got["n_both"], 1)


def test_one_surfel_at_two_metres_at_and_one_ulp_beyond_the_tolerance():
    s, v = one_surfel_view()
    import view_ref

    zm = view_ref.render(s, v, tick=1)["depth"]
    assert (zm > 0).all() and zm[2, 2] == F(2.0)  # the surfel covers the view; on the axis the depth is exact
    tol = F(2.0 ** -6)
    p = score.Params(tol_abs=float(tol), tol_rel=0.0, use_b=False, use_grey=False)
    at_far, at_near = zm + tol, zm - tol
    assert np.all(at_far - zm == tol) and np.all(at_near - zm == -tol)  # the residual is exactly the tolerance
    cases = [(at_far, 3, "n_inlier"), (np.nextafter(at_far, F(np.inf)), 5, "n_behind"), (at_near, 3, "n_inlier"), (np.nextafter(at_near, F(-np.inf)), 4, "n_front")]
    for depth, code, field in cases:
        got, cls = score_ref.score(s, v, depth, None, None, p, tick=1)
        assert (cls == code).all() and got[field] == 25 == got["n_both"] == got["n_frame"] == got["n_map"], field
        assert got["sum_abs"] >= 25 * 256 and got["n_masked"] == 0 and got["sum_grey"] == 0
    # tol_rel counts per metre of MAP depth: 2^-7 per metre at 2 m is the same bound on the axis
    got, cls = score_ref.score(s, v, at_far, None, None, score.Params(tol_abs=0.0, tol_rel=2.0 ** -7, use_b=False, use_grey=False), tick=1)
    assert cls[2, 2] == 3
    got, cls = score_ref.score(s, v, np.nextafter(at_far, F(np.inf)), None, None, score.Params(tol_abs=0.0, tol_rel=2.0 ** -7, use_b=False, use_grey=False), tick=1)
    assert cls[2, 2] == 5


def test_nan_inf_zero_and_negative_inputs():
    s, v = one_surfel_view()
    depth = np.full((5, 5), 2.0, np.float32)
    depth[0, 0], depth[0, 1], depth[0, 2], depth[0, 3] = np.nan, np.inf, 0.0, -2.0
    grey = np.full((5, 5), 0.5, np.float32)
    grey[4, 4] = np.nan
    b = np.ones((5, 5), np.float32)
    b[3, 3] = np.nan
    b[3, 2] = 0.5  # not above b_min
    p = score.Params(tol_abs=0.05, tol_rel=0.0, max_residual=8.0)
    got, cls = score_ref.score(s, v, depth, grey, b, p, tick=1)
    assert cls[0, 0] == 2 and cls[0, 2] == 2 and cls[0, 3] == 2  # NaN, 0 and negative depth: no frame pixel
    assert cls[0, 1] == 5  # inf: a frame pixel behind the map, clipped in the sums
    assert cls[3, 3] == 6 and cls[3, 2] == 6  # a NaN b, and b == b_min: masked
    assert got["n_frame"] == 20 and got["n_masked"] == 2 and got["n_map"] == 25 and got["n_both"] == 20 and got["n_behind"] == 1 and got["n_inlier"] == 19
    inl = cls == 3
    zm_abs = got["sum_abs"] - 8 * 16384
    assert 0 <= zm_abs <= 19 * 16 and got["sum_sq"] >= (8 * 16384) ** 2
    # the grey sum: 18 finite inliers, and the NaN grey adds exactly 65536
    gm = (F(0.299) * (F(200) * (F(1) / F(255))) + F(0.587) * (F(100) * (F(1) / F(255)))) + F(0.114) * (F(50) * (F(1) / F(255)))
    each = int(np.rint(np.abs(F(0.5) - gm) * F(65536)))
    assert inl[4, 4] and got["sum_grey"] == 18 * each + 65536
    # without the b image the two masked pixels are inliers; without grey the sum is 0
    got2, cls2 = score_ref.score(s, v, depth, None, None, score.Params(tol_abs=0.05, tol_rel=0.0, use_b=False, use_grey=False), tick=1)
    assert got2["n_masked"] == 0 and got2["n_inlier"] == 21 and got2["sum_grey"] == 0 and cls2[3, 3] == 3
    # no map at all: frame only / neither
    got3, cls3 = score_ref.score(np.zeros((0, 12), np.float32), v, depth, grey, b, p, tick=1)
    assert got3["n_map"] == 0 == got3["n_both"] and got3["n_frame"] == 20 and sorted(np.unique(cls3)) == [0, 1, 6]


def test_the_true_pose_has_strictly_the_most_inliers(ora):
    """the premise of the GPU ranking test, with the fixture's intrinsics and with a handle's own defaults for 80 x 60"""
    from conftest import driver_params, make_solver

    so = make_solver(ora, sc.RANK_ROWS, sc.RANK_COLS, driver_params(ora))
    mp = so.default_model_params()
    own = dict(cx=float(mp.cx), cy=float(mp.cy), fx=float(mp.fx), fy=float(mp.fy))
    so.close()
    for intr in (sc.RANK_INTRINSICS, own):
        ref = sc.ranking_reference(intr["cx"], intr["cy"], intr["fx"], intr["fy"])
        inl = [r["n_inlier"] for r in ref]
        print("inliers of the true pose and of the twelve displaced ones:", inl, "n_both", ref[0]["n_both"])
        assert inl[0] > max(inl[1:]) and inl[0] > 0.9 * ref[0]["n_both"]
    ref = sc.ranking_reference(*[sc.RANK_INTRINSICS[k] for k in ("cx", "cy", "fx", "fy")])  # (cached)
    assert ref[0]["n_inlier"] == 4597 and ref[0]["n_both"] == 4632 and max(r["n_inlier"] for r in ref[1:]) == 4272
