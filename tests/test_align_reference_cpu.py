"""The reference of the align tests (tests/align_ref.py) against hand arithmetic and against the library's pure-host step,
no GPU: one fronto-parallel disc, the gates at their ties, every special depth and b value, strides, the two stops, sfa_step
bit for bit on 100 random systems, the Cayley rotation, and the PREMISE of the GPU convergence test from the reference alone.

Measured with the stated reference (fixture score_cases.ranking_case, 60 x 80, twelve poses displaced by +-0.05 along one
twist axis, iterations 10, dist_max 0.15, stride 1, use_b 0): the worst final pose is 2.15 mm and 0.81 mrad from identity;
with step 0.15, dist_max 0.3 and 15 iterations the worst is 5.24 mm and 1.76 mrad. The bars below (0.01 and 0.03) are a fifth
of the displacement, not tuned tolerances."""
import numpy as np
import pytest

import align_cases as ac
import align_ref
import score_cases as sc
from staticfusion_amd import align
from staticfusion_amd.synth import LCG64

F = np.float32
IDENTITY = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def H_at(w, k, l):
    return w[8 + align_ref.PAIRS.index((min(k, l), max(k, l)))]


def disc_case(depth_value=2.03, rows=16, cols=16):
    v = ac.plane_view(rows, cols)
    surf = ac.flat_surfel(0.0, 0.0, 2.0, 4.0)[None]
    return v, surf, np.full((rows, cols), depth_value, np.float32), align_ref.model_image(surf, v, ac.TICK)


def test_one_disc_by_hand_and_one_damped_step():
    v, surf, depth, model = disc_case()
    assert model["drawn"].all() and np.abs(model["M"][2] - F(2)).max() <= 2.4e-7 and (model["n"][2] == F(-1)).all()
    p = ac.params(use_b=False, damping=1e-6)
    w = align_ref.linearise(model, v, depth, None, p, IDENTITY)
    n = w[0]
    # a frame pixel projects onto the border between two drawn pixels (the half pixel of the two conventions), so a pixel of
    # the first row or column may round out of the image; every other pixel pairs with the plane
    assert 15 * 15 <= n <= 256
    # n = (0, 0, -1): r = -(2.03 - 2), rho = rint(-0.03 * 65536) = -1966, a = (-Q.y, Q.x, 0, 0, 0, -1) * 4096
    assert w[1] == n * 1966 * 1966
    assert w[2 + 5] == n * 4096 * 1966 and w[2 + 2] == w[2 + 3] == w[2 + 4] == 0
    assert H_at(w, 5, 5) == n * 4096 * 4096
    for k in (2, 3, 4):
        assert all(H_at(w, k, l) == 0 for l in range(6))
    assert H_at(w, 0, 0) > 0 and H_at(w, 1, 1) > 0 and w[29:] == [0, 0, 0]
    if n == 256:  # the pixel grid is symmetric about the principal point: the first moments cancel exactly
        assert w[2] == w[3] == 0 and H_at(w, 0, 5) == H_at(w, 1, 5) == 0
    code, D = align_ref.step(w, p.damping, IDENTITY)
    assert code == align_ref.OK
    # rho is quantised to 2^-16 m (error <= 2^-17), r carries a few fp32 ulps of 2 m (<= 1e-6), the damping shrinks by 3e-8
    assert abs(D[11] + 0.03) <= 2.0 ** -16
    assert abs(D[3]) <= 2.0 ** -16 and abs(D[7]) <= 2.0 ** -16
    res, systems = align_ref.refine(surf, v, depth, None, ac.params(use_b=False, damping=1e-6, iterations=2), tick=ac.TICK)
    assert res["status"] == align_ref.OK and res["ss_last"] < res["ss_first"] and abs(float(res["pose"][14]) + 0.03) <= 2.0 ** -15


def test_a_pair_at_exactly_dist_max_and_one_ulp_beyond():
    # a 1 x 1 view whose principal point is the frame's pixel centre and whose focal length is so long that the half pixel
    # between the two conventions vanishes below an ulp: M = (1e-6, 1e-6, 2) with M.z exact, d = (., ., zf - 2)
    v = ac.view.View(np.eye(4), 0.0, 0.0, 1e6, 1e6, 1, 1, min_confidence=0.0)
    surf = ac.flat_surfel(0.0, 0.0, 2.0, 1.0)[None]
    model = align_ref.model_image(surf, v, ac.TICK)
    assert model["drawn"].all() and model["M"][2][0, 0] == F(2)
    p = ac.params(dist_max=0.125, use_b=False)
    at = np.full((1, 1), 2.125, np.float32)
    w = align_ref.linearise(model, v, at, None, p, IDENTITY)
    assert w[0] == 1 and w[1] == (2 ** 13) ** 2 and w[2 + 5] == 4096 * 2 ** 13  # |r| == dist_max pairs; rho = -0.125 * 65536
    beyond = np.nextafter(at, F(3))
    assert align_ref.linearise(model, v, beyond, None, p, IDENTITY)[0] == 0
    below = np.full((1, 1), 1.875, np.float32)
    assert align_ref.linearise(model, v, below, None, p, IDENTITY)[0] == 1
    assert align_ref.linearise(model, v, np.nextafter(below, F(0)), None, p, IDENTITY)[0] == 0


def test_special_depth_b_and_normal_values():
    v, surf, depth, model = disc_case(2.0, 15, 17)
    p = ac.params(use_b=True, z_max=2.5)
    b = np.ones((15, 17), np.float32)
    full = align_ref.linearise(model, v, depth, b, p, IDENTITY)[0]
    assert full >= 14 * 16
    inner = [(3, 4), (4, 9), (5, 5), (6, 11), (7, 2), (8, 8), (9, 13), (10, 6)]  # rows and columns away from the border: pairs for certain
    for (y, x), bad in zip(inner, (0.0, -1.5, np.nan, np.inf, 2.6, -np.inf, -0.0, np.nextafter(F(2.5), F(3)))):
        d = depth.copy()
        d[y, x] = bad
        assert align_ref.linearise(model, v, d, b, p, IDENTITY)[0] == full - 1, bad
    d = depth.copy()
    d[3, 4] = 2.5  # zf == z_max is used, but lies 0.5 m behind the plane: the distance gate drops it
    assert align_ref.linearise(model, v, d, b, ac.params(z_max=2.5, dist_max=1.0), IDENTITY)[0] == full
    assert align_ref.linearise(model, v, d, b, p, IDENTITY)[0] == full - 1
    for bad in (np.nan, 0.5, 0.25, -np.inf):  # b == b_min does not count
        bb = b.copy()
        bb[5, 5] = bad
        assert align_ref.linearise(model, v, depth, bb, p, IDENTITY)[0] == full - 1, bad
        assert align_ref.linearise(model, v, depth, bb, ac.params(use_b=False), IDENTITY)[0] == full
    bb = b.copy()
    bb[5, 5] = np.nextafter(F(0.5), F(1))
    assert align_ref.linearise(model, v, depth, bb, p, IDENTITY)[0] == full
    # a NaN normal, and one shorter than sqrt(0.5), in the model image: never a pair
    for bad in (np.nan, 0.7):
        m2 = dict(drawn=model["drawn"], M=model["M"], n=tuple(x.copy() for x in model["n"]))
        m2["n"][2][:] = F(-bad)
        assert align_ref.linearise(m2, v, depth, b, p, IDENTITY)[0] == 0
    m2["n"][2][:] = F(-0.75)  # 0.5625 > 0.5
    assert align_ref.linearise(m2, v, depth, b, p, IDENTITY)[0] == full


@pytest.mark.parametrize("stride", [1, 2, 3])
def test_strides_on_odd_sizes(stride):
    v, surf, depth, model = disc_case(2.01, 15, 17)
    rng = np.random.default_rng(stride)
    depth = (depth + rng.normal(0, 0.01, depth.shape)).astype(np.float32)
    w = align_ref.linearise(model, v, depth, None, ac.params(use_b=False, stride=stride), IDENTITY)
    keep = np.zeros(depth.shape, bool)
    keep[::stride, ::stride] = True
    assert keep.sum() == -(-15 // stride) * -(-17 // stride)
    masked = np.where(keep, depth, F(0))
    assert w == align_ref.linearise(model, v, masked, None, ac.params(use_b=False, stride=1), IDENTITY)
    assert (-(-15 // stride) - 1) * (-(-17 // stride) - 1) <= w[0] <= keep.sum()


def test_few_pairs_and_the_degenerate_plane():
    v, surf, depth, model = disc_case()
    few, systems = align_ref.refine(surf, v, depth, None, ac.params(use_b=False, min_pairs=257, damping=1e-3, iterations=3), tick=ac.TICK)
    assert few["status"] == align_ref.FEW_PAIRS and few["iterations_done"] == 0 and few["n_last"] == few["n_first"] > 200
    assert systems.shape == (4, 32) and not systems[1:].any() and np.array_equal(few["pose"], np.eye(4, dtype=np.float32).ravel())
    deg, systems = align_ref.refine(surf, v, depth, None, ac.params(use_b=False, min_pairs=6, damping=0.0, iterations=3), tick=ac.TICK)
    assert deg["status"] == align_ref.DEGENERATE and deg["iterations_done"] == 0 and not systems[1:].any()
    assert deg["ss_last"] == deg["ss_first"] and np.array_equal(deg["pose"], np.eye(4, dtype=np.float32).ravel())
    ok, systems = align_ref.refine(surf, v, depth, None, ac.params(use_b=False, min_pairs=6, damping=1e-3, iterations=3), tick=ac.TICK)
    assert ok["status"] == align_ref.OK and ok["iterations_done"] == 3 and systems[3, 0] > 200 and ok["ss_last"] < ok["ss_first"]


def random_system(g):
    """a well-posed system: sums of n random rows with |a| <= 2^18 and |rho| <= 2^16"""
    n = 6 + int(g.uniform(0, 200))
    a = np.array([[int(g.uniform(-2 ** 18, 2 ** 18)) for _ in range(6)] for _ in range(n)], np.int64)
    rho = np.array([int(g.uniform(-2 ** 16, 2 ** 16)) for _ in range(n)], np.int64)
    return [n, int((rho * rho).sum())] + [int((a[:, k] * rho).sum()) for k in range(6)] + [int((a[:, k] * a[:, l]).sum()) for k, l in align_ref.PAIRS] + [0, 0, 0]


def test_the_librarys_step_equals_the_numpy_step_bit_for_bit():
    g = LCG64(17)
    seen = set()
    for q in range(100):
        w = random_system(g)
        if q % 10 == 9:  # a rank-deficient one: the fourth column is zero
            for k in range(6):
                w[8 + align_ref.PAIRS.index((min(k, 3), max(k, 3)))] = 0
            w[2 + 3] = 0
        damping = [0.0, 1e-3, 0.5][q % 3] if q % 10 != 9 else 0.0
        D = [g.uniform(-1, 1) for _ in range(12)]
        rec = np.array(w, np.int64).view(align.SYSTEM_DTYPE)[0]
        code, got = align.step(rec, damping, D)
        want_code, want = align_ref.step(w, damping, D)
        seen.add(code)
        assert code == want_code, q
        if code == align.OK:
            assert np.array(want, np.float64).tobytes() == got.tobytes(), q
        else:
            assert got is None
    assert seen == {align.OK, align.DEGENERATE}


def test_the_cayley_rotation_is_a_rotation():
    g = LCG64(5)
    for q in range(200):
        scale = [1e-3, 0.1, 1.0, 10.0][q % 4]
        R = np.array(align_ref.cayley(*[g.uniform(-scale, scale) for _ in range(3)]))
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1.0) < 1e-14
    assert align_ref.cayley(0.0, 0.0, 0.0) == [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    R = np.array(align_ref.cayley(0.0, 0.0, 0.02))  # about z by 2 * atan(0.01)
    assert abs(np.arctan2(R[1, 0], R[0, 0]) - 2.0 * np.arctan(0.01)) < 1e-15


@pytest.mark.parametrize("step,dist_max,iterations,bar", [(sc.RANK_STEP, 0.15, 10, 0.01), (0.15, 0.3, 15, 0.03)])
def test_premise_of_the_convergence_test(step, dist_max, iterations, bar):
    ref = ac.convergence_reference(step, dist_max, iterations)
    worst = [0.0, 0.0]
    for q, (res, systems) in enumerate(ref):
        trans, rot = ac.pose_error(res["pose"])
        worst = [max(worst[0], trans), max(worst[1], rot)]
        assert res["status"] == align_ref.OK and res["iterations_done"] == iterations, q
        assert trans < bar and rot < bar, (q, trans, rot)
        assert res["ss_last"] < res["ss_first"], q
        assert res["n_first"] == systems[0, 0] and res["n_last"] == systems[iterations, 0] > 1000
    print("worst final pose: %.2f mm, %.2f mrad" % (1e3 * worst[0], 1e3 * worst[1]))
