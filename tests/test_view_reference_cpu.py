"""The premise of the GPU tests of free-view rendering, checked without a GPU: the brute-force NumPy renderer of
tests/view_ref.py draws what the CPU oracle's prediction draws, bit for bit, wherever the oracle can be asked -- the handle's
own resolution, but any pose and any intrinsics, with the stream primed so that nothing is filled in."""
import numpy as np
import pytest

import view_cases as vc
import view_ref
from conftest import driver_params, make_solver
from test_model_prediction import encode_color


@pytest.fixture(scope="module", params=vc.SIZES, ids=lambda rc: "%dx%d" % (rc[1], rc[0]))
def primed(request, ora):
    rows, cols = request.param
    s = make_solver(ora, rows, cols, driver_params(ora))
    vc.prime_pure_render(s, rows, cols)
    mp0 = s.default_model_params()
    return s, rows, cols, mp0, vc.frame_surfels(rows, cols, mp0)


@pytest.mark.parametrize("default_intrinsics", [True, False])
@pytest.mark.parametrize("max_depth", [20.0, 2.25])
def test_numpy_renderer_equals_the_oracle(primed, default_intrinsics, max_depth):
    s, rows, cols, mp0, surf = primed
    assert surf.shape[0] > 0.8 * rows * cols and np.all(view_ref.decode_colour(surf[:, 4]) >= 1)
    intr = dict(cx=mp0.cx, cy=mp0.cy, fx=mp0.fx, fy=mp0.fy) if default_intrinsics else vc.other_intrinsics(mp0)
    mp = vc.pure_render_params(s, intr, 0.25, max_depth, time=3)
    for name, pose in vc.poses():
        s.predict_from_model(0, surf, pose, mp)
        d, inten = s.prediction()
        ref = view_ref.render(surf, vc.view_of(mp, pose, rows, cols))
        # a freshly primed stream fills nothing in (black frame, b = 0.1): the whole image is compared, not the drawn pixels
        assert np.array_equal(ref["depth"], d), name
        assert np.array_equal(view_ref.grey(ref["rgb"]), inten), name
        drawn = ref["depth"] > 0
        assert np.array_equal(ref["index"] >= 0, drawn)
        assert np.array_equal(ref["rgb"][drawn], view_ref.decode_colour(surf[ref["index"][drawn], 4]))
        if name == "away":
            assert not drawn.any()
        else:
            assert drawn.mean() > (0.5 if max_depth > 3 else 0.05)
            assert np.all(surf[ref["index"][drawn], 3] >= np.float32(0.25))  # only stable surfels


def hand_surfel(z, rgb=(200, 100, 50), conf=0.5, r=0.05):
    s = np.zeros((1, 12), np.float32)
    s[0, :4] = (0, 0, z, conf)
    s[0, 4] = encode_color(np.array(rgb))
    s[0, 8:11] = (0, 0, -1)
    s[0, 11] = r
    return s


def test_hand_cases(primed):
    s, rows, cols, mp0, _ = primed
    mp = vc.pure_render_params(s, dict(cx=mp0.cx, cy=mp0.cy, fx=mp0.fx, fy=mp0.fy), 0.25, 20.0, time=1)
    eye = np.eye(4, dtype=np.float32)
    # two identical surfels at different buffer positions (another colour tells them apart): the lower index wins
    two = np.concatenate([hand_surfel(1.5, (10, 20, 30)), hand_surfel(1.5, (40, 50, 60))])
    ref = view_ref.render(two, vc.view_of(mp, eye, rows, cols))
    drawn = ref["depth"] > 0
    assert drawn.sum() >= 4 and np.all(  # (a disc of 0.05 m at 1.5 m covers four pixel centres at 40 x 30)
ref["index"][drawn] == 0) and np.all(ref["rgb"][drawn] == (10, 20, 30))
    s.predict_from_model(0, two, eye, mp)
    d, inten = s.prediction()
    assert np.array_equal(ref["depth"], d) and np.array_equal(view_ref.grey(ref["rgb"]), inten)
    swapped = view_ref.render(two[::-1].copy(), vc.view_of(mp, eye, rows, cols))
    assert np.all(swapped["index"][drawn] == 0) and np.all(swapped["rgb"][drawn] == (40, 50, 60))
    # a surfel at exactly max_depth passes the cull (z > max_depth is false) and fails the depth test (depth = 1.0): not drawn
    mp.max_depth = mp.extract_max_depth = 2.0
    at = hand_surfel(2.0)
    assert not (view_ref.render(at, vc.view_of(mp, eye, rows, cols))["depth"] > 0).any()
    s.predict_from_model(0, at, eye, mp)
    assert not (s.prediction()[0] > 0).any()
    nearer = hand_surfel(np.float32(1.9999))
    ref = view_ref.render(nearer, vc.view_of(mp, eye, rows, cols))
    s.predict_from_model(0, nearer, eye, mp)
    assert (ref["depth"] > 0).any() and np.array_equal(ref["depth"], s.prediction()[0])
    # confidence below the threshold: not drawn; the age test is off at max_age < 0 and follows sfw_filter's test B otherwise
    assert not (view_ref.render(hand_surfel(1.5, conf=0.2), vc.view_of(mp, eye, rows, cols))["depth"] > 0).any()
    old = hand_surfel(1.5)
    old[0, 7] = 2.0
    assert (view_ref.render(old, vc.view_of(mp, eye, rows, cols, max_age=3), tick=5)["depth"] > 0).any()
    assert not (view_ref.render(old, vc.view_of(mp, eye, rows, cols, max_age=2), tick=5)["depth"] > 0).any()
