"""The NumPy statement of include/sf_regions.h (tests/region_ref.py) held to hand cases, so that the yardstick of the GPU
tests is itself checked: the 4 x 5 frame whose numbers were worked out by hand, a link exactly at its threshold and one ulp
beyond it, a checkerboard, an anti-diagonal pair, a U and a spiral, max_regions below R, use_b = 0 with a NaN b image, and
the component counts of the random frame the GPU tests use."""
import numpy as np
import pytest

import region_cases as rc
import region_ref as rr

F = np.float32


def fields(rec, names):
    return tuple(int(rec[k]) for k in names)


@pytest.mark.parametrize("conn", [4, 8])
def test_the_hand_frame(conn):
    z, b = rc.hand_frame()
    summ, rec, lab = rr.label(z, b, rr.params(min_pixels=1, connectivity=conn), 6)
    assert fields(summ, rr.SUMMARY_FIELDS) == (9, 4, 4, 4)
    assert lab.tolist() == [[1, 1, 1, 0, 0], [1, 0, 1, 0, 3], [0, 0, 1, 0, 4], [2, 0, 0, 0, 0]] and lab.dtype == np.int32
    assert fields(rec[0], rr.REGION_FIELDS) == (6, 0, 0, 2, 0, 2, 1024, 1188, 4, 7, 6554, 0)  # the ramp chains
    assert fields(rec[1], ("n", "first", "z_min", "z_max")) == (1, 3, 3072, 3072)  # (3, 1) has a NaN b
    assert fields(rec[2], ("n", "first", "z_min", "z_max")) == (1, 17, 2048, 2048)  # (0, 4) has b == b_max
    assert fields(rec[3], ("n", "first", "z_min", "z_max")) == (1, 18, 2253, 2253)  # 0.2 > 0.05 + 0.04: the step splits
    assert rec[4:].tobytes() == bytes(2 * 64)
    # min_pixels = 2: one region, the three single pixels are labelled -1
    summ, rec, lab = rr.label(z, b, rr.params(min_pixels=2, connectivity=conn), 6)
    assert fields(summ, rr.SUMMARY_FIELDS) == (9, 4, 1, 1)
    assert lab.tolist() == [[1, 1, 1, 0, 0], [1, 0, 1, 0, -1], [0, 0, 1, 0, -1], [-1, 0, 0, 0, 0]]
    assert fields(rec[0], rr.REGION_FIELDS) == (6, 0, 0, 2, 0, 2, 1024, 1188, 4, 7, 6554, 0) and rec[1:].tobytes() == bytes(5 * 64)


def test_a_link_at_its_threshold_and_one_ulp_beyond():
    p = rr.params(min_pixels=1, dz_abs=0.25, dz_rel=0.5, use_b=0)
    # zp = 2: the threshold is 0.25 + 0.5 * 2 = 1.25 exactly in fp32, and 3.25 - 2 = 1.25 exactly
    at = np.array([[2.0, 3.25]], F)
    beyond = np.array([[2.0, np.nextafter(F(3.25), F(4))]], F)
    assert bool(rr.linked(at[0, 0], at[0, 1], p)) and bool(rr.linked(at[0, 1], at[0, 0], p))
    assert not bool(rr.linked(beyond[0, 0], beyond[0, 1], p)) and not bool(rr.linked(beyond[0, 1], beyond[0, 0], p))
    assert fields(rr.label(at, None, p, 2)[0], rr.SUMMARY_FIELDS) == (2, 1, 1, 1)
    assert fields(rr.label(beyond, None, p, 2)[0], rr.SUMMARY_FIELDS) == (2, 2, 2, 2)
    assert fields(rr.label(at.T, None, p, 2)[0], rr.SUMMARY_FIELDS) == (2, 1, 1, 1)  # and down a column
    assert fields(rr.label(beyond.T, None, p, 2)[0], rr.SUMMARY_FIELDS) == (2, 2, 2, 2)


@pytest.mark.parametrize("rows,cols", [(6, 8), (5, 7), (37, 53)])
def test_a_checkerboard(rows, cols):
    z, b = rc.checkerboard(rows, cols)
    n = (rows * cols + 1) // 2
    s4, r4, l4 = rr.label(z, b, rr.params(min_pixels=1, connectivity=4), 3)
    s8, r8, l8 = rr.label(z, b, rr.params(min_pixels=1, connectivity=8), 3)
    assert fields(s4, rr.SUMMARY_FIELDS) == (n, n, n, 3) and fields(s8, rr.SUMMARY_FIELDS) == (n, 1, 1, 1)
    assert l4.max() == n and sorted(l4[l4 > 0].tolist()) == list(range(1, n + 1))
    assert l4[0, 0] == 1 and l4[2, 0] == 2 and l4[1, 1] == (rows + 1) // 2 + 1  # numbered down the columns
    assert set(l8.ravel().tolist()) == {0, 1} and fields(r8[0], ("n", "first", "v_max", "u_max")) == (n, 0, rows - 1, cols - 1)


def test_an_anti_diagonal_pair_is_joined_by_connectivity_8_only():
    z = np.array([[0, 1.0], [1.0, 0]], F)  # (1, 0) and (0, 1)
    b = np.zeros((2, 2), F)
    s4, _, l4 = rr.label(z, b, rr.params(min_pixels=1, connectivity=4), 2)
    s8, r8, l8 = rr.label(z, b, rr.params(min_pixels=1, connectivity=8), 2)
    assert fields(s4, rr.SUMMARY_FIELDS) == (2, 2, 2, 2) and l4.tolist() == [[0, 2], [1, 0]]
    assert fields(s8, rr.SUMMARY_FIELDS) == (2, 1, 1, 1) and l8.tolist() == [[0, 1], [1, 0]]
    assert fields(r8[0], rr.REGION_FIELDS) == (2, 1, 0, 1, 0, 1, 1024, 1024, 1, 1, 2048, 0)
    z = np.array([[1.0, 0], [0, 1.0]], F)  # the main diagonal too
    assert fields(rr.label(z, b, rr.params(min_pixels=1, connectivity=4), 2)[0], rr.SUMMARY_FIELDS) == (2, 2, 2, 2)
    assert fields(rr.label(z, b, rr.params(min_pixels=1, connectivity=8), 2)[0], rr.SUMMARY_FIELDS) == (2, 1, 1, 1)


@pytest.mark.parametrize("conn", [4, 8])
def test_a_u_and_a_spiral(conn):
    rows, cols = 9, 11
    z, b = rc.u_shape(rows, cols)
    summ, rec, lab = rr.label(z, b, rr.params(min_pixels=1, connectivity=conn), 2)
    n = 2 * rows + cols - 2
    assert fields(summ, rr.SUMMARY_FIELDS) == (n, 1, 1, 1)
    assert fields(rec[0], ("n", "first", "v_min", "v_max", "u_min", "u_max")) == (n, 0, 0, rows - 1, 0, cols - 1)
    assert lab[0, cols - 1] == 1 and lab[0, 1] == 0  # the far bar hangs on pixel 0 through the bottom row
    assert int(rec[0]["sum_u"]) == (cols - 1) * rows + sum(range(1, cols - 1))
    z, b = rc.spiral(rows, cols)
    summ, rec, lab = rr.label(z, b, rr.params(min_pixels=1, connectivity=conn), 2)
    n = int((z > 0).sum())
    assert n == 59 and fields(summ, rr.SUMMARY_FIELDS) == (n, 1, 1, 1) and fields(rec[0], ("n", "first")) == (n, 0)
    assert z[0, 0] == z.max() and lab[4, 2] == 1 and z[4, 6] == 1.0  # the path starts in the middle; pixel 0 is its far end
    # cut the spiral: two components, the outer one keeps pixel 0
    z[2, 4] = 0
    summ, rec, lab = rr.label(z, b, rr.params(min_pixels=1, connectivity=conn), 2)
    assert fields(summ, rr.SUMMARY_FIELDS) == (n - 1, 2, 2, 2) and lab[0, 0] == 1 and lab[2, 3] == 1 and lab[2, 5] == 2 and lab[4, 6] == 2
    assert int(rec[0]["n"]) + int(rec[1]["n"]) == n - 1 and int(rec[1]["first"]) == 4 + 2 * rows  # (4, 2), far from (4, 6)


def test_max_regions_below_r():
    z, b = rc.hand_frame()
    p = rr.params(min_pixels=1)
    full = rr.label(z, b, p, 6)
    for m in (0, 1, 3, 4, 7):
        summ, rec, lab = rr.label(z, b, p, m)
        assert fields(summ, rr.SUMMARY_FIELDS) == (9, 4, 4, min(4, m)) and rec.shape == (m,)
        assert rec[:min(4, m)].tobytes() == full[1][:min(4, m)].tobytes() and rec[min(4, m):].tobytes() == bytes(64 * max(m - 4, 0))
        assert np.array_equal(lab, full[2]) and lab.max() == 4  # the label image carries all R numbers


def test_use_b_0_does_not_read_b():
    z, _ = rc.hand_frame()
    nan_b = np.full(z.shape, np.nan, F)
    p = rr.params(min_pixels=1, use_b=0)
    a, b_ = rr.label(z, nan_b, p, 6), rr.label(z, None, p, 6)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b_))
    # every finite positive depth is in: (3, 0) and (3, 1) are one region, (0, 4) and (1, 4) another
    assert fields(a[0], rr.SUMMARY_FIELDS) == (11, 4, 4, 4) and a[2].tolist() == [[1, 1, 1, 0, 3], [1, 0, 1, 0, 3], [0, 0, 1, 0, 4], [2, 2, 0, 0, 0]]
    assert all(int(r["sum_b"]) == 0 for r in a[1])
    assert fields(rr.label(z, nan_b, rr.params(min_pixels=1), 6)[0], rr.SUMMARY_FIELDS) == (0, 0, 0, 0)  # with use_b a NaN b is outside


def test_sum_b_clips_and_quantises():
    z = np.full((1, 4), 1.0, F)
    b = np.array([[-2.0, 0.25, 0.3, -0.0]], F)
    rec = rr.label(z, b, rr.params(min_pixels=1), 1)[1][0]
    assert int(rec["sum_b"]) == 0 + 1024 + int(np.rint(F(0.3) * F(4096))) and int(rec["n"]) == 4


def test_the_random_frame_of_the_gpu_tests():
    z, b = rc.random_levels(37, 53)
    s4 = rr.label(z, b, rr.params(b_max=rc.RANDOM_B_MAX, connectivity=4, min_pixels=1), 0)[0]
    s8 = rr.label(z, b, rr.params(b_max=rc.RANDOM_B_MAX, connectivity=8, min_pixels=1), 0)[0]
    assert int(s4["n_components"]) == 454 and int(s8["n_components"]) == 268 and int(s4["n_mask"]) == int(s8["n_mask"])
    s5 = rr.label(z, b, rr.params(b_max=rc.RANDOM_B_MAX, connectivity=8, min_pixels=5), 0)[0]
    assert 0 < int(s5["n_regions"]) < 268 and int(s5["n_components"]) == 268
