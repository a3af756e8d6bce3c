"""Properties of tests/keyframe_ref.py, the NumPy statement of include/sf_keyframes.h that the GPU tests compare with (no GPU
here): hand cases at and one quantum beyond every threshold and with NaN / inf / 0 / negative inputs, the remainder of an
image that is no multiple of the cell, packing and distance, the (distance, slot) order, and the premise of the GPU
retrieval test -- every query's nearest keyframe is its own, by a wide margin -- from the reference alone."""
import numpy as np

import keyframe_cases as kc
import keyframe_ref as kr

F = np.float32


def one_cell(depth_values, grey_values, cell=2):
    d = np.array(depth_values, F).reshape(cell, cell)
    g = np.array(grey_values, F).reshape(cell, cell)
    return kr.thumbnail(d, g, cell)


def fern(cell=0, t_grey=0, t_depth=0):
    f = np.zeros(1, kr.FERN_DTYPE)
    f[0] = (cell, t_grey, t_depth, 0)
    return f


def test_thresholds_at_and_one_quantum_beyond():
    # grey: four pixels of 0.5 give G = 4 * 2048 = t_grey * a exactly -> bit 0 clear; one quantum (1 / 4096) more -> set
    th = one_cell([1, 1, 1, 1], [0.5, 0.5, 0.5, 0.5])
    assert [int(x[0]) for x in th] == [4, 4 * 1024, 4 * 2048]
    assert kr.nibbles(th, fern(t_grey=2048, t_depth=32768), 2)[0] == 4 and kr.nibbles(th, fern(t_grey=2047, t_depth=32768), 2)[0] == 5
    th = one_cell([1, 1, 1, 1], [0.5, 0.5, 0.5, 0.5 + 1.0 / 4096])
    assert int(th[2][0]) == 4 * 2048 + 1 and kr.nibbles(th, fern(t_grey=2048, t_depth=32768), 2)[0] == 5
    # depth: Z = t_depth * n exactly -> bit 1 clear; one quantum (1 / 1024 m) more -> set; n counts the valid pixels only
    th = one_cell([2, 2, 2, 0], [0, 0, 0, 0])
    assert [int(x[0]) for x in th] == [3, 3 * 2048, 0]
    assert kr.nibbles(th, fern(t_depth=2048), 2)[0] == 4 and kr.nibbles(th, fern(t_depth=2047), 2)[0] == 6
    th = one_cell([2, 2, 2 + 1.0 / 1024, 0], [0, 0, 0, 0])
    assert int(th[1][0]) == 3 * 2048 + 1 and kr.nibbles(th, fern(t_depth=2048), 2)[0] == 6
    # 2 n == a sets bit 2, one valid pixel fewer clears it
    assert kr.nibbles(one_cell([1, 1, 0, 0], [0] * 4), fern(t_depth=32768), 2)[0] == 4
    assert kr.nibbles(one_cell([1, 0, 0, 0], [0] * 4), fern(t_depth=32768), 2)[0] == 0
    # a cell without a valid pixel: bit 1 is clear whatever the threshold, t_depth = 0 included
    th = one_cell([0, 0, 0, 0], [1, 1, 1, 1])
    assert [int(x[0]) for x in th] == [0, 0, 4 * 4096]
    assert kr.nibbles(th, fern(t_grey=0, t_depth=0), 2)[0] == 1 and kr.nibbles(th, fern(t_grey=4096, t_depth=0), 2)[0] == 0


def test_nan_inf_zero_and_negative_inputs():
    nan, inf = np.nan, np.inf
    n, Z, G = one_cell([nan, inf, 0.0, -2.0], [0.5] * 4)
    assert (int(n[0]), int(Z[0])) == (1, 32768)  # only +inf is valid, and it is clipped to 32 m
    n, Z, G = one_cell([-inf, 40.0, 1e-30, 0.25], [0.5] * 4)
    assert (int(n[0]), int(Z[0])) == (3, 32768 + 0 + 256)  # -inf is not valid; a tiny positive depth is, and adds 0
    n, Z, G = one_cell([1] * 4, [nan, -0.5, 1.5, inf])
    assert int(G[0]) == 0 + 0 + 4096 + 4096  # a NaN grey adds 0, +inf adds 4096
    n, Z, G = one_cell([1] * 4, [-inf, 0.0, 1.0, 0.25])
    assert int(G[0]) == 0 + 0 + 4096 + 1024
    # ties of rintf go to even: 0.5 / 4096 * 4096 = 0.5 -> 0, 1.5 -> 2
    n, Z, G = one_cell([1] * 4, [0.5 / 4096, 1.5 / 4096, 2.5 / 4096, 0])
    assert int(G[0]) == 0 + 2 + 2


def test_the_remainder_of_an_image_changes_nothing():
    rng = np.random.default_rng(3)
    for rows, cols, cell in ((5, 7, 3), (53, 37, 8), (130, 66, 64)):
        depth, grey = kc.special_frame(rows, cols, seed=rows)
        gr, gc = kr.grid(rows, cols, cell)
        ferns = kc.spread_ferns(65, gr * gc, seed=1)
        a = kr.encode(depth, grey, ferns, cell)
        d2, g2 = depth.copy(), grey.copy()
        d2[gr * cell:, :] = rng.uniform(0, 5, d2[gr * cell:, :].shape)
        d2[:, gc * cell:] = np.nan
        g2[gr * cell:, :] = 7.0
        g2[:, gc * cell:] = rng.random(g2[:, gc * cell:].shape)
        assert np.array_equal(a, kr.encode(d2, g2, ferns, cell))
        assert np.array_equal(a, kr.encode(depth[:gr * cell, :gc * cell], grey[:gr * cell, :gc * cell], ferns, cell))
        # the cell order: c = cv + cu * gr
        n, Z, G = kr.thumbnail(depth, grey, cell)
        cv, cu = gr - 1, gc - 1
        block = depth[cv * cell:(cv + 1) * cell, cu * cell:(cu + 1) * cell]
        with np.errstate(invalid="ignore"):
            assert int(n[cv + cu * gr]) == int((block > 0).sum())


def test_packing_distance_and_order():
    nib = np.array([1, 7, 0, 4, 5, 2, 6, 3, 7], np.uint32)
    code = kr.pack(nib)
    assert code.tolist() == [0x36254071, 0x7] and kr.unpack(code, 9).tolist() == nib.tolist()
    other = kr.pack(np.array([1, 6, 0, 4, 4, 2, 6, 3, 0], np.uint32))
    assert kr.distance(code, other, 9) == 3 and kr.distance(code, code, 9) == 0
    # the device's expression for eight ferns: x = a ^ b; x |= x >> 1; x |= x >> 2; popcount(x & 0x11111111)
    x = int(code[0]) ^ int(other[0])
    x |= x >> 1
    x |= x >> 2
    assert bin(x & 0x11111111).count("1") == 2
    db = [code, other, code, other, code]
    tags = [0, 0, 1, 1, 0]
    assert kr.query(db, tags, code, -1, 3, 9) == [(0, 0), (2, 0), (4, 0)]  # an equal distance goes to the lower slot
    assert kr.query(db, tags, code, 0, 4, 9) == [(0, 0), (4, 0), (1, 3), (-1, -1)]
    assert kr.query(db, tags, code, 5, 2, 9) == [(-1, -1), (-1, -1)]
    slots, near = kr.add(db, tags, [code, other, code], [0, 1, 7], 1, 9)
    assert slots == [-1, -1, 5] and near == [(0, 0), (3, 0), (-1, -1)] and len(db) == 6 and tags[5] == 7
    slots, near = kr.add(db, tags, [other], [7], 3, 9)
    assert slots == [6] and near == [(5, 3)]  # a distance equal to min_distance is novel
    slots, near = kr.add(db, tags, [code], [7], 4, 9)
    assert slots == [-1] and near == [(5, 0)]


def test_default_ferns_are_in_range_and_use_the_generator_of_synth():
    f = kr.default_ferns(513, 20261020, 192)
    assert f["cell"].min() >= 0 and f["cell"].max() < 192 and f["t_grey"].min() >= 410 and f["t_grey"].max() <= 3686
    assert f["t_depth"].min() >= 512 and f["t_depth"].max() <= 7167 and not f["reserved"].any()
    x = (6364136223846793005 * 20261020 + 1442695040888963407) % (1 << 64)
    assert int(f["cell"][0]) == (x >> 33) % 192
    assert len(set(f["cell"].tolist())) > 150  # the ferns spread over the grid


def test_every_query_is_nearest_to_its_own_keyframe():
    """the premise of the GPU retrieval test"""
    c = kc.retrieval_case()
    n = kc.RET_FERNS
    D = np.array([[kr.distance(q, k, n) for k in c["key_codes"]] for q in c["query_codes"]])
    own = np.diag(D)
    others = D + np.eye(12, dtype=np.int64) * 10000
    print("distances of the twelve queries to their own keyframes:", own.tolist(), "to the nearest other:", others.min(axis=1).tolist())
    assert (D.argmin(axis=1) == np.arange(12)).all()
    assert own.max() <= 10 and others.min() >= 30
    assert (others.min(axis=1) - own).min() >= 10  # own strictly first, with a margin of at least 10 (it is 21)
    assert (c["keyframes"][0][0] > 0).mean() > 0.9 and c["keyframes"][0][0].shape == (kc.RET_ROWS, kc.RET_COLS)
    # added one by one under one tag with min_distance 20, all twelve keyframes are novel (the nearest two are 30 apart)
    db, tags = [], []
    for k in range(12):
        slots, near = kr.add(db, tags, [c["key_codes"][k]], [0], kc.RET_MIN_DISTANCE, n)
        assert slots == [k] and (k == 0 or near[0][1] >= 30), k
    # and a query added on top of them is not
    slots, near = kr.add(db, tags, [c["query_codes"][5]], [0], kc.RET_MIN_DISTANCE, n)
    assert slots == [-1] and near == [(5, int(own[5]))]
