"""The voxel key, the hash and the table size of include/sf_join.h without a GPU: sfj_voxel_key, sfj_hash_slot and
sfj_table_slots of the library held bit for bit against tests/join_ref.py -- by hand, on cell borders, at both ends of the grid,
on every special value and on 10 000 random positions --, the ranks by hand, and the reference's own premises checked with the
reference alone."""
import numpy as np

import join_cases as jc
import join_ref
from staticfusion_amd import join
from staticfusion_amd.synth import LCG64

BIAS = 1 << 20


def key_of(q):
    return ((q[0] + BIAS) << 42) | ((q[1] + BIAS) << 21) | (q[2] + BIAS)


def both(pos, cell):
    """the library's key and the reference's, which agree"""
    got = join.voxel_key(join.Params(cell=cell), pos)
    want = join_ref.voxel_key(pos, cell)
    assert got == want, (pos, cell, got, want)
    return got


def test_keys_by_hand_on_borders_at_the_ends_and_on_special_values():
    assert both((0.03, -0.01, 0.0), 0.02) == key_of((1, -1, 0))
    assert both((0.0, -0.0, 0.0), 0.02) == key_of((0, 0, 0))  # -0.0 * inv = -0.0, floor -0.0, cell 0
    assert key_of((0, 0, 0)) < (1 << 63) and key_of((BIAS - 1,) * 3) < (1 << 63)  # the top bit of a key is clear
    # exact multiples of the cell (cells that are powers of two: p * inv is exact)
    for cell in (0.5, 0.25, 0.015625):
        for k in (-5, -1, 0, 1, 2, 7, 1000):
            assert both((k * cell, 0.0, -k * cell), cell) == key_of((k, 0, -k)), (cell, k)
            below = float(np.nextafter(np.float32(k * cell), np.float32(-1e9)))
            assert both((below, 0.0, 0.0), cell) == key_of((k - 1, 0, 0)), (cell, k)
    # ... and of 0.02, whose inverse is rounded: whatever fp32 gives, the library gives
    for k in range(-300, 300):
        both((np.float32(k) * np.float32(0.02), np.float32(k * 0.02), 0.0), 0.02)
    # the ends of the grid: |q| = 2^20 - 1 inside, 2^20 outside, on every axis (cell 1: q = floor(p))
    last = float(BIAS - 1)
    for axis in range(3):
        for sign in (1.0, -1.0):
            p = [0.5, 0.5, 0.5]
            p[axis] = sign * last
            q = [0, 0, 0]
            q[axis] = int(sign * last)
            assert both(p, 1.0) == key_of(q)
            p[axis] = sign * float(BIAS)
            assert both(p, 1.0) is None
    assert both((last + 0.5, 0.0, 0.0), 1.0) == key_of((BIAS - 1, 0, 0))
    assert both((-last - 0.5, 0.0, 0.0), 1.0) is None  # floor(-(2^20 - 1) - 0.5) = -2^20
    assert both((last, last, last), 1.0) == key_of((BIAS - 1,) * 3) and both((-last, -last, -last), 1.0) == key_of((1 - BIAS,) * 3)
    # NaN and +-inf, on every axis
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            p = [0.01, 0.01, 0.01]
            p[axis] = bad
            assert both(p, 0.02) is None
    # a cell so small that p * inv overflows (inv = 2^126; 8 * 2^126 = 2^129), and one where it is merely huge
    small = float(np.float32(2.0 ** -126))
    assert both((8.0, 0.0, 0.0), small) is None and both((-8.0, 0.0, 0.0), small) is None and both((1.0, 0.0, 0.0), small) is None
    assert both((0.0, 0.0, 0.0), small) == key_of((0, 0, 0))


def test_ten_thousand_positions_the_hash_and_the_table_size():
    rng = LCG64(2024)
    cells = (0.02, 0.01, 0.05, 0.3, 1e-5)
    pos = np.array([[rng.uniform(-30.0, 30.0) for _ in range(3)] for _ in range(10000)], np.float32)
    for j, cell in enumerate(cells):
        part = pos[j::len(cells)]
        keys, inside = join_ref.voxel_keys(part, cell)
        p = join.Params(cell=cell)
        got = [join.voxel_key(p, x) for x in part]
        assert got == [int(k) if i else None for k, i in zip(keys.tolist(), inside.tolist())], cell
        assert inside.all() == (cell > 1e-4) and inside.any()  # at cell 1e-5 the grid ends at about 10.5 m
        for k in keys[inside][:400].tolist():
            for slots in (64, 128, 4096, 1 << 20, 1 << 30):
                assert join.hash_slot(k, slots) == join_ref.hash_slot(k, slots), (k, slots)
    for key in (0, 1, join_ref.EMPTY, join_ref.EMPTY - 1, 1 << 63, key_of((0, 0, 0))):
        for slots in (64, 1 << 30):
            assert join.hash_slot(key, slots) == join_ref.hash_slot(key, slots)
    assert join_ref.hash_slot(1, 64) == 0x9E3779B97F4A7C15 >> 58
    for count, want in ((0, 64), (1, 64), (32, 64), (33, 128), (64, 128), (65, 256), (1025, 4096), (256 * 1024, 1 << 19), (256 * 1024 + 1, 1 << 20),
                        (1 << 29, 1 << 30)):
        assert join.table_slots(count) == want == join_ref.table_slots(count), count


def test_ranks_by_hand():
    conf = np.array([np.nan, -1.0, -0.0, 0.0, 0.08, 1.0, -np.inf, np.inf, -np.nan], np.float32)
    r = join_ref.ranks(conf).tolist()
    assert r[0] == 0 and r[8] == 0
    assert r[1] == 0xFFFFFFFF ^ 0xBF800000 and r[2] == 0x7FFFFFFF and r[3] == 0x80000000
    assert r[4] == 0x80000000 | int(np.float32(0.08).view(np.uint32)) and r[5] == 0xBF800000
    assert r[0] < r[6] < r[1] < r[2] < r[3] < r[4] < r[5] < r[7]


def test_the_premises_of_the_reference():
    s = jc.special_surfels(3000, seed=1)
    kept, c, mask = join_ref.thin(s, jc.CELL)
    assert c["n_out"] == c["n_voxels"] + c["n_outside"] == kept.shape[0] and 0 < c["n_outside"] < 20 and c["n_voxels"] < 2800
    again, c2, mask2 = join_ref.thin(kept, jc.CELL)
    assert again.tobytes() == kept.tobytes() and mask2.all() and c2["n_voxels"] == c["n_voxels"]  # idempotent
    # the winner of a voxel: no surfel of the voxel ranks higher, none of equal rank comes earlier
    keys, inside = join_ref.voxel_keys(s[:, 0:3], jc.CELL)
    rk = join_ref.ranks(s[:, 3])
    for e in np.flatnonzero(mask & inside)[:300].tolist():
        same = np.flatnonzero(keys == keys[e])
        assert rk[same].max() == rk[e] and same[rk[same] == rk[e]].min() == e
    # merged with itself at the identity a map gains exactly its outside-grid surfels (those that keep their bits)
    merged, cm = join_ref.merge(s, s, None, jc.CELL)
    assert cm["n_out"] == cm["n_outside"] == c["n_outside"] and cm["n_shared"] == 3000 - c["n_outside"] and cm["n_voxels"] == c["n_voxels"]
    assert merged.shape[0] == 3000 + c["n_outside"] and merged[:3000].tobytes() == s.tobytes()
    # a merge into an empty map adds every surfel that passes
    into_empty, ce = join_ref.merge(np.zeros((0, 12), np.float32), s, jc.rigid(), jc.CELL, min_confidence=0.25, stamp=7)
    passes = s[:, 3] >= np.float32(0.25)
    assert ce["n_out"] == int(passes.sum()) == into_empty.shape[0] and ce["n_shared"] == 0 and ce["n_voxels"] == 0 and ce["n_below"] == 3000 - ce["n_out"]
    assert (into_empty[:, 6] == 7).all() and (into_empty[:, 7] == 7).all()
    assert into_empty[:, [3, 4, 5, 11]].tobytes() == s[passes][:, [3, 4, 5, 11]].tobytes()
    # collisions can be built: five cells on one slot, three on the last slot of a table of 64
    assert len(jc.cells_on_slot(64, 63, 3)) == 3 and len(set(jc.cells_on_slot(64, 17, 5))) == 5
