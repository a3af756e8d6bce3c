"""Shared set-up of the join tests (test_join_reference_cpu.py, test_gpu_join.py): surfel sets whose voxels are shared by
several surfels, with every special value of include/sf_join.h among them, positions at the centre of given cells, and cells
found by search whose keys fall on given slots of a table."""
import numpy as np

import join_ref

CELL = 0.02
TICK = 10


def centre_of(q, cell=CELL):
    """a position whose cell index is q (three integers), checked with the reference"""
    p = ((np.asarray(q, np.float64) + 0.5) * cell).astype(np.float32)
    want = ((int(q[0]) + (1 << 20)) << 42) | ((int(q[1]) + (1 << 20)) << 21) | (int(q[2]) + (1 << 20))
    assert join_ref.voxel_key(p, cell) == want, (q, p)
    return p


def plain_surfels(n, seed, box=0.2):
    """n surfels with positions uniform in [-box, box]^3 (at CELL and box 0.2: 8000 cells), confidences from a few values so that
    ranks tie, and from a continuous range; colours, times, unit normals, radii"""
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 12), np.float32)
    s[:, 0:3] = rng.uniform(-box, box, (n, 3))
    tied = rng.choice(np.array([0.1, 0.25, 0.5, 0.5, 1.0], np.float32), n)
    s[:, 3] = np.where(rng.uniform(size=n) < 0.5, tied, rng.uniform(0.0, 1.0, n).astype(np.float32))
    s[:, 4] = (rng.integers(1, 256, n) << 16) + (rng.integers(1, 256, n) << 8) + rng.integers(1, 256, n)
    s[:, 5] = np.arange(n) % 1000  # (not read by anybody: it tells the surfels of a set apart)
    s[:, 7] = rng.integers(1, TICK + 1, n)
    s[:, 6] = np.minimum(s[:, 7], rng.integers(1, TICK + 1, n))
    nrm = rng.normal(size=(n, 3))
    s[:, 8:11] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    s[:, 11] = rng.uniform(0.001, 0.05, n)
    return s


def box_for(n, per_cell=3.0, cell=CELL):
    """half the edge of a cube of whole cells that holds about n / per_cell of them"""
    return max(1, round((max(n, 1) / per_cell) ** (1.0 / 3.0))) * cell / 2


def special_surfels(n, seed, cell=CELL, box=0.2):
    """plain_surfels with, spread over the set: NaN and +-inf positions, |q| = 2^20 and 2^20 - 1 on both sides, positions on
    exact cell borders, -0.0 coordinates, NaN / -0 / +0 / negative / inf confidences"""
    s = plain_surfels(n, seed, box)
    edge = np.float32(cell) * np.float32(1 << 20)
    inside_edge = np.float32(cell) * np.float32((1 << 20) - 1)
    special = [(0, np.nan), (1, np.inf), (2, -np.inf), (0, edge), (1, -edge), (2, inside_edge), (0, -inside_edge), (1, np.float32(3e38)),
               (0, np.float32(cell) * 3), (1, -np.float32(cell) * 2), (2, np.float32(-0.0)), (0, 0.0),
               (3, np.nan), (3, np.float32(-0.0)), (3, 0.0), (3, -1.0), (3, np.inf), (3, -np.inf)]
    for j, (col, v) in enumerate(special):
        if n:
            s[(j * 7 + 3) % n, col] = v
    return s


def cells_on_slot(slots, first_slot, how_many, start=0):
    """`how_many` distinct cells (q_x, 0, 0), q_x >= start, whose keys' first slot in a table of `slots` is first_slot: found by
    search with the reference's hash"""
    found, qx = [], start
    while len(found) < how_many:
        q = (qx, 0, 0)
        key = ((q[0] + (1 << 20)) << 42) | ((1 << 20) << 21) | (1 << 20)
        if join_ref.hash_slot(key, slots) == first_slot:
            found.append(q)
        qx += 1
        assert qx < start + 100000
    return found


def rigid(seed=5):
    """a rotation plus a translation, 4 x 4 float32"""
    rng = np.random.default_rng(seed)
    a, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(a) < 0:
        a[:, 0] = -a[:, 0]
    M = np.eye(4, dtype=np.float32)
    M[:3, :3] = a
    M[:3, 3] = (0.013, -0.021, 0.034)
    return M
