"""Joined and thinned maps (include/sf_join.h, staticfusion_amd/join.py) on the GPU. Every surfel buffer and every count is held
to tests/join_ref.py bit for bit: thins of every size around a wave, a workgroup and the scan's trip, with one voxel for all and
one voxel each, with keys that collide and walks that wrap at 64 slots, with every special confidence and position; the dry run,
the extract and its buffer limits; a batch against single calls; merges with and without a transform, into and from empty maps,
with the confidence test, the stamp, one source for two destinations and the capacity; every refusal; what a call leaves
alone; the state a thin leaves; and one case each on the precise and reference-order libraries."""
import ctypes as C
import os

import numpy as np
import pytest

import join_cases as jc
import join_ref
from join_cases import CELL, TICK
from staticfusion_amd import SfError, SurfelMap, align, join, keyframes, regions, score, view
from test_gpu_view import small_solver, uploaded, walk

pytestmark = pytest.mark.gpu

BIG = 256 * 1024 + 1  # more than 1024 blocks of 256: the second trip of the scan; 2^20 slots
POSE = np.array([[0, -1, 0, 0.25], [1, 0, 0, -1.5], [0, 0, 1, 2.0], [0, 0, 0, 1]], np.float32)
_fp = C.POINTER(C.c_float)
EMPTY = np.zeros((0, 12), np.float32)


@pytest.fixture(scope="module")
def box(hip_auto):
    s = small_solver(hip_auto, 60, 80)
    yield s
    s.close()


def same_bits32(a, b):
    """float32 arrays bit for bit (a NaN made by arithmetic: a NaN in both at the same place)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    a, b = a.ravel(), b.ravel()
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def state(m):
    i = m.info()
    return i["count"], i["tick"], i["pose"].tobytes(), tuple(i["stats"]), m.download().tobytes()


def check_thin(s, surf, cell=CELL, where=""):
    """dry run, extract and thin of one map against the reference; returns (the mask kept, the counts)"""
    want, wc, mask = join_ref.thin(surf, cell)
    n = surf.shape[0]
    m = uploaded(s, surf, pose=POSE, tick=TICK)
    before = state(m)
    assert join.thin([m], join.Params(cell=cell, dry_run=True)) == [wc], where
    assert state(m) == before, where
    got, c = join.thin_extract(m, join.Params(cell=cell))
    assert c == wc and got.tobytes() == want.tobytes(), where
    assert state(m) == before, where
    assert join.thin([m], join.Params(cell=cell)) == [wc], where
    info = m.info()
    assert info["count"] == wc["n_out"] and info["tick"] == TICK and np.array_equal(info["pose"], POSE), where
    assert m.download().tobytes() == want.tobytes(), where
    assert wc["n_out"] == wc["n_voxels"] + wc["n_outside"] and wc["n_in"] == n
    m.close()
    return mask, wc


# ---- 1. thin: sizes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1025, BIG])
def test_thin_sizes_against_the_reference(box, n):
    surf = jc.special_surfels(n, seed=100 + n % 97, box=jc.box_for(n))
    mask, c = check_thin(box, surf, where=n)
    if n >= 255:
        assert c["n_outside"] >= 5 and c["n_voxels"] < 0.8 * n  # voxels are shared, and the special positions are there
    if n == BIG:
        assert join.table_slots(n) == 1 << 20 and (n + 255) // 256 > 1024


# ---- 2. thin: the table under pressure --------------------------------------------------------------------------------
def test_thin_one_voxel_for_all_one_voxel_each_and_colliding_keys(box):
    rng = np.random.default_rng(5)
    # every surfel in one voxel: one address takes every atomic
    one = jc.plain_surfels(1000, seed=6)
    one[:, 0:3] = rng.uniform(0.0201, 0.0399, (1000, 3))
    mask, c = check_thin(box, one, where="one voxel")
    assert c["n_voxels"] == 1 and c["n_out"] == 1
    top = join_ref.ranks(one[:, 3]).max()
    assert mask[np.flatnonzero(join_ref.ranks(one[:, 3]) == top)[0]]
    # every surfel in its own voxel
    own = jc.plain_surfels(1000, seed=7)
    own[:, 0:3] = np.stack([jc.centre_of((i % 10 - 5, (i // 10) % 10 - 5, i // 100 - 5)) for i in range(1000)])
    mask, c = check_thin(box, own[rng.permutation(1000)], where="own voxel")
    assert c["n_voxels"] == 1000 and mask.all()
    # 64 slots: three cells whose first slot is the last one (the walk wraps), five whose first slots coincide; 4 surfels each
    cells = jc.cells_on_slot(64, 63, 3) + jc.cells_on_slot(64, 17, 5, start=5000)
    assert len(set(cells)) == 8
    crowd = jc.plain_surfels(32, seed=8)
    crowd[:, 0:3] = np.stack([jc.centre_of(cells[i % 8]) for i in range(32)])
    assert join.table_slots(32) == 64
    keys, inside = join_ref.voxel_keys(crowd[:, 0:3], CELL)
    assert inside.all() and sorted(join.hash_slot(int(k), 64) for k in set(keys.tolist())) == [17] * 5 + [63] * 3
    mask, c = check_thin(box, crowd, where="colliding keys")
    assert c["n_voxels"] == 8 and c["n_out"] == 8


# ---- 3. thin: ranks and positions by hand -----------------------------------------------------------------------------
def test_thin_special_confidences_and_positions_by_hand(box):
    cell_a, cell_b, cell_c, cell_d, cell_e = (jc.centre_of(q) for q in ((0, 0, 0), (-3, 2, -1), (7, -7, 7), (-1, -1, -1), (40, 0, 0)))
    rows = [  # (position, confidence, kept)
        (cell_a, 0.5, True), (cell_a, 0.5, False), (cell_a, 0.5, False),             # equal confidences: the lowest index wins
        (cell_b, -0.0, False), (cell_b, 0.0, True),                                    # -0 ranks below +0
        (cell_c, 0.0, True), (cell_c, -0.0, False),                                    # ... in either order
        (cell_d, np.nan, False), (cell_d, -np.inf, True),                              # a NaN ranks below every number
        (cell_e, np.nan, True),                                                        # ... and wins a voxel it has alone
        ((np.nan, 0.0, 0.0), 0.1, True), ((0.0, np.inf, 0.0), 0.1, True), ((0.0, 0.0, -np.inf), 0.1, True),  # outside the grid: kept
        ((np.float32(CELL) * np.float32(1 << 20), 0.0, 0.0), 0.2, True), ((np.float32(CELL) * np.float32(1 << 20), 0.0, 0.0), 0.9, True),  # |q| = 2^20
        ((-0.03, -0.01, -0.05), 0.3, False), ((-0.035, -0.005, -0.059), 0.4, True),    # negative coordinates: cell (-2, -1, -3)
        ((0.5, 0.25, 0.0), 0.3, True), ((0.5, 0.25, -0.0), 0.2, False),                # exact borders at cell 0.25 below
    ]
    surf = jc.plain_surfels(len(rows), seed=9)
    for j, (p, conf, _) in enumerate(rows):
        surf[j, 0:3], surf[j, 3] = p, conf
    mask, c = check_thin(box, surf, where="by hand")
    assert mask.tolist() == [r[2] for r in rows]
    assert c["n_outside"] == 5
    # exact borders: at a cell of 0.25, 0.5 and 0.25 are the lower faces of cells 2 and 1
    border = jc.plain_surfels(6, seed=10)
    border[:, 0:3] = [(0.5, 0.25, 0.0), (0.5, 0.25, -0.0), (0.74, 0.49, 0.2), (np.nextafter(np.float32(0.5), np.float32(0)), 0.25, 0.0), (0.75, 0.25, 0.0), (-0.25, -0.5, 0.0)]
    border[:, 3] = [0.1, 0.1, 0.1, 0.9, 0.9, 0.9]
    mask, c = check_thin(box, border, cell=0.25, where="borders")
    assert mask.tolist() == [True, False, False, True, True, True] and c["n_voxels"] == 4


# ---- 4. thin: extract's buffer --------------------------------------------------------------------------------------
def test_thin_extract_buffer_limits(box):
    b = join._bind(box.api)
    surf = jc.special_surfels(1000, seed=3, box=jc.box_for(1000))
    want, wc, _ = join_ref.thin(surf, CELL)
    k = wc["n_out"]
    assert 1 < k < 999
    m = uploaded(box, surf, pose=POSE)
    before = state(m)
    p = join.Params()
    canary = np.full((k, 12), -77.25, np.float32)
    got = join.SfjCounts()
    assert b.thin_extract(m.m, C.byref(p), canary.ctypes.data_as(_fp), k - 1, C.byref(got)) == -1  # SF_ERR_ARG
    assert got.as_dict() == wc and np.all(canary == np.float32(-77.25)) and state(m) == before
    got = join.SfjCounts()
    assert b.thin_extract(m.m, C.byref(p), None, 0, C.byref(got)) == -1 and got.n_out == k and state(m) == before  # the size query
    assert b.thin_extract(m.m, C.byref(p), canary.ctypes.data_as(_fp), k, C.byref(got)) == 0 and canary.tobytes() == want.tobytes()
    m.close()
    e = uploaded(box, EMPTY, pose=POSE)
    got.n_out = -5
    assert b.thin_extract(e.m, C.byref(p), None, 0, C.byref(got)) == 0 and got.as_dict() == join_ref.counts()  # nothing kept: SF_OK
    e.close()


# ---- 5. thin: batch ---------------------------------------------------------------------------------------------------
def test_a_batch_of_thins_equals_single_calls_and_the_reference(box):
    sizes = [0, 257, 70000, 1, 300, 5000, 640]
    cells = [0.02, 0.01, 0.05, 0.02, 0.3, 0.02, 0.02]
    dry = [False, False, False, False, False, True, False]
    data = [jc.special_surfels(n, seed=20 + q, box=jc.box_for(n)) for q, n in enumerate(sizes)]
    want = [join_ref.thin(d, c) for d, c in zip(data, cells)]
    params = [join.Params(cell=c, dry_run=d) for c, d in zip(cells, dry)]
    results = []
    for batched in (True, False):
        maps = [uploaded(box, d, pose=POSE) for d in data]
        if batched:
            got = join.thin(maps[:6], params[:6])  # one sfj_thin_maps; the seventh map is not named
        else:
            got = [join.thin([m], [p])[0] for m, p in zip(maps[:6], params[:6])]
        assert got == [w[1] for w in want[:6]]
        results.append([m.download() for m in maps])
        for m in maps:
            m.close()
    for q in range(7):
        expect = want[q][0] if q < 5 else data[q]  # the dry run and the map not named keep everything
        assert results[0][q].tobytes() == expect.tobytes() and results[1][q].tobytes() == expect.tobytes(), q
    assert 0 < want[2][1]["n_out"] < 70000 and want[4][1]["n_voxels"] <= 8 + 18  # a cell of 0.3: the 8 around the origin, and the special positions


# ---- 6. merge ---------------------------------------------------------------------------------------------------------
def check_merge(s, d, sr, M=None, capacity=0, where="", **kw):
    """dry run and merge of one pair against the reference; returns the counts"""
    want, wc = join_ref.merge(d, sr, M, **kw)
    md = uploaded(s, d, pose=POSE, tick=TICK, capacity=capacity or max(d.shape[0] + sr.shape[0], s.rows * s.cols))
    ms = uploaded(s, sr, tick=TICK - 1)
    before = state(md), state(ms)
    kw.setdefault("cell", CELL)
    assert join.merge([md], [ms], None if M is None else [M], join.Params(dry_run=True, **kw)) == [wc], where
    assert (state(md), state(ms)) == before, where
    assert join.merge([md], [ms], None if M is None else [M], join.Params(**kw)) == [wc], where
    assert state(ms) == before[1], where  # the source is never changed
    info, got = md.info(), md.download()
    assert info["count"] == d.shape[0] + wc["n_out"] and info["tick"] == TICK and np.array_equal(info["pose"], POSE), where
    assert got[: d.shape[0]].tobytes() == d.tobytes(), where  # the destination's own surfels are not touched
    assert same_bits32(got, want), where
    added, ref_added = got[d.shape[0]:], want[d.shape[0]:]
    assert added[:, [3, 4, 5, 6, 7, 11]].tobytes() == ref_added[:, [3, 4, 5, 6, 7, 11]].tobytes(), where
    md.close()
    ms.close()
    return wc


def test_merge_identity_transform_null_and_the_same_map(box):
    d = jc.special_surfels(2000, seed=31)
    sr = jc.special_surfels(1500, seed=32)
    ident = check_merge(box, d, sr, np.eye(4, dtype=np.float32), where="identity")
    assert check_merge(box, d, sr, None, where="T = NULL") == ident
    moved = check_merge(box, d, sr, jc.rigid(), where="rigid")
    assert ident["n_shared"] > 100 and moved["n_shared"] > 100 and ident["n_out"] > 100 and moved != ident and ident["n_outside"] >= 5
    # a source equal to the destination adds only the surfels outside the grid
    same = check_merge(box, d, d.copy(), None, where="the same surfels")
    assert same["n_out"] == same["n_outside"] > 0 and same["n_shared"] == 2000 - same["n_outside"]
    # a large source, a small destination: several workgroups, a table of 64 slots
    check_merge(box, d[:20], jc.special_surfels(70001, seed=33, box=jc.box_for(70001)), jc.rigid(3), where="large source")
    check_merge(box, jc.special_surfels(70001, seed=34), sr, jc.rigid(4), where="large destination")


def test_merge_empty_maps_confidence_and_stamp(box):
    sr = jc.special_surfels(700, seed=41)
    c = check_merge(box, EMPTY, sr, jc.rigid(), where="empty destination")
    assert c["n_out"] == 700 and c["n_voxels"] == 0
    c = check_merge(box, sr, EMPTY, jc.rigid(), where="empty source")
    assert c == join_ref.counts(n_voxels=c["n_voxels"]) and c["n_voxels"] > 0
    assert check_merge(box, EMPTY, EMPTY, None, where="both empty") == join_ref.counts()
    # min_confidence: exactly at it, one float below it, NaN
    at = np.float32(0.25)
    conf = jc.plain_surfels(6, seed=42)
    conf[:, 0:3] = np.stack([jc.centre_of((3 * i, 0, 0)) for i in range(6)])
    conf[:, 3] = [at, np.nextafter(at, np.float32(0)), np.nan, np.nextafter(at, np.float32(1)), np.inf, -1.0]
    c = check_merge(box, sr, conf, None, min_confidence=float(at), where="min_confidence")
    assert c["n_below"] == 3 and c["n_out"] + c["n_shared"] == 3
    c = check_merge(box, EMPTY, conf, None, min_confidence=0.0, where="no confidence test")  # 0 disables: the NaN is added too
    assert c["n_below"] == 0 and c["n_out"] == 6
    c = check_merge(box, EMPTY, conf, None, min_confidence=-1.0, where="a negative min_confidence is no test")
    assert c["n_below"] == 0 and c["n_out"] == 6
    for stamp in (-1, 0, 7):
        check_merge(box, jc.special_surfels(300, seed=43), sr, jc.rigid(), stamp=stamp, min_confidence=0.1, where="stamp %d" % stamp)


def test_merge_one_source_into_two_destinations_and_the_capacity(hip_auto):
    s = small_solver(hip_auto, 30, 40)
    cap = s.rows * s.cols
    sr = jc.special_surfels(500, seed=51)
    d1, d2 = jc.special_surfels(300, seed=52), jc.special_surfels(64, seed=53)
    M = [jc.rigid(1), np.eye(4, dtype=np.float32)]
    kw = [dict(cell=0.02, stamp=3), dict(cell=0.05, min_confidence=0.3)]
    want = [join_ref.merge(d, sr, m, **k) for d, m, k in zip((d1, d2), M, kw)]
    ms, m1, m2 = uploaded(s, sr), uploaded(s, d1, pose=POSE), uploaded(s, d2)
    assert join.merge([m1, m2], [ms, ms], M, [join.Params(**k) for k in kw]) == [w[1] for w in want]
    assert same_bits32(m1.download(), want[0][0]) and same_bits32(m2.download(), want[1][0]) and ms.download().tobytes() == sr.tobytes()
    assert want[0][1] != want[1][1]
    # the capacity: a destination far from the source takes all 500; one surfel too many is SF_ERR_STATE and nothing changes
    far = jc.plain_surfels(cap - 500 + 1, seed=54)
    far[:, 0] += 50.0
    full = uploaded(s, far, pose=POSE, capacity=cap)
    m1.upload(d1, POSE, TICK)
    before = state(full), state(ms), state(m1)
    b = join._bind(s.api)
    out = (join.SfjCounts * 2)()
    two_dst, two_src = (C.c_void_p * 2)(m1.m.value, full.m.value), (C.c_void_p * 2)(ms.m.value, ms.m.value)
    pr = (join.SfjParams * 2)(join.Params(), join.Params())
    assert b.merge_maps(s.h, 2, two_dst, two_src, None, pr, out) == -3  # SF_ERR_STATE: the second entry does not fit
    assert b"capacity" in s.api.last_error()
    assert (state(full), state(ms), state(m1)) == before and out[1].n_out == 500
    with pytest.raises(SfError, match="capacity"):
        join.merge([full], [ms])
    assert join.merge([full], [ms], params=join.Params(dry_run=True))[0]["n_out"] == 500  # a dry run only counts
    assert (state(full), state(ms)) == before[:2]
    full.upload(far[:-1], POSE, TICK)  # one surfel fewer: exactly the capacity
    assert join.merge([full], [ms])[0]["n_out"] == 500 and full.info()["count"] == cap
    assert same_bits32(full.download(), join_ref.merge(far[:-1], sr)[0])
    for m in (ms, m1, m2, full):
        m.close()
    s.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(box, hip_auto):
    s = box
    b = join._bind(s.api)
    cap = s.rows * s.cols
    m1, m2, m3 = SurfelMap(s, cap), SurfelMap(s, cap), SurfelMap(s, cap)
    d1, d2 = jc.special_surfels(300, seed=1), jc.special_surfels(65, seed=2)
    m1.upload(d1, POSE, TICK)
    m2.upload(d2, POSE, TICK)
    m3.upload(d2, POSE, TICK)
    other = small_solver(hip_auto, 60, 80)
    mo = SurfelMap(other, cap)
    mo.upload(d2, POSE, TICK)
    before = [state(m) for m in (m1, m2, m3, mo)]
    arr = lambda *ms: (C.c_void_p * len(ms))(*[None if m is None else m.m.value for m in ms])  # noqa: E731
    two, twice, foreign, with_null = arr(m1, m2), arr(m1, m1), arr(m1, mo), arr(m1, None)
    good = (join.SfjParams * 2)(join.Params(), join.Params())
    nan, inf = float("nan"), float("inf")
    bad = [(join.SfjParams * 2)(join.Params(), join.Params(**kw)) for kw in (dict(cell=nan), dict(cell=0.0), dict(cell=-1.0), dict(cell=inf), dict(cell=1e-45),
                                                                              dict(min_confidence=nan))]
    dry2 = (join.SfjParams * 2)(join.Params(), join.Params())
    dry2[1].dry_run = 2
    bad.append(dry2)
    out = (join.SfjCounts * 2)()
    C.memset(out, 0xFB, C.sizeof(out))  # a sentinel in every field
    sentinel = bytes(out)
    buf = np.full((400, 12), -77.25, np.float32)
    # thin
    cases = [(None, 2, two, good, out), (s.h, 2, None, good, out), (s.h, 2, two, None, out), (s.h, 2, two, good, None), (s.h, -1, two, good, out),
             (s.h, 2, foreign, good, out), (other.h, 2, two, good, out), (s.h, 2, twice, good, out), (s.h, 2, with_null, good, out)]
    cases += [(s.h, 2, two, x, out) for x in bad]
    for q, args in enumerate(cases):
        assert b.thin_maps(*args) == -1, q
        assert s.api.last_error(), q
    assert b.thin_maps(s.h, 0, None, None, None) == 0  # an empty batch is fine
    # extract
    p = good[0]
    one = C.cast(out, C.POINTER(join.SfjCounts))
    cases = [(None, C.byref(p), buf.ctypes.data_as(_fp), 400, one), (m1.m, None, buf.ctypes.data_as(_fp), 400, one), (m1.m, C.byref(p), None, 400, one),
             (m1.m, C.byref(p), buf.ctypes.data_as(_fp), -1, one), (m1.m, C.byref(p), buf.ctypes.data_as(_fp), 400, None)]
    cases += [(m1.m, C.byref(x[1]), buf.ctypes.data_as(_fp), 400, one) for x in bad]
    for q, args in enumerate(cases):
        assert b.thin_extract(*args) == -1, q
    # merge
    src2 = arr(m3, m3)
    t_ok = np.tile(np.eye(4, dtype=np.float32).reshape(-1), 2)
    t_bad = []
    for v in (nan, inf, -inf):
        t = t_ok.copy()
        t[16 + 13] = v
        t_bad.append(t)
    tp = lambda t: t.ctypes.data_as(_fp)  # noqa: E731
    cases = [(None, 2, two, src2, tp(t_ok), good, out), (s.h, 2, None, src2, tp(t_ok), good, out), (s.h, 2, two, None, tp(t_ok), good, out),
             (s.h, 2, two, src2, tp(t_ok), None, out), (s.h, 2, two, src2, tp(t_ok), good, None), (s.h, -1, two, src2, tp(t_ok), good, out),
             (s.h, 2, foreign, src2, None, good, out), (s.h, 2, two, foreign, None, good, out), (other.h, 2, two, src2, None, good, out),
             (s.h, 2, twice, src2, None, good, out), (s.h, 2, with_null, src2, None, good, out), (s.h, 2, two, with_null, None, good, out),
             (s.h, 2, two, arr(m3, m1), None, good, out),   # m1: a destination in entry 0, a source in entry 1
             (s.h, 2, two, arr(m1, m3), None, good, out),   # ... and its own source
             (s.h, 1, arr(m1), arr(m1), None, good, out)]
    cases += [(s.h, 2, two, src2, tp(t), good, out) for t in t_bad]
    cases += [(s.h, 2, two, src2, None, x, out) for x in bad]
    for q, args in enumerate(cases):
        assert b.merge_maps(*args) == -1, q
        assert s.api.last_error(), q
    assert b.merge_maps(s.h, 0, None, None, None, None, None) == 0
    with pytest.raises(SfError):
        join.thin([m1, mo])  # maps of two solvers
    with pytest.raises(SfError):
        join.thin([m1, m1])
    with pytest.raises(SfError):
        join.merge([m1], [m1])
    with pytest.raises(SfError):
        join.thin([m1], join.Params(cell=nan))
    assert bytes(out) == sentinel and np.all(buf == np.float32(-77.25))
    assert [state(m) for m in (m1, m2, m3, mo)] == before
    # the handle goes first: the map is an empty shell that fails cleanly
    other.close()
    one_map = arr(mo)
    assert b.thin_maps(s.h, 1, one_map, good, out) == -3 and b.thin_extract(mo.m, C.byref(p), buf.ctypes.data_as(_fp), 400, one) == -3  # SF_ERR_STATE
    assert b.merge_maps(s.h, 1, arr(m1), one_map, None, good, out) == -3 and b.merge_maps(s.h, 1, one_map, arr(m1), None, good, out) == -3
    assert bytes(out) == sentinel and np.all(buf == np.float32(-77.25)) and [state(m) for m in (m1, m2, m3)] == before[:3]
    # and the live maps still work
    assert join.thin([m1, m2]) == [join_ref.thin(d, CELL)[1] for d in (d1, d2)]
    assert join.merge([m1], [m3])[0] == join_ref.merge(join_ref.thin(d1, CELL)[0], d2)[1]
    for m in (m1, m2, m3, mo):
        m.close()


# ---- 8. what a call leaves alone; the state a thin leaves -------------------------------------------------------------
@pytest.fixture(scope="module")
def walked(hip_auto):
    s, m, out = walk(hip_auto, 5, render_between=False)
    yield s, m, out
    m.close()
    s.close()


def test_a_join_call_leaves_everything_else_alone(walked):
    s, m, out = walked
    SurfelMap.predict_frames(s, [0], [m], s.default_model_params())
    v = view.default_view(s, m)
    big = view.View(view.look_at((0.4, 0.2, -0.6), (0.0, 0.0, 2.0)), 150.0, 100.0, 250.0, 250.0, 200, 300, min_confidence=0.0)
    db = keyframes.KeyframeDb(s, 10, n_ferns=64)
    db.add_streams([0], [np.eye(4)], [0])
    view.render([m, m], [v, big])

    def readable():
        i = m.info()
        sc_ = score.score_streams([m], [v], [0])
        summ, reg = regions.label_streams(s, [0])
        res = align.refine_streams([m], [v], [0], align.Params(iterations=2))
        return (i["count"], i["tick"], i["pose"].tobytes(), tuple(i["stats"]), m.download().tobytes(), m.index_map().tobytes(),
                s.prediction()[0].tobytes(), s.prediction()[1].tobytes(), s.prediction_dense_stream(0), s.current(0)[0].tobytes(), s.b_image(0).tobytes(),
                sc_.tobytes(), db.query_streams([0]).tobytes(), db.encode_streams([0]).tobytes(), summ.tobytes(), res.tobytes(),
                tuple(view.last_large_sprites(s, 2)))

    before = readable()
    surf = m.download()
    small = uploaded(s, surf[:100], pose=POSE)
    assert join.thin([small], join.Params(dry_run=True))[0] == join_ref.thin(surf[:100], CELL)[1]
    assert readable() == before
    # larger calls grow the scratch: the map itself extracted, then merged into a map of 70 000 surfels and back from it
    got, c = join.thin_extract(m)
    want, wc, _ = join_ref.thin(surf, CELL)
    assert c == wc and got.tobytes() == want.tobytes()
    assert readable() == before
    large = jc.special_surfels(70000, seed=61)
    other = uploaded(s, large, capacity=70000 + surf.shape[0])
    assert join.merge([other, small], [m, m], [jc.rigid(), np.eye(4)])[0] == join_ref.merge(large, surf, jc.rigid())[1]
    assert readable() == before
    for x in (small, other):
        x.close()
    db.close()


def test_a_fused_map_thinned_and_the_state_a_thin_leaves(walked):
    s, m, out = walked
    info, surf = m.info(), m.download()
    assert m.index_map().max() > 0 and surf.shape[0] > 3000
    want, wc, _ = join_ref.thin(surf, CELL)
    assert join.thin([m], join.default_params()) == [wc] and 0 < wc["n_out"] < surf.shape[0]  # several surfels of a real map share a 2 cm voxel
    assert m.download().tobytes() == want.tobytes()
    with pytest.raises(SfError, match="index map"):
        m.index_map()
    after = m.info()
    assert after["count"] == wc["n_out"] and after["tick"] == info["tick"] and np.array_equal(after["pose"], info["pose"]) and after["stats"] == info["stats"]
    # the prediction straight after the thin is the prediction from the reference's array
    m.predict(0)
    d1, i1 = s.prediction()
    mp = s.default_model_params()
    mp.time = mp.max_time = info["tick"]
    s.predict_from_model(0, want, info["pose"], mp)
    d2, i2 = s.prediction()
    assert d1.tobytes() == d2.tobytes() and i1.tobytes() == i2.tobytes() and (d1 > 0).any()
    # ... and the next fuse works and renders a new index image
    SurfelMap.fuse_frames(s, [0], [m], list(s.batch_results()[0]), 1.0, s.default_model_params())
    assert m.index_map().max() > 0 and m.info()["tick"] == info["tick"] + 1


# ---- 9. the other two libraries link the same object -----------------------------------------------------------------
@pytest.mark.parametrize("lib", ["libsf_hip_precise.so", "libsf_hip_reforder.so"])
def test_the_precise_and_reference_order_libraries_join_the_same(lib):
    import staticfusion_amd as sf

    api = sf.Api(os.path.join(os.path.dirname(sf.LIB), lib), "sf_")
    s = small_solver(api, 60, 80)
    check_thin(s, jc.special_surfels(1025, seed=71, box=jc.box_for(1025)), where=lib)
    c = check_merge(s, jc.special_surfels(700, seed=72), jc.special_surfels(600, seed=73), jc.rigid(), stamp=4, min_confidence=0.2, where=lib)
    assert c["n_shared"] > 10 and c["n_below"] > 10
    s.close()
