"""Place recognition (include/sf_keyframes.h, staticfusion_amd/keyframes.py) on the GPU. Every comparison is integer equality
with the NumPy statement of the header in tests/keyframe_ref.py: image sizes on every load width of the encode kernel (4, 2
and 1 floats per lane) crossed with fern counts around the word size, frames with 0 / NaN / inf / negative depths and
NaN / out-of-range greys, a batch against single calls, the three encode forms against one another, queries over database
counts around the wave and workgroup sizes with exact ties and tag filters, the novelty rule of add, checkpoint and resume,
the state a keyframe call must leave alone, every refusal, and the retrieval of twelve views of a room."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import keyframe_cases as kc
import keyframe_ref as kr
import test_gpu_view as tv
from conftest import ROOT, hip_runtime
from staticfusion_amd import SfError, keyframes, score, view
from test_gpu_view import random_surfels, small_solver, uploaded, walk
from test_map_fusion import same_bits

pytestmark = pytest.mark.gpu

# rows, cols, cell: one cell; the smallest image; nothing a multiple of anything; an odd row count (one float per lane) with
# a remainder in both directions; four floats per lane and several items per lane; two floats per lane and 64 x 64 cells
SIZES = [(8, 8, 8), (1, 1, 1), (5, 7, 3), (53, 37, 8), (64, 48, 4), (130, 66, 64)]
FERN_COUNTS = [1, 7, 8, 9, 64, 65, 513]


@pytest.fixture(scope="module")
def box(hip_auto):
    s = small_solver(hip_auto, 60, 80)
    yield s
    s.close()


def frames_of(rows, cols, seed):
    """three frames: special values by position, a plain one, and one without any valid depth"""
    rng = np.random.default_rng(seed)
    plain = (rng.uniform(0.4, 6.0, (rows, cols)).astype(np.float32), rng.random((rows, cols)).astype(np.float32))
    empty = (np.zeros((rows, cols), np.float32), np.full((rows, cols), np.nan, np.float32))
    return [kc.special_frame(rows, cols, seed), plain, empty]


def as_list(matches_row):
    return [(int(s), int(d)) for s, d in zip(matches_row["slot"], matches_row["distance"])]


def random_codes(n, n_ferns, seed, pool=5, flips=3):
    """n codes near one of `pool` base codes (at most `flips` nibbles away): many exact distance ties"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 8, (pool, n_ferns))
    out = []
    for q in range(n):
        nib = base[rng.integers(0, pool)].copy()
        for _ in range(int(rng.integers(0, flips + 1))):
            nib[rng.integers(0, n_ferns)] = rng.integers(0, 8)
        out.append(kr.pack(nib.astype(np.uint32)))
    return np.array(out, np.uint32).reshape(n, (n_ferns + 7) // 8)


def poses_of(n, seed=0):
    return np.random.default_rng(seed).normal(size=(n, 4, 4)).astype(np.float32)


# ---- 1. encode: sizes x fern counts, frames with every special value ------------------------------------------------------
@pytest.mark.parametrize("rows,cols,cell", SIZES)
def test_encode_equals_numpy(box, rows, cols, cell):
    gr, gc = kr.grid(rows, cols, cell)
    frames = frames_of(rows, cols, seed=rows * 100 + cols)
    seen = set()
    for n_ferns in FERN_COUNTS:
        ferns = kc.spread_ferns(n_ferns, gr * gc, seed=n_ferns)
        db = keyframes.KeyframeDb(box, cell, ferns=ferns, capacity=4, rows=rows, cols=cols)
        info = db.info()
        assert (info["grid_rows"], info["grid_cols"], info["n_ferns"], info["words"], info["count"]) == (gr, gc, n_ferns, (n_ferns + 7) // 8, 0)
        got = db.encode_images([f[0] for f in frames], [f[1] for f in frames])
        assert got.dtype == np.uint32 and got.shape == (3, (n_ferns + 7) // 8)
        for q, (d, g) in enumerate(frames):
            want = kr.encode(d, g, ferns, cell)
            assert np.array_equal(got[q], want), (n_ferns, q, got[q], want)
            seen |= set(kr.unpack(want, n_ferns).tolist())
        if n_ferns % 8:
            assert (got[:, -1] >> np.uint32(4 * (n_ferns % 8)) == 0).all()  # unused nibbles are 0
        db.close()
    assert seen <= set(range(8)) and len(seen) >= (2 if rows * cols == 1 else 5)  # the cases reach most nibble values


# ---- 2. a batch against single calls; the three forms --------------------------------------------------------------------
def batch_case(s):
    rows, cols, cell = 64, 48, 4
    ferns = kc.spread_ferns(65, (rows // cell) * (cols // cell), seed=2)
    db = keyframes.KeyframeDb(s, cell, ferns=ferns, capacity=8, rows=rows, cols=cols)
    frames = frames_of(rows, cols, seed=1) + frames_of(rows, cols, seed=2)
    frames[4] = frames[0]  # one frame twice
    return db, ferns, frames


def test_a_batch_equals_single_calls_and_device_pointers(box):
    db, ferns, frames = batch_case(box)
    got = db.encode_images([f[0] for f in frames], [f[1] for f in frames])
    for q, (d, g) in enumerate(frames):
        assert np.array_equal(db.encode_images([d], [g])[0], got[q]), q
        assert np.array_equal(got[q], kr.encode(d, g, ferns, 4)), q
    assert np.array_equal(got[0], got[4]) and not np.array_equal(got[0], got[1])
    # at the C interface: the code of a seventh entry is left alone
    col = [[np.ascontiguousarray(f[k].T) for f in frames] for k in range(2)]
    ptrs = [(C.c_void_p * 6)(*[a.ctypes.data for a in col[k]]) for k in range(2)]
    raw = np.full((7, db.words), 0xabcdabcd, np.uint32)
    assert db.b.encode_images(db.db, 6, ptrs[0], ptrs[1], raw.ctypes.data) == 0
    assert np.array_equal(raw[:6], got) and (raw[6] == 0xabcdabcd).all()
    # device pointers (plain hipMalloc memory), aligned and -- four bytes into a block -- not: the same codes
    rt = hip_runtime()
    blocks = []

    def dev(a, shift=0):
        p = C.c_void_p()
        assert rt.hipMalloc(C.byref(p), C.c_size_t(a.nbytes + 16)) == 0
        blocks.append(p)
        assert rt.hipMemcpy(C.c_void_p(p.value + shift), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
        return p.value + shift

    for shift in (0, 4, 8):
        dp = [[dev(a, shift if q == 3 else 0) for q, a in enumerate(col[k])] for k in range(2)]
        dcodes = dev(np.full((7, db.words), 0xabcdabcd, np.uint32))
        db.encode_images_device(dp[0], dp[1], dcodes)
        box.synchronize()
        back = np.zeros((7, db.words), np.uint32)
        assert rt.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(dcodes), C.c_size_t(back.nbytes), 2) == 0
        assert np.array_equal(back[:6], got) and (back[6] == 0xabcdabcd).all(), shift
    for p in blocks:
        rt.hipFree(p)
    db.close()


TORCH_CHILD = r"""
import sys
import numpy as np
import torch  # first, as bench.py does: the process then holds the HIP runtime torch brought
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import staticfusion_amd as sf
import test_gpu_keyframes as t
s = t.small_solver(sf.load(), 60, 80)
db, ferns, frames = t.batch_case(s)
host = db.encode_images([f[0] for f in frames], [f[1] for f in frames])
dev = [[torch.from_numpy(np.ascontiguousarray(f[k].T)).cuda() for f in frames] for k in range(2)]  # column-major, like sf_get_current
codes = torch.full((len(frames) + 1, db.words), 7, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
db.encode_images_device([x.data_ptr() for x in dev[0]], [x.data_ptr() for x in dev[1]], codes.data_ptr())
s.synchronize()
got = codes.cpu().numpy().view(np.uint32)
assert np.array_equal(got[:len(frames)], host) and (got[len(frames)] == 7).all()
print("torch tensors ok", int((host != 0).sum()))
"""


def test_encode_torch_tensors_in_a_fresh_process():
    """sfk_encode_images_device on torch tensors equals the host form (a fresh process with torch imported first, for the
    reason test_gpu_view.py gives)"""
    out = subprocess.run([sys.executable, "-c", TORCH_CHILD, ROOT], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0 and "torch tensors ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert int(out.stdout.split("torch tensors ok")[1].split()[0]) > 10


# ---- 3. the stream form after real frames ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walked(hip_auto):
    s, m, out = walk(hip_auto, 5, render_between=False)
    yield s, m, out
    m.close()
    s.close()


def test_stream_form_equals_image_form_and_numpy(walked):
    s, m, out = walked
    d, g = s.current(0)
    assert (d > 0).mean() > 0.5
    for cell, n_ferns in ((4, 128), (5, 65), (6, 9)):  # 60 x 80: four floats per lane, one, and two
        db = keyframes.KeyframeDb(s, cell, n_ferns=n_ferns, capacity=4)
        a = db.encode_streams([0, 0])
        b = db.encode_images([d], [g])
        want = kr.encode(d, g, db.ferns, cell)
        assert np.array_equal(a[0], want) and np.array_equal(a[1], want) and np.array_equal(b[0], want), cell
        assert 0 < len(set(kr.unpack(want, n_ferns).tolist())) and want.any()
        db.close()


# ---- 4. query --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257])
def test_query_equals_numpy(box, count):
    n_ferns = 65
    db = keyframes.KeyframeDb(box, 4, n_ferns=n_ferns, capacity=300)
    codes = random_codes(count, n_ferns, seed=count)
    tags = np.random.default_rng(count).integers(0, 3, count).astype(np.int32)
    if count >= 63:
        tags[tags == 2] = 1
        tags[7] = 2  # exactly one slot of tag 2: m larger than the matching slots
    db.set(codes, poses_of(count), tags, np.arange(count))
    assert db.info()["count"] == count
    queries = np.concatenate([random_codes(5, n_ferns, seed=count), random_codes(2, n_ferns, seed=1000 + count, pool=1, flips=0)])
    if count:
        queries[5] = codes[count // 2]  # a stored code itself: distance 0
    qtags = [-1, 0, 2, 9, -5, 1, -1]  # every slot, a tag, a rare tag, a tag no slot has
    ties = 0
    for m in (1, 3, 16):
        got = db.query_codes(queries, qtags, m)
        assert got.shape == (7, m)
        for q in range(7):
            want = kr.query(list(codes), list(tags), queries[q], qtags[q], m, n_ferns)
            assert as_list(got[q]) == want, (count, m, q, as_list(got[q]), want)
            ds = [d for s, d in want if s >= 0]
            ties += len(ds) - len(set(ds))
        assert as_list(got[3]) == [(-1, -1)] * m
        if count >= 63 and m > 1:
            assert as_list(got[2])[1:] == [(-1, -1)] * (m - 1) and got[2][0]["slot"] == 7
    assert count < 63 or ties > 10  # exact ties occur, and went to the lower slot
    if count:
        assert as_list(db.query_codes(queries[5:6], None, 1)[0])[0][1] == 0
    # the same code any number of times in one call
    rep = db.query_codes(np.repeat(queries[:1], 4, axis=0), [-1, -1, 0, -1], 3)
    assert rep[0].tobytes() == rep[1].tobytes() == rep[3].tobytes()
    db.close()


# ---- 5. add -----------------------------------------------------------------------------------------------------------------
def test_add_equals_numpy(box):
    n_ferns = 9
    db = keyframes.KeyframeDb(box, 4, n_ferns=n_ferns, capacity=20)
    ref_codes, ref_tags = [], []

    def step(codes, tags, min_distance, nearest):
        got = db.add_codes(codes, poses_of(len(tags), seed=len(ref_codes)), tags, np.arange(len(tags)) + 100 * len(ref_codes), min_distance, nearest=nearest)
        slots, near = kr.add(ref_codes, ref_tags, list(codes), list(tags), min_distance, n_ferns)
        if nearest:
            assert got[0].tolist() == slots and as_list(got[1]) == near, (got, slots, near)
        else:
            assert got.tolist() == slots, (got, slots)
        state = db.get()
        assert np.array_equal(state["codes"], np.array(ref_codes, np.uint32).reshape(-1, db.words)) and state["tags"].tolist() == ref_tags
        return slots

    a = random_codes(6, n_ferns, seed=1, pool=2, flips=2)
    assert step(a, [0, 1, 2, 3, 4, 5], 0, True) == [0, 1, 2, 3, 4, 5]  # an empty database: everything is novel
    assert step(a[:3], [0, 1, 2], 0, False) == [6, 7, 8]  # min_distance 0: always added, the same codes too
    # a value that splits a batch: distances to the slots of each tag lie on both sides of it
    b = a.copy()
    b[1] = kr.pack((kr.unpack(a[1], n_ferns) ^ np.uint32(1)))  # every nibble differs from tag 1's slots: distance 9
    b[3] = kr.pack(kr.unpack(a[3], n_ferns) ^ np.uint32([1, 1, 0, 0, 0, 0, 0, 0, 0]))  # distance 2 to tag 3's slot
    slots = step(b[[0, 1, 3, 5]], [0, 1, 3, 7], 3, True)
    assert slots == [-1, 9, -1, 10]  # near tag 0's slots; far from tag 1's; near tag 3's; tag 7 has no slot
    # n_ferns + 1: no distance reaches it, so only a tag without a slot is novel
    assert step(b[[1, 2]], [1, 8], n_ferns + 1, True) == [-1, 11]
    assert step(b[[1]], [1], n_ferns, False) == [-1]  # (tag 1 now holds b[1] itself)
    # stamps and poses went where the slots went
    state = db.get()
    assert state["stamps"].tolist() == [0, 1, 2, 3, 4, 5, 600, 601, 602, 901, 903, 1101]
    assert same_bits(state["poses"][9], poses_of(4, seed=9)[1]) and same_bits(state["poses"][11], poses_of(2, seed=11)[1])
    assert same_bits(db.get(9, 1)["poses"][0], state["poses"][9]) and db.get(3, 4)["stamps"].tolist() == [3, 4, 5, 600]
    # an overflow by one is SF_ERR_STATE and nothing changes: 12 slots of 20, nine novel entries
    before = db.get()
    nine = random_codes(9, n_ferns, seed=5)
    slots = np.full(9, -77, np.int32)
    near = np.full(9, -77, keyframes.MATCH_DTYPE)
    tg, st = np.arange(20, 29, dtype=np.int32), np.zeros(9, np.int32)
    ps = np.zeros((9, 16), np.float32)
    ip = C.POINTER(C.c_int32)
    code = db.b.add_codes(db.db, 9, nine.ctypes.data, ps.ctypes.data, tg.ctypes.data_as(ip), st.ctypes.data_as(ip), 0, slots.ctypes.data, near.ctypes.data)
    assert code == -3 and (slots == -77).all() and (near["slot"] == -77).all()
    after = db.get()
    assert db.info()["count"] == 12 and all(before[k].tobytes() == after[k].tobytes() for k in before)
    assert step(nine[:8], list(range(20, 28)), 0, True) == list(range(12, 20))  # eight fit exactly
    assert db.info()["count"] == db.info()["capacity"] == 20
    db.clear()
    assert db.info()["count"] == 0 and as_list(db.query_codes(nine[:1], None, 2)[0]) == [(-1, -1)] * 2
    db.close()


# ---- 6. retrieval, end to end ---------------------------------------------------------------------------------------------
def test_retrieval_of_twelve_views(hip_auto):
    c = kc.retrieval_case()
    s = small_solver(hip_auto, kc.RET_ROWS, kc.RET_COLS)
    db = keyframes.KeyframeDb(s, kc.RET_CELL, n_ferns=kc.RET_FERNS, seed=kc.RET_SEED, capacity=16)
    assert db.ferns.tobytes() == c["ferns"].tobytes()
    for k, (d, g) in enumerate(c["keyframes"]):
        s.set_current(0, d, g)
        slots, near = db.add_streams([0], c["poses"][k:k + 1], [0], [k], min_distance=kc.RET_MIN_DISTANCE, nearest=True)
        assert slots.tolist() == [k], k  # all twelve are novel (the CPU premise)
    assert np.array_equal(db.get()["codes"], np.array(c["key_codes"]))
    s.set_current(0, *c["queries"][5])
    slots, near = db.add_streams([0], c["poses"][5:6], [0], [99], min_distance=kc.RET_MIN_DISTANCE, nearest=True)
    assert slots.tolist() == [-1] and as_list(near) == [(5, kr.distance(c["query_codes"][5], c["key_codes"][5], kc.RET_FERNS))]
    for k, (d, g) in enumerate(c["queries"]):
        s.set_current(0, d, g)
        got = db.query_streams([0], None, 4)
        want = kr.query(c["key_codes"], [0] * 12, c["query_codes"][k], -1, 4, kc.RET_FERNS)
        assert as_list(got[0]) == want, k
        assert got[0]["slot"][0] == k and got[0]["distance"][1] - got[0]["distance"][0] >= 10, k  # own strictly first, with the margin
        cand = db.candidates(got)
        assert cand["slot"].tolist() == [w[0] for w in want] and cand["entry"].tolist() == [0] * 4
        assert same_bits(cand["pose"][0], c["poses"][k]) and same_bits(cand["pose"][3], c["poses"][want[3][0]])
    assert db.candidates(db.query_streams([0], [3], 2))["pose"].shape == (0, 4, 4)
    db.close()
    s.close()


# ---- 7. checkpoint and resume ---------------------------------------------------------------------------------------------
def test_get_then_set_into_a_second_database(box):
    n_ferns = 64
    a = keyframes.KeyframeDb(box, 4, n_ferns=n_ferns, capacity=100)
    codes = random_codes(70, n_ferns, seed=3)
    tags = (np.arange(70) % 4).astype(np.int32)
    for lo in range(0, 70, 4):  # four distinct tags per call
        a.add_codes(codes[lo:lo + 4], poses_of(70)[lo:lo + 4], tags[lo:lo + 4], np.arange(lo, min(lo + 4, 70)))
    saved = a.get()
    assert saved["codes"].shape == (70, 8) and np.array_equal(saved["codes"], codes) and same_bits(saved["poses"], poses_of(70))
    b = keyframes.KeyframeDb(box, 4, n_ferns=n_ferns, capacity=73)  # another capacity: another device layout
    b.set(saved["codes"], saved["poses"], saved["tags"], saved["stamps"])
    queries = random_codes(6, n_ferns, seed=4)
    for qt in (None, [0, 1, 2, 3, 0, 9]):
        assert a.query_codes(queries, qt, 16).tobytes() == b.query_codes(queries, qt, 16).tobytes()
    more = random_codes(3, n_ferns, seed=6, pool=9)
    ra = a.add_codes(more, poses_of(3), [0, 1, 2], [7, 8, 9], min_distance=2, nearest=True)
    rb = b.add_codes(more, poses_of(3), [0, 1, 2], [7, 8, 9], min_distance=2, nearest=True)
    assert ra[0].tolist() == rb[0].tolist() and ra[1].tobytes() == rb[1].tobytes()
    with pytest.raises(SfError):
        b.add_codes(more, poses_of(3), [0, 1, 2], [7, 8, 9])  # 73 slots are full now
    ga, gb = a.get(), b.get()
    for k in ga:
        assert ga[k].shape == gb[k].shape and ga[k].tobytes() == gb[k].tobytes(), (k, ga[k][-4:], gb[k][-4:])
    b.set(saved["codes"][:0], saved["poses"][:0], [], [])  # an empty content
    assert b.info()["count"] == 0
    a.close()
    b.close()


# ---- 8. a keyframe call leaves everything else alone -----------------------------------------------------------------------
def test_a_walk_with_keyframe_calls_in_between_equals_the_walk_without(hip_auto, walked, monkeypatch):
    plain = walked[2]
    calls, dbs = [], {}

    def keyframes_instead(maps, views, **kw):
        """stands in for view.render inside walk(): encode, add and query on the walking stream"""
        s = maps[0].solver
        if id(s) not in dbs:
            dbs[id(s)] = keyframes.KeyframeDb(s, 4, n_ferns=128, capacity=32)
        db = dbs[id(s)]
        code = db.encode_streams([0])
        slots = db.add_streams([0], view.view_pose(views[-1])[None], [0], [len(calls)], min_distance=1)
        got = db.query_streams([0, 0], [-1, 0], 3)
        d, g = s.current(0)
        assert np.array_equal(code[0], kr.encode(d, g, db.ferns, 4)) and np.array_equal(db.encode_images([d], [g]), code)
        assert got[0]["distance"][0] == 0 or slots[0] < 0  # a frame just added is found at distance 0
        calls.append(int(slots[0]))

    monkeypatch.setattr(tv.view, "render", keyframes_instead)
    s2, m2, with_calls = walk(hip_auto, 5, render_between=True)
    monkeypatch.undo()
    assert len(calls) == 10 and calls[0] == 0
    tv.same_walk(plain, with_calls)  # maps, index images, predictions, trajectories
    assert same_bits(walked[0].b_image(0), s2.b_image(0)) and same_bits(walked[0].current(0)[0], s2.current(0)[0])
    for db in dbs.values():
        db.close()
    m2.close()
    s2.close()


def test_keyframe_calls_leave_the_last_render_and_the_scores_alone(box):
    v = tv.large_view(min_confidence=0.0)
    small = random_surfels(300, v, seed=17, ordered=True)
    surf = np.concatenate([small[:150], tv.flat_surfel(0.01, -0.02, 0.45, 2.0, (9, 8, 7))[None], small[150:]])
    m = uploaded(box, surf)
    own = view.default_view(box, m)
    view.render([m, m], [v, own])
    counts = view.last_large_sprites(box, 2)
    assert counts[0] == 1
    d, g = kc.special_frame(60, 80, seed=1)
    box.set_current(0, np.where(np.isfinite(d), d, 1.0).astype(np.float32), np.where(np.isfinite(g), g, 0.5).astype(np.float32))
    p = score.Params(use_b=False)
    before = score.score_streams([m], [own], [0], p)
    db = keyframes.KeyframeDb(box, 5, n_ferns=65, capacity=8)
    code = db.encode_streams([0])
    db.add_streams([0], np.eye(4)[None], [3], [1])
    db.add_codes(code, np.eye(4)[None], [4], [2])
    assert as_list(db.query_streams([0], None, 3)[0]) == [(0, 0), (1, 0), (-1, -1)]
    assert view.last_large_sprites(box, 2) == counts  # still the render's n and the render's counts
    assert score.score_streams([m], [own], [0], p).tobytes() == before.tobytes()
    assert box.current(0)[0].tobytes() == np.where(np.isfinite(d), d, 1.0).astype(np.float32).tobytes()
    db.close()
    m.close()


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(hip_auto):
    s = small_solver(hip_auto, 32, 40)
    other = small_solver(hip_auto, 32, 40)
    b = keyframes._bind(s.api)
    ip = C.POINTER(C.c_int32)
    ferns = keyframes.default_ferns(9, 1, 80)
    fp = ferns.ctypes.data
    out = C.c_void_p()
    # -- create
    bad_fern = ferns.copy()
    bad_fern["cell"][8] = 80
    creates = [(None, 32, 40, 4, fp, 9, 8), (s.h, 32, 40, 4, None, 9, 8), (s.h, 0, 40, 4, fp, 9, 8), (s.h, 4097, 40, 4, fp, 9, 8), (s.h, 32, 0, 4, fp, 9, 8),
               (s.h, 32, 4097, 4, fp, 9, 8), (s.h, 32, 40, 0, fp, 9, 8), (s.h, 32, 40, 65, fp, 9, 8), (s.h, 32, 40, 41, fp, 9, 8),  # no cell at all
               (s.h, 128, 130, 2, fp, 9, 8),  # 64 x 65 = 4160 cells
               (s.h, 32, 40, 4, fp, 0, 8), (s.h, 32, 40, 4, fp, 4097, 8), (s.h, 32, 40, 4, bad_fern.ctypes.data, 9, 8), (s.h, 32, 40, 4, fp, 9, 0),
               (s.h, 32, 40, 4, fp, 9, 1048577)]
    for q, args in enumerate(creates):
        assert b.db_create(*args, C.byref(out)) == -1 and out.value is None, q
        assert s.api.last_error(), q
    assert b.db_create(s.h, 32, 40, 4, fp, 9, 8, None) == -1
    db = keyframes.KeyframeDb(s, 4, ferns=ferns, capacity=8)
    odd = keyframes.KeyframeDb(s, 4, n_ferns=9, capacity=8, rows=16, cols=40)  # not the handle's size: no stream form
    gone = keyframes.KeyframeDb(other, 4, ferns=ferns, capacity=8)
    codes = random_codes(3, 9, seed=1)
    db.add_codes(codes, poses_of(3), [0, 1, 2], [5, 6, 7])
    state = db.get()
    # prefilled outputs
    oc = np.full((3, 2), 0xabcdabcd, np.uint32)
    om = np.full((3, 16), -77, keyframes.MATCH_DTYPE)
    osl = np.full(3, -77, np.int32)
    st = (C.c_int32 * 3)(0, 0, 0)
    tg = (C.c_int32 * 3)(3, 4, 5)
    ps = np.zeros((3, 16), np.float32)
    img = np.zeros((40, 32), np.float32)
    imgs = (C.c_void_p * 3)(*[img.ctypes.data] * 3)
    half = (C.c_void_p * 3)(img.ctypes.data, None, img.ctypes.data)
    big = 65536
    many_st, many_tg = (C.c_int32 * big)(), (C.c_int32 * big)(*range(big))
    many_ptr = (C.c_void_p * big)(*[img.ctypes.data] * big)
    huge_c = np.full((big, 2), 0xabcdabcd, np.uint32)
    huge_m = np.full(big, -77, keyframes.MATCH_DTYPE)
    huge_s = np.full(big, -77, np.int32)
    huge_p = np.zeros((big, 16), np.float32)
    getter = s.api.get_current(s.h, 1, img.ctypes.data_as(C.POINTER(C.c_float)), None)  # the getters' own code for a stream out of range
    assert getter != 0
    c, m_, sl, pp = oc.ctypes.data, om.ctypes.data, osl.ctypes.data, ps.ctypes.data
    cases = [
        # encode
        (b.encode_streams, (None, 3, st, c), -1), (b.encode_streams, (db.db, 3, None, c), -1), (b.encode_streams, (db.db, 3, st, None), -1),
        (b.encode_streams, (db.db, -1, st, c), -1), (b.encode_streams, (db.db, big, many_st, huge_c.ctypes.data), -1),
        (b.encode_streams, (db.db, 3, (C.c_int32 * 3)(0, 1, 0), c), getter), (b.encode_streams, (db.db, 3, (C.c_int32 * 3)(0, 0, -1), c), getter),
        (b.encode_streams, (odd.db, 3, st, c), -1),
        (b.encode_images, (None, 3, imgs, imgs, c), -1), (b.encode_images, (db.db, 3, None, imgs, c), -1), (b.encode_images, (db.db, 3, imgs, None, c), -1),
        (b.encode_images, (db.db, 3, imgs, imgs, None), -1), (b.encode_images, (db.db, 3, half, imgs, c), -1), (b.encode_images, (db.db, 3, imgs, half, c), -1),
        (b.encode_images, (db.db, -1, imgs, imgs, c), -1), (b.encode_images, (db.db, big, many_ptr, many_ptr, huge_c.ctypes.data), -1),
        (b.encode_images_device, (None, 3, imgs, imgs, c), -1), (b.encode_images_device, (db.db, 3, None, imgs, c), -1),
        (b.encode_images_device, (db.db, 3, imgs, half, c), -1), (b.encode_images_device, (db.db, 3, imgs, imgs, None), -1),
        (b.encode_images_device, (db.db, -2, imgs, imgs, c), -1), (b.encode_images_device, (db.db, big, many_ptr, many_ptr, c), -1),
        # query
        (b.query_streams, (None, 3, st, tg, 4, m_), -1), (b.query_streams, (db.db, 3, None, tg, 4, m_), -1), (b.query_streams, (db.db, 3, st, None, 4, m_), -1),
        (b.query_streams, (db.db, 3, st, tg, 4, None), -1), (b.query_streams, (db.db, 3, st, tg, 0, m_), -1), (b.query_streams, (db.db, 3, st, tg, 17, m_), -1),
        (b.query_streams, (db.db, -1, st, tg, 4, m_), -1), (b.query_streams, (db.db, big, many_st, many_tg, 1, huge_m.ctypes.data), -1),
        (b.query_streams, (db.db, 3, (C.c_int32 * 3)(0, 0, 1), tg, 4, m_), getter), (b.query_streams, (odd.db, 3, st, tg, 4, m_), -1),
        (b.query_codes, (None, 3, codes.ctypes.data, tg, 4, m_), -1), (b.query_codes, (db.db, 3, None, tg, 4, m_), -1),
        (b.query_codes, (db.db, 3, codes.ctypes.data, None, 4, m_), -1), (b.query_codes, (db.db, 3, codes.ctypes.data, tg, 4, None), -1),
        (b.query_codes, (db.db, 3, codes.ctypes.data, tg, 0, m_), -1), (b.query_codes, (db.db, 3, codes.ctypes.data, tg, 17, m_), -1),
        (b.query_codes, (db.db, big, huge_c.ctypes.data, many_tg, 1, huge_m.ctypes.data), -1),
        # add
        (b.add_streams, (None, 3, st, pp, tg, st, 0, sl, m_), -1), (b.add_streams, (db.db, 3, None, pp, tg, st, 0, sl, m_), -1),
        (b.add_streams, (db.db, 3, st, None, tg, st, 0, sl, m_), -1), (b.add_streams, (db.db, 3, st, pp, None, st, 0, sl, m_), -1),
        (b.add_streams, (db.db, 3, st, pp, tg, None, 0, sl, m_), -1), (b.add_streams, (db.db, 3, st, pp, tg, st, 0, None, m_), -1),
        (b.add_streams, (db.db, 3, st, pp, tg, st, -1, sl, m_), -1), (b.add_streams, (db.db, 3, st, pp, (C.c_int32 * 3)(3, -1, 5), st, 0, sl, m_), -1),
        (b.add_streams, (db.db, 3, st, pp, (C.c_int32 * 3)(3, 4, 3), st, 0, sl, m_), -1), (b.add_streams, (db.db, -1, st, pp, tg, st, 0, sl, m_), -1),
        (b.add_streams, (db.db, big, many_st, huge_p.ctypes.data, many_tg, many_st, 0, huge_s.ctypes.data, None), -1),
        (b.add_streams, (db.db, 3, (C.c_int32 * 3)(1, 0, 0), pp, tg, st, 0, sl, m_), getter), (b.add_streams, (odd.db, 3, st, pp, tg, st, 0, sl, m_), -1),
        (b.add_codes, (None, 3, codes.ctypes.data, pp, tg, st, 0, sl, m_), -1), (b.add_codes, (db.db, 3, None, pp, tg, st, 0, sl, m_), -1),
        (b.add_codes, (db.db, 3, codes.ctypes.data, pp, tg, st, -5, sl, m_), -1), (b.add_codes, (db.db, 3, codes.ctypes.data, pp, (C.c_int32 * 3)(7, 7, 8), st, 0, sl, m_), -1),
        (b.add_codes, (db.db, 3, codes.ctypes.data, pp, (C.c_int32 * 3)(-2, 7, 8), st, 0, sl, m_), -1),
        (b.add_codes, (db.db, big, huge_c.ctypes.data, huge_p.ctypes.data, many_tg, many_st, 0, huge_s.ctypes.data, None), -1),
        # get / set / info
        (b.db_get, (None, 0, 1, c, None, None, None), -1), (b.db_get, (db.db, 0, 4, c, None, None, None), -1), (b.db_get, (db.db, 3, 1, c, None, None, None), -1),
        (b.db_get, (db.db, -1, 1, c, None, None, None), -1), (b.db_get, (db.db, 0, -1, c, None, None, None), -1),
        (b.db_set, (None, 1, codes.ctypes.data, pp, tg, st), -1), (b.db_set, (db.db, 9, codes.ctypes.data, pp, tg, st), -1), (b.db_set, (db.db, -1, codes.ctypes.data, pp, tg, st), -1),
        (b.db_set, (db.db, 2, None, pp, tg, st), -1), (b.db_set, (db.db, 2, codes.ctypes.data, None, tg, st), -1), (b.db_set, (db.db, 2, codes.ctypes.data, pp, None, st), -1),
        (b.db_set, (db.db, 2, codes.ctypes.data, pp, tg, None), -1), (b.db_set, (db.db, 2, codes.ctypes.data, pp, (C.c_int32 * 3)(0, -1, 0), st), -1),
        (b.db_info, (None, c), -1), (b.db_info, (db.db, None), -1), (b.db_clear, (None,), -1),
    ]
    for q, (fn, args, want) in enumerate(cases):
        args = tuple(a.ctypes.data_as(ip) if isinstance(a, np.ndarray) else a for a in args)
        assert fn(*args) == want, (q, fn.__name__)
        assert s.api.last_error(), q
    # n == 0 is fine and touches nothing
    assert b.encode_streams(db.db, 0, None, None) == 0 and b.encode_images(db.db, 0, None, None, None) == 0 and b.encode_images_device(db.db, 0, None, None, None) == 0
    assert b.query_streams(db.db, 0, None, None, 4, None) == 0 and b.query_codes(db.db, 0, None, None, 4, None) == 0
    assert b.add_streams(db.db, 0, None, None, None, None, 0, None, None) == 0 and b.add_codes(db.db, 0, None, None, None, None, 0, None, None) == 0
    assert b.db_get(db.db, 3, 0, None, None, None, None) == 0
    with pytest.raises(SfError):
        db.encode_images([np.zeros((40, 32), np.float32)], [np.zeros((40, 32), np.float32)])  # an image of another shape
    with pytest.raises(SfError):
        db.query_codes(np.zeros((1, 3), np.uint32))  # codes of another length
    with pytest.raises(SfError):
        db.add_codes(codes, poses_of(2), [0, 1, 2])
    # the handle goes first: its database is an empty shell that fails cleanly, and can still be destroyed
    other.close()
    for fn, args in ((b.encode_streams, (gone.db, 3, st, c)), (b.encode_images, (gone.db, 3, imgs, imgs, c)), (b.encode_images_device, (gone.db, 3, imgs, imgs, c)),
                     (b.query_streams, (gone.db, 3, st, tg, 4, m_)), (b.query_codes, (gone.db, 3, codes.ctypes.data, tg, 4, m_)),
                     (b.add_streams, (gone.db, 3, st, pp, tg, st, 0, sl, m_)), (b.add_codes, (gone.db, 3, codes.ctypes.data, pp, tg, st, 0, sl, m_)),
                     (b.db_get, (gone.db, 0, 0, None, None, None, None)), (b.db_set, (gone.db, 0, None, None, None, None)), (b.db_clear, (gone.db,)),
                     (b.db_info, (gone.db, c)), (b.encode_streams, (gone.db, 0, None, None))):
        assert fn(*args) == -3, fn.__name__  # SF_ERR_STATE
    gone.close()
    # nothing was written, and the database is what it was
    assert (oc == 0xabcdabcd).all() and (om["slot"] == -77).all() and (om["distance"] == -77).all() and (osl == -77).all()
    assert (huge_c == 0xabcdabcd).all() and (huge_m["slot"] == -77).all() and (huge_s == -77).all()
    after = db.get()
    assert db.info()["count"] == 3 and all(state[k].tobytes() == after[k].tobytes() for k in state)
    # and the same arguments, valid, still work
    assert b.query_codes(db.db, 3, codes.ctypes.data, (C.c_int32 * 3)(-1, -1, -1), 4, m_) == 0
    assert as_list(om[0][:4])[0] == (0, 0) and om["slot"][2][4] == -77
    assert b.add_streams(db.db, 3, st, pp, tg, st, 0, sl, None) == 0 and osl.tolist() == [3, 4, 5]
    for d in (db, odd):
        d.close()
    s.close()


# ---- 10. the other two libraries link the same object ------------------------------------------------------------------------
@pytest.mark.parametrize("lib", ["libsf_hip_precise.so", "libsf_hip_reforder.so"])
def test_the_precise_and_reference_order_libraries_do_the_same(lib):
    import staticfusion_amd as sf

    api = sf.Api(os.path.join(os.path.dirname(sf.LIB), lib), "sf_")
    s = small_solver(api, 48, 64)
    c = kc.retrieval_case()
    db = keyframes.KeyframeDb(s, kc.RET_CELL, n_ferns=kc.RET_FERNS, seed=kc.RET_SEED, capacity=16)
    got = db.encode_images([f[0] for f in c["keyframes"]], [f[1] for f in c["keyframes"]])
    assert np.array_equal(got, np.array(c["key_codes"]))
    for lo in range(12):
        assert db.add_codes(got[lo:lo + 1], c["poses"][lo:lo + 1], [0], [lo], min_distance=kc.RET_MIN_DISTANCE).tolist() == [lo]
    s.set_current(0, *c["queries"][7])
    assert as_list(db.query_streams([0], [0], 4)[0]) == kr.query(c["key_codes"], [0] * 12, c["query_codes"][7], 0, 4, kc.RET_FERNS)
    db.close()
    s.close()
