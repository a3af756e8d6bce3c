"""The host side's resources on the GPU (staticfusion_amd/csrc/sf_resources.h): a block that grows is replaced and the outgrown
one released, and nothing computed may depend on whether a handle's blocks grew call by call or were large from the start;
a handle goes with work outstanding and takes everything it owns along. Handles of 30 x 40 (tests/golden/fusion_40x30.npz: two
levels, even sides); every comparison is np.array_equal."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, driver_params, hip_runtime, make_solver
from staticfusion_amd import SfError, SurfelMap, closure, deform, keyframes, map_window, score, streams, tracks, view
from staticfusion_amd.synth import make_sequence

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "fusion_40x30.npz"))


def small(api, g, batch):
    p = driver_params(api)
    p.ctf_levels = 2
    return make_solver(api, int(g["rows"]), int(g["cols"]), p, batch=batch)


def load(s, g, k):
    """frame k of the fixture into every stream, filtered, with the fixture's segmentation"""
    for b in range(s.batch_size):
        s.load_frame(b, g["color_full_%d" % k], g["depth_full_%d" % k], int(g["res_factor"]))
    s.filter_depth()
    for b in range(s.batch_size):
        s.set_segm_state(b, g["labels"], g["b_segm"], np.ones(24, np.float32))
    s.build_segm_image()


def batched_calls(s, g, maps, k):
    """one call of each batched kind on maps[q] and stream q; everything they give back"""
    n = len(maps)
    st = list(range(n))
    SurfelMap.fuse_frames(s, st, maps, [g["increments"][k]] * n)
    out = [m.download() for m in maps] + [m.info()["stats"] for m in maps]
    SurfelMap.predict_frames(s, st, maps)
    for b in st:
        out += list(s.prediction(b)) + [s.prediction_dense_stream(b)]
    # keep the more confident half (the threshold comes from the map itself: both handles hold the same map, or the test fails above)
    fl = [map_window.Filter(min_confidence=float(np.median(m.download()[:, 3]))) for m in maps]
    kept = map_window.cull(maps, fl)
    assert all(0 < c <= m.info()["stats"][3] for c, m in zip(kept, maps))
    out += [np.array(kept)] + [m.download() for m in maps]
    views = [view.default_view(s, m) for m in maps]
    for im in view.render(maps, views):
        out += [im["depth"], im["rgb"], im["index"]]
    out.append(score.score_streams(maps, views, st))
    return out


def three_frames(api, g, grown_first):
    s = small(api, g, 4)
    if grown_first:  # one throw-away call of each kind with n = 4 on maps of its own: every block is as large as it will get
        load(s, g, 0)
        own = [SurfelMap(s) for _ in range(4)]
        batched_calls(s, g, own, 0)
        for m in own:
            m.close()
    maps = [SurfelMap(s) for _ in range(4)]
    out = []
    for k, n in enumerate((1, 2, 4)):  # the batched calls take 1, 2, 4 entries: their blocks grow twice
        load(s, g, k)
        out += batched_calls(s, g, maps[:n], k)
    for m in maps:
        m.close()
    s.close()
    return out


def test_growth_changes_no_result(hip_auto, golden):
    a = three_frames(hip_auto, golden, False)
    b = three_frames(hip_auto, golden, True)
    assert len(a) == len(b) and len(a) > 60
    for q, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y, equal_nan=True) if isinstance(x, np.ndarray) and x.dtype.kind == "f" else np.array_equal(x, y), q
    assert any(isinstance(x, np.ndarray) and x.dtype.kind == "f" and x.size > 100 and np.isfinite(x).any() and (x != 0).any() for x in a)


class Dev:  # a device copy of a host array (plain hipMalloc: the tests use no torch)
    def __init__(self, h):
        self.rt = hip_runtime()
        self.ptr = C.c_void_p()
        assert self.rt.hipMalloc(C.byref(self.ptr), C.c_size_t(h.nbytes)) == 0
        assert self.rt.hipMemcpy(self.ptr, h.ctypes.data_as(C.c_void_p), C.c_size_t(h.nbytes), 1) == 0

    def free(self):
        assert self.rt.hipFree(self.ptr) == 0


def test_multi_frame_launches_of_growing_length(hip_auto, golden, pair):
    """2 then 5 frames per launch (the index, staging and trajectory blocks grow) against a handle whose blocks held 5 frames
    from the start and whose streams were put back to constructor state (sfm_reset_streams)"""
    F = 8
    pr = pair(seed=31, rows=30, cols=40, sphere=True)
    seq = make_sequence(2100, F, sphere=True, out_rows=30, out_cols=40)
    col = lambda a: np.ascontiguousarray(np.asarray(a, np.float32).T).ravel()
    pd, pi = Dev(np.stack([col(f[0]) for f in seq["frames"]])), Dev(np.stack([col(f[1]) for f in seq["frames"]]))
    index = np.stack([(np.arange(2) * 3 + k) % F for k in range(7)]).astype(np.int32)

    def run(s):
        for b in range(2):
            s.set_current(b, *pr["new"])
            s.set_prediction(b, *pr["old"])
        out = [s.process_frames(0, 2, trajectory=True), s.process_frames(2, 5, trajectory=True)]
        out.append(s.process_sequence_frames_device(pd.ptr.value, pi.ptr.value, index[:2], F, 7, trajectory=True))
        out.append(s.process_sequence_frames_device(pd.ptr.value, pi.ptr.value, index[2:], F, 9, trajectory=True))
        return out + [s.T(0), s.T(1), s.b_image(1), s.labels(0, 0)]

    grown = small(hip_auto, golden, 2)
    a = run(grown)
    large = small(hip_auto, golden, 2)
    for b in range(2):
        large.set_current(b, *pr["old"])
        large.set_prediction(b, *pr["new"])
    large.process_frames(0, 5, trajectory=True)
    large.process_sequence_frames_device(pd.ptr.value, pi.ptr.value, index[:5], F, 5, trajectory=True)
    streams.reset_streams(large, [0, 1])
    b = run(large)
    assert [x.shape for x in a[:4]] == [(2, 2, 4, 4), (5, 2, 4, 4), (2, 2, 4, 4), (5, 2, 4, 4)]
    for q, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), q
    assert all(np.isfinite(x).all() for x in a[:6]) and not np.array_equal(a[1][4, 0], np.eye(4))  # frames were solved
    grown.close()
    large.close()
    pd.free()
    pi.free()


def test_release_with_work_outstanding(hip_auto, golden, pair):
    """sf_destroy with two live maps, an upload that was never committed and a migration ring that has gone round: the maps are
    orphans that close without an error, and a fresh handle of the same size works"""
    g = golden
    s = small(hip_auto, g, 2)
    load(s, g, 0)
    maps = [SurfelMap(s) for _ in range(2)]
    SurfelMap.fuse_frames(s, [0, 1], maps, None)
    assert all(m.info()["count"] > 0 for m in maps)
    for _ in range(6):  # four slots: the ring has been round once
        streams.reset_streams(s, [1])
    n0 = s.rows * s.cols
    host = np.zeros((2, 2, n0), np.float32) + 1.5
    fp = C.POINTER(C.c_float)
    hip_auto.check(hip_auto.upload_current_async(s.h, host[0].ctypes.data_as(fp), host[1].ctypes.data_as(fp)))
    s.close()  # no sf_commit_upload
    for m in maps:
        with pytest.raises(SfError):
            m.download()  # SF_ERR_STATE: the handle this map was created from has been destroyed
        m.close()
        assert not m.m
    fresh = small(hip_auto, g, 2)
    load(fresh, g, 0)
    m = SurfelMap(fresh)
    m.fuse_frame(0, None)
    pr = pair(seed=31, rows=30, cols=40, sphere=True)
    for b in range(2):
        fresh.set_current(b, *pr["new"])
        fresh.set_prediction(b, *pr["old"])
    fresh.process_frame(0)
    assert m.info()["count"] > 0 and np.isfinite(fresh.T(0)).all() and not np.array_equal(fresh.T(0), np.eye(4))
    m.close()
    fresh.close()


# ---- the five kinds of part of a handle (csrc/sf_parts.h): a map, a keyframe database, a tracker, a deformation graph, a closure builder
SENT = -77


def five_parts(s):
    return SurfelMap(s), keyframes.KeyframeDb(s, 5, n_ferns=32), tracks.Tracker(s, 1, 4), deform.Graph(s, 4), closure.Builder(s)


def camera(s):
    return tracks.Camera(np.eye(4), 0.5 * (s.cols - 1), 0.5 * (s.rows - 1), 0.5 * s.cols, 0.5 * s.cols)


def use_each_once(s, g, parts):
    """every part used once, so that it holds device memory and a grown call block; everything the five calls return"""
    m, db, t, gr, bld = parts
    load(s, g, 0)
    m.fuse_frame(0, None)  # a fuse into the map
    out = [m.download(), np.array(m.info()["stats"])]
    out += [db.add_streams([0], [np.eye(4)], [0]), db.get()["codes"]]  # one keyframe added to the database
    summ, per = t.update_streams([0], [0], [camera(s)])  # one tracker update
    out += [summ, per[0]]
    nodes = out[0][:: max(out[0].shape[0] // 4, 1)][:4]
    gr.set(nodes[:, 0:3], nodes[:, 6])  # a graph of 4 nodes set ...
    idx, w = deform.bind_maps([m], gr)[0]  # ... and bound
    out += [idx, w]
    v = view.default_view(s, m)
    recs, counts = bld.build([m], [m], [v], [v], closure.Params(stride=4))  # one closure build at stride 4
    out += [recs, np.array([counts[0][k] for k in sorted(counts[0])])]
    assert out[0].shape[0] > 4 and gr.info()["n_nodes"] == 4 and db.info()["count"] == 1 and counts[0]["n_samples"] > 0 and idx.shape == (out[0].shape[0], 4)
    return out


def refused_with_sentinels(s, parts, v):
    """after sf_destroy of the handle: one call per part answers SF_ERR_STATE (-3) and writes nothing (v: a view made before)"""
    m, db, t, gr, bld = parts
    fp = C.POINTER(C.c_float)
    buf = np.full((4, 12), SENT, np.float32)
    assert s.api.map_download(m.m, buf.ctypes.data_as(fp), 4) == -3 and (buf == SENT).all()
    one, pose, slots = (C.c_int32 * 1)(0), np.eye(4, dtype=np.float32).ravel(), np.full(1, SENT, np.int32)
    assert db.b.add_streams(db.db, 1, one, pose.ctypes.data, one, one, 0, slots.ctypes.data, None) == -3 and (slots == SENT).all()
    summ, trk = np.full(1, SENT, tracks.SUMMARY_DTYPE), np.full(4, SENT, tracks.TRACK_DTYPE)
    code = t.b.update_streams(t.t, 1, one, one, (tracks.SftCamera * 1)(camera(s)), (tracks.SfrParams * 1)(tracks.RegionParams()), (tracks.SftParams * 1)(tracks.Params()),
                              summ.ctypes.data, trk.ctypes.data, None)
    assert code == -3 and (summ == np.full(1, SENT, tracks.SUMMARY_DTYPE)).all() and (trk == np.full(4, SENT, tracks.TRACK_DTYPE)).all()
    pos, times, M = np.full((4, 3), SENT, np.float32), np.full(4, SENT, np.float32), np.full((4, 12), SENT, np.float32)
    assert gr.b.graph_get(gr.g, pos.ctypes.data_as(fp), times.ctypes.data_as(fp), M.ctypes.data_as(fp)) == -3
    assert (pos == SENT).all() and (times == SENT).all() and (M == SENT).all()
    counts = (closure.SfcCounts * 1)()
    C.memset(counts, 0xAB, C.sizeof(counts))
    before = bytes(counts)
    recs = np.full(2 * closure.RECORD.itemsize // 4, SENT, np.int32)  # room for two records
    maps, views = (C.c_void_p * 1)(m.m.value), (closure.SfvView * 1)(v)
    assert bld.b.build(bld.c, 1, maps, maps, views, views, (closure.SfcParams * 1)(closure.Params(stride=4)), recs.ctypes.data, 2, counts) == -3
    assert bytes(counts) == before and (recs == SENT).all()


def test_the_five_kinds_of_part_outlive_their_handle_or_go_before_it(hip_auto, golden):
    """One 30 x 40 handle with two streams and one part of every kind, each used once. The handle goes first: every part is a
    shell that refuses with SF_ERR_STATE, writes nothing and closes, twice. The parts go first, in the order they were made:
    nothing errors. And a third handle gives what the first one gave."""
    g = golden
    s = small(hip_auto, g, 2)
    parts = five_parts(s)
    first = use_each_once(s, g, parts)
    v = view.default_view(s, parts[0])
    s.close()
    refused_with_sentinels(s, parts, v)
    for p in parts:
        p.close()
        p.close()
    assert not parts[0].m and not parts[1].db and not parts[2].t and not parts[3].g and not parts[4].c
    s = small(hip_auto, g, 2)
    parts = five_parts(s)
    use_each_once(s, g, parts)
    for p in parts:
        p.close()
        p.close()
    s.close()
    s = small(hip_auto, g, 2)
    parts = five_parts(s)
    third = use_each_once(s, g, parts)
    assert len(first) == len(third) == 10
    for q, (x, y) in enumerate(zip(first, third)):
        assert x.dtype == y.dtype and (np.array_equal(x, y, equal_nan=True) if x.dtype.kind == "f" else np.array_equal(x, y)), q
    for p in parts:
        p.close()
    s.close()
