"""Stream migration (include/sf_migrate.h, staticfusion_amd/streams.py) on the GPU: a stream that was copied to another handle,
exported and imported again, or reset continues exactly -- bit for bit -- like the stream that stayed where it was. A copy has
no tolerance: every comparison is np.array_equal(..., equal_nan=True).

The continuation tests are what proves the list of what travels (include/sf_migrate.h): if a frame read anything else from its
predecessor, the moved stream would leave the reference's trajectory."""
import ctypes as C

import numpy as np
import pytest

from conftest import config2_params, driver_params, make_solver
from staticfusion_amd import SfError, SurfelMap, capi, streams
from staticfusion_amd.synth import make_sequence

pytestmark = pytest.mark.gpu

_frames = {}


def img(rows, cols, q, j):
    """frame j of synthetic sequence q at rows x cols: (depth, intensity)"""
    key = (rows, cols, q)
    if key not in _frames:
        _frames[key] = make_sequence(4000 + q, 20, sphere=True, out_rows=rows, out_cols=cols)["frames"]
    return _frames[key][j]


def sources(batch):
    """stream b replays sequence b % 3 from frame b // 3 on: no two streams of a handle see the same images"""
    return [(b % 3, b // 3) for b in range(batch)]


def start(s, src):
    for b, (q, off) in enumerate(src):
        s.set_current(b, *img(s.rows, s.cols, q, off))


def frame(s, k, src):
    """frame k of the handle: prediction := current, the next image of every stream's sequence, one process_frame"""
    s.current_to_prediction()
    for b, (q, off) in enumerate(src):
        s.set_current(b, *img(s.rows, s.cols, q, off + k + 1))
    s.process_frame(k)


def run(s, src, k0, k1):
    for k in range(k0, k1):
        frame(s, k, src)


def fed(api, batch, frames, rows=60, cols=80, params=None, src=None):
    s = make_solver(api, rows, cols, params if params is not None else driver_params(api), batch=batch)
    src = sources(batch) if src is None else src
    start(s, src)
    run(s, src, 0, frames)
    return s, src


def probe(s, b, im_count):
    """everything of one stream: the probe of tests/test_multi_frame.py, the twist, every level of both pyramids and of the labels, the blob"""
    out = [s.T(b), s.twist(b), s.twist_old(b), s.b(b), s.kmeans_centres(b), s.cluster_residuals(b), s.b_image(b), s.connectivity(b)]
    for L in range(s.levels):
        out.append(s.labels(L, b))
        for pset in (capi.SET_NEW, capi.SET_PRED):
            for ch in (capi.CH_DEPTH, capi.CH_INTENSITY):
                out.append(s.plane(pset, ch, L, b))
    st = s.stats(b)
    out.append(np.array([st.n_outer, st.n_irls, st.kmeans_iters, st.status, st.pixel_iters]))
    out.append(streams.export_stream(s, b, im_count))
    return out


def same(x, y):
    return len(x) == len(y) and all(np.array_equal(p, q, equal_nan=True) for p, q in zip(x, y))


def assert_same_stream(s, b, t, c, count_s, count_t=None):
    x, y = probe(s, b, count_s), probe(t, c, count_s if count_t is None else count_t)
    for q, (p, r) in enumerate(zip(x, y)):
        assert np.array_equal(p, r, equal_nan=True), (b, c, q)


# ---- 4: compaction ---------------------------------------------------------------------------------
def _compaction(hip, rows, cols, src_streams, dst_streams, dst_batch):
    A, src = fed(hip, 5, 7, rows, cols)
    R, _ = fed(hip, 5, 7, rows, cols)
    # the destination has a history of its own: slots in use are overwritten, the others go on undisturbed
    csrc = [(c % 3, 4 + c // 3) for c in range(dst_batch)]
    Cn, _ = fed(hip, dst_batch, 7, rows, cols, src=csrc)
    idle = [c for c in range(dst_batch) if c not in dst_streams]
    idle_before = [streams.export_stream(Cn, c, 7) for c in idle]
    streams.copy_streams(Cn, dst_streams, 7, A, src_streams, 7)
    for c, blob in zip(idle, idle_before):  # a head or tail that wrote past its segment would land in a neighbour
        assert np.array_equal(streams.export_stream(Cn, c, 7), blob), c
    for a, c in zip(src_streams, dst_streams):
        csrc[c] = src[a]
    for k in range(7, 12):
        for s, ss in ((R, src), (Cn, csrc), (A, src)):
            frame(s, k, ss)
        for a, c in zip(src_streams, dst_streams):
            assert np.array_equal(Cn.T(c), R.T(a)), (k, a, c)
    for a, c in zip(src_streams, dst_streams):
        assert_same_stream(R, a, Cn, c, 12)
    for b in range(5):  # the source was not disturbed
        assert_same_stream(R, b, A, b, 12)
    for s, ss in ((R, src), (Cn, csrc)):  # one more frame, launched alone
        frame(s, 12, ss)
    for a, c in zip(src_streams, dst_streams):
        assert np.array_equal(Cn.T(c), R.T(a)) and np.array_equal(streams.export_stream(Cn, c, 13), streams.export_stream(R, a, 13))


def test_compaction_continues_bit_identically(hip):
    _compaction(hip, 60, 80, [4, 1, 3], [0, 2, 1], 3)


# ---- 5: phase change -------------------------------------------------------------------------------
def test_a_stream_changes_ring_phase_when_it_moves(hip):
    A, asrc = fed(hip, 5, 7)
    R, _ = fed(hip, 5, 7)
    dsrc0 = [(b % 3, 3 + b // 3) for b in range(4)]
    D, _ = fed(hip, 4, 9, src=dsrc0)
    ctl, _ = fed(hip, 4, 9, src=dsrc0)
    streams.copy_streams(D, [3], 9, A, [2], 7)  # count 7, phase 2 -> count 9, phase 4
    q, off = asrc[2]
    dsrc = dsrc0[:3] + [(q, off - 2)]  # D's frame k is frame k - 2 of the moved stream's sequence
    for k in range(9, 14):
        frame(D, k, dsrc)
        frame(ctl, k, dsrc0)
        frame(R, k - 2, asrc)
        assert np.array_equal(D.T(3), R.T(2)), k
    assert_same_stream(R, 2, D, 3, 12, 14)  # (the blob exported with each side's own count)
    for b in range(3):  # the other streams of D never noticed
        assert_same_stream(ctl, b, D, b, 14)


# ---- 6: young streams ------------------------------------------------------------------------------
def test_young_streams_move_at_equal_counts_only(hip):
    A, src = fed(hip, 3, 3)
    R, _ = fed(hip, 3, 3)
    Y = make_solver(hip, 60, 80, driver_params(hip), batch=2)
    streams.copy_streams(Y, [1, 0], 3, A, [0, 2], 3)
    ysrc = [src[2], src[0]]
    for k in range(3, 7):  # across the switch-on of the residual stage at frame 5
        frame(Y, k, ysrc)
        frame(R, k, src)
        assert np.array_equal(Y.T(1), R.T(0)) and np.array_equal(Y.T(0), R.T(2)), k
    assert_same_stream(R, 0, Y, 1, 7)
    assert_same_stream(R, 2, Y, 0, 7)
    # a young stream does not enter a mature handle
    M, _ = fed(hip, 2, 9)
    before = [streams.export_stream(M, b, 9) for b in range(2)]
    with pytest.raises(SfError, match="failed with -1"):
        streams.copy_streams(M, [1], 9, A, [1], 3)
    with pytest.raises(SfError, match="failed with -1"):
        streams.copy_streams(A, [1], 3, M, [1], 9)
    assert all(np.array_equal(streams.export_stream(M, b, 9), before[b]) for b in range(2))


# ---- 7: checkpoint ---------------------------------------------------------------------------------
def test_checkpoint_and_resume_in_another_handle(hip):
    A, src = fed(hip, 4, 7)
    R, _ = fed(hip, 4, 7)
    blobs = [streams.export_stream(A, b, 7) for b in range(4)]
    assert all(len(x) == streams.blob_bytes(60, 80, A.levels, 0) for x in blobs)
    A.close()
    N = make_solver(hip, 60, 80, driver_params(hip), batch=4)
    perm = [2, 0, 3, 1]  # blob b -> slot perm[b]
    for b in range(4):
        streams.import_stream(N, perm[b], 7, blobs[b])
    nsrc = [None] * 4
    for b in range(4):
        nsrc[perm[b]] = src[b]
        assert np.array_equal(streams.export_stream(N, perm[b], 7), blobs[b])  # the round trip is the identity
    for k in range(7, 10):
        frame(N, k, nsrc)
        frame(R, k, src)
        for b in range(4):
            assert np.array_equal(N.T(perm[b]), R.T(b)), (k, b)
    for b in range(4):
        assert_same_stream(R, b, N, perm[b], 10)
    # what is not a blob of this handle is refused and changes nothing
    good = streams.export_stream(N, 1, 10)
    raw = streams._bind(N.api)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    bad_magic = good.copy()
    bad_magic[0] ^= 0xFF
    bad_geometry = good.copy()
    bad_geometry[8:12].view(np.int32)[0] = 62  # rows
    bad_version = good.copy()
    bad_version[4:8].view(np.uint32)[0] = 2
    bad_length = good.copy()
    bad_length[24:32].view(np.uint64)[0] -= 16
    for bad, nbytes in ((bad_magic, len(good)), (bad_geometry, len(good)), (bad_version, len(good)), (bad_length, len(good)), (good, len(good) - 16), (good, 32)):
        assert raw.import_stream(N.h, 1, 10, ptr(bad), nbytes) == -1 and N.api.last_error()
    small = np.zeros(len(good) - 16, np.uint8)
    assert raw.export_stream(N.h, 1, 10, ptr(small), small.nbytes) == -1 and N.api.last_error() and not small.any()
    assert np.array_equal(streams.export_stream(N, 1, 10), good)


def test_a_blob_crosses_between_builds(hip_auto):
    """exported from a throughput handle, imported into a latency handle: the getters agree right after the import (the builds
    are not bit-identical to each other in what they compute, so the continuation is not compared)"""
    tp, lat = hip_auto.with_variant("throughput"), hip_auto.with_variant("latency")
    A, _ = fed(tp, 2, 6)
    L = make_solver(lat, 60, 80, driver_params(lat), batch=3)
    assert A.variant()[0] == "throughput" and L.variant()[0] == "latency"
    streams.import_stream(L, 2, 6, streams.export_stream(A, 1, 6))
    assert_same_stream(A, 1, L, 2, 6)


# ---- 8: reset --------------------------------------------------------------------------------------
def test_reset_leaves_constructor_state(hip):
    S, src = fed(hip, 3, 6)
    fresh = make_solver(hip, 60, 80, driver_params(hip), batch=3)
    keep = [streams.export_stream(S, b, 6) for b in (0, 2)]
    streams.reset_streams(S, [1])
    assert np.array_equal(streams.export_stream(S, 1, 0), streams.export_stream(fresh, 1, 0))
    assert np.array_equal(streams.export_stream(S, 1, 0), streams.export_stream(fresh, 0, 0))  # (a blob does not depend on the slot)
    assert all(np.array_equal(streams.export_stream(S, b, 6), x) for b, x in zip((0, 2), keep))
    # a new sequence in the used slot: what a fresh handle computes for it
    new = [(1, 4)]
    F = make_solver(hip, 60, 80, driver_params(hip), batch=1)
    start(F, new)
    S.set_current(1, *img(60, 80, 1, 4))
    for k in range(6):
        # streams 0 and 2 of S go on with their own frame numbers in a service; here they simply solve again at stream 1's count
        S.current_to_prediction()
        S.set_current(1, *img(60, 80, 1, 4 + k + 1))
        S.process_frame(k)
        frame(F, k, new)
        assert np.array_equal(S.T(1), F.T(0)), k
    assert_same_stream(F, 0, S, 1, 6)


# ---- 9: refusals -----------------------------------------------------------------------------------
def test_refusals_launch_nothing(hip):
    A, src = fed(hip, 3, 2)
    R, _ = fed(hip, 3, 2)
    B = make_solver(hip, 60, 80, driver_params(hip), batch=2)
    other_size = make_solver(hip, 40, 42, driver_params(hip), batch=2)
    p2 = driver_params(hip)
    p2.ctf_levels = 2
    other_levels = make_solver(hip, 60, 80, p2, batch=2)
    before = [streams.export_stream(B, b, 2) for b in range(2)]
    cases = [
        lambda: streams.copy_streams(other_size, [0], 2, A, [0], 2),       # rows / cols
        lambda: streams.copy_streams(other_levels, [0], 2, A, [0], 2),     # pyramid levels
        lambda: streams.copy_streams(B, [2], 2, A, [0], 2),                # destination out of range
        lambda: streams.copy_streams(B, [0], 2, A, [3], 2),                # source out of range
        lambda: streams.copy_streams(B, [-1], 2, A, [0], 2),
        lambda: streams.copy_streams(B, [1, 1], 2, A, [0, 2], 2),          # twice among the destinations
        lambda: streams.copy_streams(A, [0, 1], 2, A, [1, 2], 2),          # one handle: a destination is also a source
        lambda: streams.copy_streams(B, [], 2, A, [], 2),                  # n < 1
        lambda: streams.copy_streams(B, [0], -1, A, [0], -1),
        lambda: streams.reset_streams(B, []),
        lambda: streams.reset_streams(B, [0, 0]),
        lambda: streams.reset_streams(B, [2]),
        lambda: streams.export_stream(B, 2, 2),
        lambda: streams.import_stream(B, 0, 2, streams.export_stream(other_size, 0, 2)),  # a blob of another geometry
    ]
    try:
        far = capi.Solver(hip, 60, 80, 2, driver_params(hip), device=1)
    except SfError:
        far = None  # a node with one GPU: the case cannot be set up
    if far is not None:
        cases.append(lambda: streams.copy_streams(far, [0], 2, A, [0], 2))  # another device: the blob is the route
    for q, call in enumerate(cases):
        with pytest.raises(SfError, match=r"failed with -1: \S"):
            call()
    # maps: orphaned, another resolution
    m = SurfelMap(other_size)
    with pytest.raises(SfError, match=r"failed with -1: \S"):
        streams.rebind_map(m, B)
    assert m.solver is other_size
    other_size.close()
    with pytest.raises(SfError, match=r"failed with -1: \S"):
        streams.rebind_map(m, B)
    m.close()
    assert all(np.array_equal(streams.export_stream(B, b, 2), before[b]) for b in range(2))
    # within one handle with disjoint lists it is a plain copy, and the handles solve on normally
    streams.copy_streams(A, [0], 2, A, [1], 2)
    assert np.array_equal(streams.export_stream(A, 0, 2), streams.export_stream(R, 1, 2))
    asrc = [src[1], src[1], src[2]]
    frame(A, 2, asrc)
    frame(R, 2, src)
    assert np.array_equal(A.T(0), R.T(1)) and np.array_equal(A.T(1), R.T(1)) and np.array_equal(A.T(2), R.T(2))
    start(B, sources(2))
    frame(B, 0, sources(2))
    assert np.isfinite(B.T(0)).all() and B.stats(0).n_irls > 0


# ---- 10: alignment ---------------------------------------------------------------------------------
def test_copy_between_differently_aligned_streams(hip):
    """40 x 42 with 3 levels: n_tot = 2200 bytes of labels per stream, 8 modulo 16 -- odd streams start 8 bytes off. Odd sources
    into even destinations and the other way round; the destination's streams in between are not touched"""
    _compaction(hip, 40, 42, [1, 3, 2, 4], [0, 2, 5, 3], 6)


def _full_frame(rows, cols, q, j):
    """a decoder-order full-resolution frame (2 x the solver's) made from a synthetic one: (H, W, 3) uint8, (H, W) uint16 mm"""
    d, i = img(rows, cols, q, j)
    full_d = np.repeat(np.repeat(np.clip(np.rint(d[::-1] * 1000), 0, 65535).astype(np.uint16), 2, 0), 2, 1)
    g = np.clip(np.rint(i[::-1] * 255), 0, 255).astype(np.uint8)
    rgb = np.stack([g, 255 - g, g // 2 + 7], -1)
    return np.repeat(np.repeat(rgb, 2, 0), 2, 1), full_d


def _inputs(s, b):
    return [s.input_image(w, b) for w in (capi.IN_DEPTH_MM, capi.IN_DEPTH_FILTERED_MM, capi.IN_DEPTH_METRIC, capi.IN_COLOR)]


def test_input_images_of_odd_and_even_streams(hip):
    """18 x 22, one level, no segmentation: n0 = 396, 4 modulo 8 -- the uint16 planes of odd streams are only 8-byte aligned and
    the colour planes (1188 bytes per stream) only 4-byte"""
    p = config2_params(hip, levels=1)
    A, Bh = (make_solver(hip, 18, 22, p, batch=4) for _ in range(2))
    for s, base in ((A, 0), (Bh, 8)):
        for b in range(4):
            s.load_frame(b, *_full_frame(18, 22, b % 3, base + b))
        s.filter_depth()
    a_before = [_inputs(A, b) for b in range(4)]
    b_before = [_inputs(Bh, b) for b in range(4)]
    streams.copy_streams(Bh, [2, 1], 0, A, [1, 2], 0)  # odd -> even, even -> odd
    assert same(_inputs(Bh, 2), a_before[1]) and same(_inputs(Bh, 1), a_before[2])
    assert same(_inputs(Bh, 0), b_before[0]) and same(_inputs(Bh, 3), b_before[3])  # the neighbours
    assert all(same(_inputs(A, b), a_before[b]) for b in range(4))
    assert len(streams.export_stream(A, 1, 0)) == streams.blob_bytes(18, 22, 1, 1)
    # into a handle that never used its input stage: it gets one
    N = make_solver(hip, 18, 22, p, batch=3)
    streams.copy_streams(N, [1], 0, A, [3], 0)
    assert same(_inputs(N, 1), a_before[3]) and not any(x.any() for x in _inputs(N, 0) + _inputs(N, 2))
    streams.import_stream(N, 2, 0, streams.export_stream(A, 0, 0))
    assert same(_inputs(N, 2), a_before[0]) and same(_inputs(N, 1), a_before[3])


# ---- 11: input stage and map follow the stream -----------------------------------------------------
def _loop_frame(s, k, feeds, maps):
    """the full loop for the streams named in `feeds` (stream -> sequence) and `maps` (stream -> SurfelMap)"""
    for b, q in feeds.items():
        s.load_frame(b, *_full_frame(60, 80, q, k))
    s.filter_depth()
    if k:
        s.process_frame(k)
    for b, m in maps.items():
        m.fuse_frame(b, None if k == 0 else s.T(b))
        m.predict(b)


def test_input_stage_and_map_follow_the_stream(hip):
    S, ctl = (make_solver(hip, 60, 80, driver_params(hip), batch=2) for _ in range(2))
    maps_s, maps_c = ({b: SurfelMap(s) for b in range(2)} for s in (S, ctl))
    feeds = {0: 0, 1: 1}
    for k in range(3):
        _loop_frame(S, k, feeds, maps_s)
        _loop_frame(ctl, k, feeds, maps_c)
    N = make_solver(hip, 60, 80, driver_params(hip), batch=1)
    streams.copy_streams(N, [0], 3, S, [1], 3)
    moved = maps_s.pop(1)
    streams.rebind_map(moved, N)
    assert moved.solver is N
    for k in range(3, 5):
        _loop_frame(N, k, {0: 1}, {0: moved})
        _loop_frame(S, k, feeds, maps_s)  # (stream 1 of the old handle goes on being solved; its map has left)
        _loop_frame(ctl, k, feeds, maps_c)

    def compare():
        for (m, s, b), (mc, c) in (((moved, N, 0), (maps_c[1], 1)), ((maps_s[0], S, 0), (maps_c[0], 0))):
            i, ic = m.info(), mc.info()
            assert i["count"] == ic["count"] > 0 and i["tick"] == ic["tick"] and i["stats"] == ic["stats"] and np.array_equal(i["pose"], ic["pose"])
            assert np.array_equal(m.download(), mc.download(), equal_nan=True)
            assert same(list(s.prediction(b)), list(ctl.prediction(c))) and same(_inputs(s, b), _inputs(ctl, c))
            assert np.array_equal(s.T(b), ctl.T(c))

    compare()
    S.close()  # the old handle goes: the rebound map is not its any more
    assert moved.download().shape[0] == maps_c[1].info()["count"]
    _loop_frame(N, 5, {0: 1}, {0: moved})
    assert moved.info()["tick"] == maps_c[1].info()["tick"] + 1


# ---- 12: ordering ----------------------------------------------------------------------------------
def test_a_copy_is_ordered_with_the_frames_of_both_handles(hip):
    A, R, R3 = (make_solver(hip, 60, 80, driver_params(hip), batch=3) for _ in range(3))
    for s in (A, R, R3):
        for b, (q, off) in enumerate(sources(3)):
            s.set_prediction(b, *img(60, 80, q, off))
            s.set_current(b, *img(60, 80, q, off + 1))
    X = make_solver(hip, 60, 80, driver_params(hip), batch=2)
    R3.process_frames(0, 3)
    R.process_frames(0, 6)
    # three frames, the copy, three more frames: queued back to back, the host never waits in between
    A.process_frames(0, 3)
    streams.copy_streams(X, [1, 0], 3, A, [0, 2], 3)
    A.process_frames(3, 3)
    assert np.array_equal(streams.export_stream(X, 1, 3), streams.export_stream(R3, 0, 3))
    assert np.array_equal(streams.export_stream(X, 0, 3), streams.export_stream(R3, 2, 3))
    for b in range(3):
        assert_same_stream(R, b, A, b, 6)
