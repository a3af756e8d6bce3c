"""Deformation graphs on the GPU (include/sf_deform.h): sfd_bind_maps and sfd_apply_maps against tests/deform_ref.py, bit for bit
(np.array_equal throughout). Maps of 0, 1, 255, 257 and 1025 surfels (a partly filled last wave, more than one workgroup) under
graphs of 1, 4, 5, 65, 257 and 1024 nodes (the node walk crosses the edge of the 256-node LDS tile), on the lattice scenes whose
queries tie at every rank, with duplicate nodes and NaN / inf nodes; a time window that leaves a third of a map unbound; three
maps in one call; identity and rigid transforms; the state of a map after a call; every refusal; the node sampling against the
thinning; a graph's call block reused small, large, small; a destroyed handle. References are computed once per case."""
import ctypes as C
import functools

import numpy as np
import pytest

import deform_cases as dc
import deform_ref as dr
from staticfusion_amd import SfError, SurfelMap, deform, join, view
from test_gpu_view import small_solver, uploaded, walk

pytestmark = pytest.mark.gpu

F = np.float32
COUNTS = (0, 1, 255, 257, 1025)
SIZES = (1, 4, 5, 65, 257, 1024)
EMPTY = np.zeros((0, 12), F)


@pytest.fixture(scope="module")
def box(hip_auto):
    s = small_solver(hip_auto, 60, 80)
    yield s
    s.close()


@functools.lru_cache(maxsize=None)
def scene(G, n=1025, window=np.inf):
    """(pos, times, M, surfels, the restatement's (m, idx, w), its deformed surfels) for a graph of G nodes and n surfels"""
    pos, times, M = dc.graph_scene(G, seed=G)
    q = dc.lattice_queries(min(G, 125))
    surf = dc.surfels(n, seed=G + 7, queries=q[::max(q.shape[0] // 600, 1)])
    m, idx, w = dr.bind(pos, times, window, surf[:, 0:3], surf[:, 6])
    deformed, _ = dr.deform(pos, times, M, window, surf)
    return pos, times, M, surf, (m, idx, w), deformed


def graph_of(s, pos, times, M=None, max_nodes=deform.MAX_NODES):
    g = deform.Graph(s, max_nodes)
    g.set(pos, times, M)
    return g


def state(m):
    i = m.info()
    return (i["count"], i["tick"], i["pose"].tobytes(), tuple(i["stats"]), m.download().tobytes())


# ---- 1. bind and apply against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("G", SIZES)
def test_bind_and_apply_equal_the_restatement(box, G):
    pos, times, M, surf, (m, idx, w), deformed = scene(G)
    g = graph_of(box, pos, times, M)
    assert g.info() == dict(max_nodes=1024, n_nodes=G)
    got = g.get()
    assert np.array_equal(got[0], pos, equal_nan=True) and np.array_equal(got[1], times, equal_nan=True) and np.array_equal(got[2], M)
    for n in COUNTS:  # a prefix of the surfels is the same case at another count: a surfel's binding does not depend on the others
        mp = uploaded(box, surf[:n])
        (gi, gw), = deform.bind_maps([mp], g)
        assert np.array_equal(gi, idx[:n]) and np.array_equal(gw, w[:n]), (G, n)
        assert mp.download().tobytes() == surf[:n].tobytes()  # a bind changes nothing
        c, = deform.apply_maps([mp], g)
        assert c == dr.counts(m[:n]), (G, n)
        assert np.array_equal(mp.download(), deformed[:n]), (G, n)
        mp.close()
    if G >= 5:
        assert int((m == 4).sum()) > 900
        assert int((w[:, 0] == F(0.25)).sum()) > 0  # the ties of a cell centre: every weight 0, so all four count the same
    g.close()


def test_a_time_window_that_leaves_a_third_unbound(box):
    pos, times = dc.lattice_nodes(65, times_mod=1)  # every node at time 0
    M = dc.random_affine(65, seed=3)
    surf = dc.surfels(1025, seed=4, queries=dc.lattice_queries(27))
    surf[:, 6] = np.where(np.arange(1025) % 3 == 2, F(100.0), F(np.arange(1025) % 2))  # init times 0, 1, 100, 0, 1, 100, ...
    window = 5.0
    want, m = dr.deform(pos, times, M, window, surf)
    assert dr.counts(m) == dict(n_surfels=1025, n_bound=684, n_unbound=341, n_short=0)
    g, mp = graph_of(box, pos, times, M), uploaded(box, surf)
    c, = deform.apply_maps([mp], g, deform.Params(time_window=window))
    got = mp.download()
    assert c == dr.counts(m) and np.array_equal(got, want)
    assert got[m == 0].tobytes() == surf[m == 0].tobytes() and not np.array_equal(got[m > 0, 0:3], surf[m > 0, 0:3])  # unbound: byte for byte
    assert got[:, 3:8].tobytes() == surf[:, 3:8].tobytes() and got[:, 11].tobytes() == surf[:, 11].tobytes()
    # a window that leaves some surfels fewer than four nodes: n_short
    times2 = (np.arange(65) % 33).astype(F)  # two nodes per time
    g.set(pos, times2, M)
    mp.upload(surf, np.eye(4, dtype=F), 7)
    want, m = dr.deform(pos, times2, M, 0.0, surf)
    c, = deform.apply_maps([mp], g, deform.Params(time_window=0.0))
    assert c == dr.counts(m) and c["n_short"] > 0 and c["n_unbound"] > 0 and np.array_equal(mp.download(), want)
    mp.close()
    g.close()


def test_three_maps_in_one_call_equal_the_single_calls(box):
    scenes = [scene(257), scene(65), scene(5)]
    counts = (1025, 257, 300)
    surfs = [scenes[0][3][:counts[0]], scenes[1][3][:counts[1]], scenes[2][3][:counts[2]]]
    shared = graph_of(box, *scenes[0][:3])
    own = [graph_of(box, *sc[:3]) for sc in scenes]
    for graphs, refs in ((shared, [scenes[0]] * 3), (own, scenes)):
        maps = [uploaded(box, a) for a in surfs]
        single = []
        for q, a in enumerate(surfs):  # the single calls, and the restatement
            one = uploaded(box, a)
            gq = graphs if isinstance(graphs, deform.Graph) else graphs[q]
            b1, = deform.bind_maps([one], gq)
            c1, = deform.apply_maps([one], gq)
            single.append((b1, c1, one.download()))
            one.close()
            pos, times, M = refs[q][:3]
            want, m = dr.deform(pos, times, M, np.inf, a)
            assert np.array_equal(single[q][2], want) and c1 == dr.counts(m)
        binds = deform.bind_maps(maps, graphs)
        cs = deform.apply_maps(maps, graphs)
        for q in range(3):
            assert np.array_equal(binds[q][0], single[q][0][0]) and np.array_equal(binds[q][1], single[q][0][1])
            assert cs[q] == single[q][1] and np.array_equal(maps[q].download(), single[q][2])
        for mp in maps:
            mp.close()
    for g in own + [shared]:
        g.close()


# ---- 2. identity and rigid --------------------------------------------------------------------------------------------------------
def test_identity_transforms(box):
    """Identity transforms give the restatement's result everywhere. Positions stay bit for bit where (p - g) + g is exact and
    the weights are exact and sum to exactly 1 -- surfels with dyadic coordinates on the lattice scene that are bound to one
    node, or to duplicates and ties whose weights are all 1/2 or 1/4; elsewhere w_i * x sums round."""
    pos, times = dc.duplicate_nodes(65)
    q = dc.lattice_queries(65)
    surf = dc.surfels(1025, seed=21, queries=q)
    want, m = dr.deform(pos, times, np.tile(np.eye(3, 4, dtype=F), (65, 1, 1)), np.inf, surf)
    _, _, w = dr.bind(pos, times, np.inf, surf[:, 0:3], surf[:, 6])
    g, mp = graph_of(box, pos, times), uploaded(box, surf)  # M = None: identities
    deform.apply_maps([mp], g)
    got = mp.download()
    assert np.array_equal(got, want)
    dyadic = np.all(surf[:, 0:3] * F(64) == np.round(surf[:, 0:3] * F(64)), axis=1)  # the lattice queries (multiples of 1/32)
    exact_w = np.all((w == 0) | (w == F(1)) | (w == F(0.5)) | (w == F(0.25)), axis=1) & (w.sum(axis=1) == 1)
    sel = dyadic & exact_w
    assert sel.sum() > 100 and got[sel, 0:3].tobytes() == surf[sel, 0:3].tobytes()
    assert np.abs(got[:, 0:3] - surf[:, 0:3]).max() < 1e-6  # (and nowhere more than rounding)
    g.set(pos, times, np.tile(np.eye(3, 4, dtype=F), (65, 1, 1)))  # the identities spelled out: the same bytes
    mp.upload(surf, np.eye(4, dtype=F), 7)
    deform.apply_maps([mp], g)
    assert mp.download().tobytes() == got.tobytes()
    mp.close()
    g.close()


def test_every_node_carrying_one_rigid_motion(box):
    pos, times = dc.lattice_nodes(65)
    R, t = dc.rotation([0.3, -1, 0.5], 0.4), np.array([0.2, -0.1, 0.05])
    M = dc.rigid_M(pos, R, t)
    surf = dc.surfels(1025, seed=22, queries=dc.lattice_queries(27))
    want, m = dr.deform(pos, times, M, np.inf, surf)
    g, mp = graph_of(box, pos, times, M), uploaded(box, surf)
    c, = deform.apply_maps([mp], g)
    got = mp.download()
    assert c["n_bound"] == 1025 and np.array_equal(got, want)
    moved = surf[:, 0:3].astype(np.float64) @ R.T + t  # (what the blend of one rigid motion is, to fp32 rounding)
    assert np.abs(got[:, 0:3] - moved).max() < 2e-5 and np.abs(got[:, 8:11] - surf[:, 8:11].astype(np.float64) @ R.T).max() < 2e-6
    mp.close()
    g.close()


# ---- 3. the map after a call --------------------------------------------------------------------------------------------------------
def test_the_state_of_a_map_after_a_call(hip_auto):
    s, fused, _ = walk(hip_auto, 2, render_between=False)  # predict -> load -> solve -> fuse: a map with an index image
    assert fused.index_map() is not None
    before = fused.info()
    surf = fused.download()
    assert before["count"] > 1000
    pos, times = deform.sample_nodes(fused, 0.5)
    assert 1 <= pos.shape[0] <= 1024
    M = dc.rigid_M(pos, dc.rotation([0, 1, 0], 0.01), np.array([0.01, 0.0, 0.0]))
    g = graph_of(s, pos, times, M)
    c, = deform.apply_maps([fused], g)
    after = fused.info()
    assert c["n_surfels"] == before["count"] == after["count"] and after["tick"] == before["tick"] and after["stats"] == before["stats"]
    assert after["pose"].tobytes() == before["pose"].tobytes()
    want, m = dr.deform(pos, times, M, np.inf, surf)
    assert np.array_equal(fused.download(), want) and c == dr.counts(m)
    with pytest.raises(SfError, match="failed with -3|index map"):  # sf_map_get_index_map: SF_ERR_STATE
        fused.index_map()
    images = view.render([fused], [view.default_view(s, fused)])  # a following render and a fuse work
    assert images is not None
    fused.predict(0)
    fused.fuse_frame(0, np.eye(4, dtype=F))
    assert fused.info()["tick"] == before["tick"] + 1 and fused.index_map() is not None
    fused.close()
    g.close()
    s.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(box, hip_auto):
    pos, times, M, surf, _, _ = scene(65)
    other = small_solver(hip_auto, 60, 80)
    a, b2 = uploaded(box, surf[:300]), uploaded(box, surf[300:700])
    foreign_map = uploaded(other, surf[:50])
    g, empty, foreign_graph = graph_of(box, pos, times, M), deform.Graph(box, 16), graph_of(other, pos, times, M)
    b = deform._bind(hip_auto)
    before = (state(a), state(b2), state(foreign_map))
    h = box.h
    one = lambda x: (C.c_void_p * 1)(x)  # noqa: E731
    p1 = (deform.SfdParams * 1)(deform.Params())
    out = (deform.SfdCounts * 2)()
    C.memset(out, 0xFB, C.sizeof(out))
    sentinel = bytes(out)
    idx, w = np.full((700, 4), -7, np.int32), np.full((700, 4), -7, F)
    ip, wp = idx.ctypes.data_as(C.POINTER(C.c_int32)), w.ctypes.data_as(C.POINTER(C.c_float))

    def both(code, n, maps, graphs, params):
        assert b.apply_maps(h, n, maps, graphs, params, out) == code and bytes(out) == sentinel
        assert b.bind_maps(h, n, maps, graphs, params, ip, wp) == code and np.all(idx == -7) and np.all(w == -7)
        assert (state(a), state(b2), state(foreign_map)) == before

    ma, ga = one(a.m.value), one(g.g.value)
    both(-1, -1, ma, ga, p1)                                   # n < 0
    both(-1, 65536, ma, ga, p1)                                # n > 65535
    both(-1, 1, None, ga, p1)                                  # null arguments
    both(-1, 1, ma, None, p1)
    both(-1, 1, ma, ga, None)
    assert b.apply_maps(h, 1, ma, ga, p1, None) == -1 and b.bind_maps(h, 1, ma, ga, p1, None, wp) == -1 and b.bind_maps(h, 1, ma, ga, p1, ip, None) == -1
    assert b.apply_maps(None, 1, ma, ga, p1, out) == -1
    both(-1, 1, one(None), ga, p1)                             # a null map, a null graph
    both(-1, 1, ma, one(None), p1)
    both(-1, 1, one(foreign_map.m.value), ga, p1)              # a map of another handle
    both(-1, 1, ma, one(foreign_graph.g.value), p1)            # a graph of another handle
    both(-3, 1, ma, one(empty.g.value), p1)                    # a graph with G == 0: SF_ERR_STATE
    two_m, two_g = (C.c_void_p * 2)(a.m.value, a.m.value), (C.c_void_p * 2)(g.g.value, g.g.value)
    p2 = (deform.SfdParams * 2)(deform.Params(), deform.Params())
    both(-1, 2, two_m, two_g, p2)                              # the same map twice
    for bad in (deform.Params(time_window=float("nan")), deform.Params(time_window=-1.0), deform.Params(time_window=float("-inf"))):
        both(-1, 1, ma, ga, (deform.SfdParams * 1)(bad))
        both(-1, 2, (C.c_void_p * 2)(a.m.value, b2.m.value), two_g, (deform.SfdParams * 2)(deform.Params(), bad))  # ... in a later entry
    assert b.apply_maps(h, 0, None, None, None, None) == 0 and (state(a), state(b2)) == before[:2]  # n == 0: SF_OK
    # the graph object
    bad_M = M.copy()
    bad_M[3, 1, 1] = np.nan
    with pytest.raises(SfError, match="failed with -1"):
        g.set(pos, times, bad_M)
    with pytest.raises(SfError, match="failed with -1"):
        empty.set(pos, times, M)  # 65 nodes into a graph of 16
    with pytest.raises(SfError, match="failed with -1"):
        deform.Graph(box, 0)
    with pytest.raises(SfError, match="failed with -1"):
        deform.Graph(box, 1025)
    assert g.info()["n_nodes"] == 65 and empty.info()["n_nodes"] == 0
    # the calls still work, and a graph may serve two maps
    cs = deform.apply_maps([a, b2], g)
    assert [c["n_surfels"] for c in cs] == [300, 400]
    # more nodes than there is room for: SF_ERR_STATE with the count
    k = C.c_int32(-1)
    npos, ntimes = np.full((4, 3), -7, F), np.full(4, -7, F)
    code = b.sample_nodes(a.m, C.c_float(0.05), 4, npos.ctypes.data_as(C.POINTER(C.c_float)), ntimes.ctypes.data_as(C.POINTER(C.c_float)), C.byref(k))
    assert code == -3 and k.value == join.thin_extract(a, join.Params(cell=0.05))[1]["n_out"] > 4 and np.all(npos == -7) and np.all(ntimes == -7)
    for x in (a, b2, foreign_map, g, empty, foreign_graph):
        x.close()
    other.close()


def test_a_graph_whose_handle_was_destroyed_answers_state(hip_auto):
    pos, times, M, surf, _, _ = scene(5)
    s = small_solver(hip_auto, 60, 80)
    g, mp = graph_of(s, pos, times, M), uploaded(s, surf[:100])
    assert deform.apply_maps([mp], g)[0]["n_bound"] == 100
    b = deform._bind(hip_auto)
    gone = C.c_void_p(s.h.value)
    s.close()
    info = deform.SfdInfo()
    fp = pos.ctypes.data_as(C.POINTER(C.c_float))
    assert b.graph_info(g.g, C.byref(info)) == -3 and b.graph_set(g.g, 1, fp, fp, None) == -3 and b.graph_get(g.g, None, None, None) == -3
    out = (deform.SfdCounts * 1)()
    args = (gone, 1, (C.c_void_p * 1)(mp.m.value), (C.c_void_p * 1)(g.g.value), (deform.SfdParams * 1)(deform.Params()))
    assert b.apply_maps(*args, out) == -3
    k = C.c_int32(0)
    assert b.sample_nodes(mp.m, C.c_float(0.1), 8, fp, fp, C.byref(k)) == -3
    out_g = C.c_void_p()
    assert b.graph_create(gone, 8, C.byref(out_g)) == -3
    g.close()  # (frees the shell)
    mp.close()


# ---- 5. node sampling; the call block -------------------------------------------------------------------------------------------------
def test_sample_nodes_equals_the_thinning_at_the_same_cell(box):
    surf = dc.surfels(1025, seed=31)
    surf[5, 0] = np.inf  # outside the thinning's grid: kept by it, and so a node candidate too (never eligible)
    mp = uploaded(box, surf)
    for cell in (0.5, 0.3, 1.7):
        kept, counts = join.thin_extract(mp, join.Params(cell=cell))
        pos, times = deform.sample_nodes(mp, cell)
        assert pos.shape[0] == counts["n_out"] > 1 and np.array_equal(pos, kept[:, 0:3]) and np.array_equal(times, kept[:, 6])
    assert mp.download().tobytes() == surf.tobytes()
    with pytest.raises(SfError, match="failed with -1"):
        deform.sample_nodes(mp, 0.0)
    with pytest.raises(SfError, match="failed with -1"):
        deform.sample_nodes(mp, 0.5, max_nodes=1025)
    mp.close()


def test_a_graphs_block_reused_small_large_small(box, hip_auto):
    """as tests/test_gpu_call_blocks.py: a small call, one large enough to grow the block and move every offset, the small one again"""
    def call(s, g, size):
        G, n_maps, n = dict(small=(5, 1, 257), large=(1024, 3, 1025))[size]
        pos, times, M, surf, _, _ = scene(G)
        g.set(pos, times, M)
        maps = [uploaded(s, surf[q:n]) for q in range(n_maps)]
        binds = deform.bind_maps(maps, g)
        counts = deform.apply_maps(maps, g)
        out = repr(counts).encode() + b"".join(i.tobytes() + w.tobytes() for i, w in binds) + b"".join(m.download().tobytes() for m in maps)
        for m in maps:
            m.close()
        return out

    fresh = small_solver(hip_auto, 60, 80)
    used_g, fresh_g = deform.Graph(box), deform.Graph(fresh)
    first = call(box, used_g, "small")
    large = call(box, used_g, "large")
    third = call(box, used_g, "small")
    assert len(large) > 3 * len(first) and third == first
    assert call(fresh, fresh_g, "small") == first and call(fresh, fresh_g, "large") == large
    used_g.close()
    fresh_g.close()
    fresh.close()
