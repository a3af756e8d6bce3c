"""Closure constraints on the GPU (include/sf_closure.h): sfc_build against tests/closure_ref.py, np.array_equal on the records and
integer equality on the counts throughout. Views of 1 x 1, 1 x 65, 257 x 1, 16 x 16, 53 x 37 (negative fy) and 64 x 48 at strides
1, 2, 3, 7, 64 and 4096 -- 0, 1, 63, 64, 65, 256, 257, 336 and 3072 samples: a partial wave, a whole workgroup, two, twelve, and
workgroups that emit nothing between two that do --, maps of 0, 1, 255, 257 and 1025 surfels, map_old the same map and another
one, an age that selects a third, scenes in which every sample emits two records and none does, every pins mode, gates and a time
gap that cut about half, NaN and inf init times, a sum_dz beyond 32 bits, a batch of five entries against the five single calls,
the capacity refusal behind guard words and the size query, the state a build leaves alone, the builder's block reused small,
large, small, every refusal, a destroyed handle, and the doubled wall through solve and apply. References are computed once
per case (closure_cases.reference)."""
import ctypes as C

import numpy as np
import pytest

import closure_cases as cc
import closure_ref as cr
from staticfusion_amd import SfError, closure, deform, map_window, view
from test_closure_reference_cpu import far_planes
from test_gpu_view import small_solver, uploaded, walk

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def box(hip_auto):
    s = small_solver(hip_auto, 60, 80)
    yield s
    s.close()


@pytest.fixture(scope="module")
def builder(box):
    b = closure.Builder(box)
    yield b
    b.close()


def run(s, b, entries):
    """the entries of closure_ref.build through sfc_build: (records, counts); `same` entries share one map"""
    maps, new, old = [], [], []
    for surf_new, tick_new, surf_old, tick_old, vf, vt, p in entries:
        mn = uploaded(s, surf_new, tick=tick_new)
        mo = mn if surf_old is surf_new else uploaded(s, surf_old, tick=tick_old)
        maps += [mn] + ([] if mo is mn else [mo])
        new.append(mn)
        old.append(mo)
    try:
        return b.build(new, old, [e[4] for e in entries], [e[5] for e in entries], [cc.as_product(e[6]) for e in entries])
    finally:
        for m in maps:
            m.close()


def assert_equal(got, want, where):
    (recs, counts), (want_recs, want_counts) = got, want
    assert counts == want_counts, (where, counts, want_counts)
    assert recs.dtype == closure.RECORD and cr.same_records(recs, want_recs), where


# ---- 1. against the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [k for k in cc.CASES if k != "batch"])
def test_build_equals_the_restatement(box, builder, key):
    assert_equal(run(box, builder, cc.CASES[key]()), cc.reference(key), key)


def test_a_sum_dz_that_needs_more_than_32_bits(box, builder):
    new, old, v = far_planes()
    p = cc.params(stride=1, pins=0, gate_abs=np.inf, min_time_gap=100.0)
    recs, (c,) = run(box, builder, [(new, 1, old, 1, v, v, p)])
    assert c == cr.build_entry(new, 1, old, 1, v, v, p)[1] and c["sum_dz"] == 1 << 37 and recs.shape == (0,)


def test_a_batch_of_five_equals_the_five_single_calls(box, builder):
    entries = cc.CASES["batch"]()
    got = run(box, builder, entries)
    assert_equal(got, cc.reference("batch"), "batch")
    first = 0
    for q, e in enumerate(entries):
        recs, (c,) = run(box, builder, [e])
        k = c["n_links"] + c["n_pins"]
        assert got[1][q]["first"] == first and dict(c, first=first) == got[1][q]
        assert cr.same_records(got[0][first:first + k], recs), q
        first += k
    assert first == got[0].shape[0] > 1000 and len({c["n_samples"] for c in got[1]}) == 4  # entries of different sizes


# ---- 2. the capacity ------------------------------------------------------------------------------------------------------------------
def test_capacity_refusal_and_size_query(box, builder):
    e, = cc.CASES["64x48/s3/p2"]()
    want_recs, (want,) = cc.reference("64x48/s3/p2")
    total = want_recs.shape[0]
    assert total > 100
    mn, mo = uploaded(box, e[0], tick=e[1]), uploaded(box, e[2], tick=e[3])
    b = builder.b
    args = (builder.c, 1, (C.c_void_p * 1)(mn.m.value), (C.c_void_p * 1)(mo.m.value), (closure.SfvView * 1)(e[4]), (closure.SfvView * 1)(e[5]),
            (closure.SfcParams * 1)(cc.as_product(e[6])))
    counts = (closure.SfcCounts * 1)()
    assert b.build(*args, None, 0, counts) == 0 and counts[0].as_dict() == want  # the size query
    assert builder.sizes([mn], [mo], [e[4]], [e[5]], cc.as_product(e[6])) == [want]
    out = np.full(total + 8, -7.0, closure.RECORD)
    guard = out.tobytes()
    C.memset(counts, 0, C.sizeof(counts))
    assert b.build(*args, out.ctypes.data, total - 1, counts) == -1  # one record too many: SF_ERR_ARG
    assert counts[0].as_dict() == want and out.tobytes() == guard  # the counts are filled, out is untouched
    assert b.build(*args, out.ctypes.data, total, counts) == 0  # exactly enough
    assert cr.same_records(out[:total], want_recs) and out[total:].tobytes() == guard[total * 32:]
    for m in (mn, mo):
        m.close()


# ---- 3. what a build leaves alone -----------------------------------------------------------------------------------------------------
def test_a_build_only_reads(hip_auto):
    s, fused, _ = walk(hip_auto, 2, render_between=False)  # predict -> load -> solve -> fuse: a map with an index image and a prediction
    b = closure.Builder(s)
    state = lambda: (repr(fused.info()), fused.download().tobytes(), fused.index_map().tobytes(), [x.tobytes() for x in s.prediction()],  # noqa: E731
                     s.prediction_dense_stream(0))
    before = state()
    v = view.default_view(s, fused)
    for p in (closure.Params(), closure.Params(stride=1, pins=2, gate_abs=np.inf, min_time_gap=-np.inf)):
        recs, (c,) = b.build([fused], [fused], [v], [v], p)
        assert state() == before
    assert c["n_both"] == c["n_new"] > 1000 and c["n_links"] == c["n_pins"] > 1000  # the same map from the same pose: every drawn sample
    surf = fused.download()
    want = cr.build_entry(surf, fused.info()["tick"], surf, fused.info()["tick"], v, v, p)
    assert_equal((recs, [c]), (want[0], [want[1]]), "walked map")
    b.close()
    fused.close()
    s.close()


def test_the_builders_block_reused_small_large_small(box, hip_auto):
    """as tests/test_gpu_call_blocks.py: a small call, one large enough to grow the block and move every offset, the small one again"""
    def call(s, b, size):
        recs, counts = run(s, b, cc.CASES[dict(small="16x16/s2/p1", large="batch")[size]]())
        return repr(counts).encode() + recs.tobytes()

    fresh = small_solver(hip_auto, 60, 80)
    used_b, fresh_b = closure.Builder(box), closure.Builder(fresh)
    first = call(box, used_b, "small")
    large = call(box, used_b, "large")
    third = call(box, used_b, "small")
    assert len(large) > 3 * len(first) and third == first
    assert call(fresh, fresh_b, "small") == first and call(fresh, fresh_b, "large") == large
    used_b.close()
    fresh_b.close()
    fresh.close()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(box, builder, hip_auto):
    e, = cc.CASES["16x16/s1/p1"]()
    other = small_solver(hip_auto, 60, 80)
    mn, mo, foreign_map = uploaded(box, e[0]), uploaded(box, e[2]), uploaded(other, e[0][:50])
    foreign_builder = closure.Builder(other)
    b = builder.b
    state = lambda: tuple((repr(m.info()), m.download().tobytes()) for m in (mn, mo, foreign_map))  # noqa: E731
    before = state()
    one = lambda x: (C.c_void_p * 1)(x)  # noqa: E731
    vf, vt, p = (closure.SfvView * 1)(e[4]), (closure.SfvView * 1)(e[5]), (closure.SfcParams * 1)(cc.as_product(e[6]))
    counts = (closure.SfcCounts * 2)()
    C.memset(counts, 0xFB, C.sizeof(counts))
    sentinel = bytes(counts)
    out = np.full(1024, -7.0, closure.RECORD)
    guard = out.tobytes()

    def refused(code, bld, n, a_new, a_old, a_vf, a_vt, a_p, a_out=out.ctypes.data, room=1024, a_counts=counts):
        assert b.build(bld, n, a_new, a_old, a_vf, a_vt, a_p, a_out, room, a_counts) == code
        assert bytes(counts) == sentinel and out.tobytes() == guard and state() == before

    a, o = one(mn.m.value), one(mo.m.value)
    refused(-1, None, 1, a, o, vf, vt, p)                               # a null builder
    refused(-1, builder.c, -1, a, o, vf, vt, p)                         # n < 0
    refused(-1, builder.c, 32768, a, o, vf, vt, p)                      # 2n > 65535
    refused(-1, builder.c, 1, None, o, vf, vt, p)                       # null arguments
    refused(-1, builder.c, 1, a, None, vf, vt, p)
    refused(-1, builder.c, 1, a, o, None, vt, p)
    refused(-1, builder.c, 1, a, o, vf, None, p)
    refused(-1, builder.c, 1, a, o, vf, vt, None)
    refused(-1, builder.c, 1, a, o, vf, vt, p, a_counts=None)
    refused(-1, builder.c, 1, a, o, vf, vt, p, a_out=None)              # out == NULL with max_records > 0
    refused(-1, builder.c, 1, a, o, vf, vt, p, room=-1)
    refused(-1, builder.c, 1, one(None), o, vf, vt, p)                  # a null map
    refused(-1, builder.c, 1, a, one(None), vf, vt, p)
    refused(-1, builder.c, 1, one(foreign_map.m.value), o, vf, vt, p)   # a map of another handle
    refused(-1, builder.c, 1, a, one(foreign_map.m.value), vf, vt, p)
    refused(-1, foreign_builder.c, 1, a, o, vf, vt, p)                  # a builder of another handle
    for field, value in (("fx", 0.0), ("rows", 0), ("cols", 4097), ("max_depth", 0.4), ("shade", 7), ("cx", float("nan"))):  # views sfv_check_view refuses
        for which in (0, 1):
            bad = [(closure.SfvView * 1)(e[4]), (closure.SfvView * 1)(e[5])]
            setattr(bad[which][0], field, value)
            refused(-1, builder.c, 1, a, o, bad[0], bad[1], p)
    for field, value in (("rows", 17), ("cols", 15), ("cx", 8.5), ("cy", 7.0), ("fx", 20.5), ("fy", -21.0)):  # two views that differ
        bad = (closure.SfvView * 1)(e[5])
        setattr(bad[0], field, value)
        refused(-1, builder.c, 1, a, o, vf, bad, p)
    nan, inf = float("nan"), float("inf")
    bad_params = [dict(stride=0), dict(stride=4097), dict(pins=-1), dict(pins=3), dict(gate_abs=nan), dict(gate_rel=nan), dict(min_time_gap=nan), dict(w_link=nan),
                  dict(w_pin=nan), dict(gate_abs=-1.0), dict(gate_rel=-1.0), dict(w_link=-1.0), dict(w_pin=-1.0), dict(gate_rel=inf), dict(w_link=inf), dict(w_pin=inf),
                  dict(min_time_gap=inf)]
    two = lambda x, y: (C.c_void_p * 2)(x, y)  # noqa: E731
    for kw in bad_params:
        refused(-1, builder.c, 1, a, o, vf, vt, (closure.SfcParams * 1)(closure.Params(**kw)))
        refused(-1, builder.c, 2, two(mn.m.value, mn.m.value), two(mo.m.value, mo.m.value), (closure.SfvView * 2)(e[4], e[4]), (closure.SfvView * 2)(e[5], e[5]),
                (closure.SfcParams * 2)(closure.Params(), closure.Params(**kw)))  # ... in a later entry
    assert b.build(builder.c, 0, None, None, None, None, None, None, 0, None) == 0 and bytes(counts) == sentinel  # n == 0: SF_OK
    # max_depth, min_confidence and max_age may differ between the two views, shade is not read; and the call still works
    vt2 = (closure.SfvView * 1)(e[5])
    vt2[0].max_depth, vt2[0].min_confidence, vt2[0].max_age, vt2[0].shade = 19.0, 0.05, 100, 1
    assert b.build(builder.c, 1, a, o, vf, vt2, p, out.ctypes.data, 1024, counts) == 0
    for m in (mn, mo, foreign_map, foreign_builder):
        m.close()
    other.close()


def test_a_builder_whose_handle_was_destroyed_answers_state(hip_auto):
    e, = cc.CASES["16x16/s2/p1"]()
    s = small_solver(hip_auto, 60, 80)
    bld, mn, mo = closure.Builder(s), uploaded(s, e[0]), uploaded(s, e[2])
    args = ([mn], [mo], [e[4]], [e[5]], cc.as_product(e[6]))
    recs, counts = bld.build(*args)
    assert counts == cc.reference("16x16/s2/p1")[1]
    gone = C.c_void_p(s.h.value)
    s.close()
    with pytest.raises(SfError, match="failed with -3"):
        bld.build(*args)
    out_b = C.c_void_p()
    assert bld.b.builder_create(gone, C.byref(out_b)) == -3
    bld.close()  # (frees the shell)
    mn.close()
    mo.close()
    alive = small_solver(hip_auto, 60, 80)  # a live builder handed maps whose handle is gone: SF_ERR_STATE too
    bld2, mn2 = closure.Builder(alive), uploaded(alive, e[0])
    dead = small_solver(hip_auto, 60, 80)
    orphan = uploaded(dead, e[2])
    dead.close()
    counts = (closure.SfcCounts * 1)()
    code = bld2.b.build(bld2.c, 1, (C.c_void_p * 1)(mn2.m.value), (C.c_void_p * 1)(orphan.m.value), (closure.SfvView * 1)(e[4]), (closure.SfvView * 1)(e[5]),
                        (closure.SfcParams * 1)(cc.as_product(e[6])), None, 0, counts)
    assert code == -3
    for x in (orphan, mn2, bld2):
        x.close()
    alive.close()


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------------
def test_the_doubled_wall_closed_end_to_end(box, builder):
    """The old part is made as a caller makes it: map_window.extract with max_age and invert, appended into a second map. The built
    records equal the restatement's, the solve accepts them (all bound, SFD_OK) and lowers the energy, and apply_maps runs."""
    whole, old, vf, vt, tick = cc.doubled_wall()
    m_all = uploaded(box, whole, tick=tick, capacity=2 * whole.shape[0])
    old_surf = map_window.extract(m_all, map_window.Filter(max_age=3, invert=True))  # what the last 3 ticks did NOT see
    assert old_surf.tobytes() == old.tobytes()
    m_old = uploaded(box, old_surf[:0], tick=tick)
    map_window.append(m_old, old_surf)
    p = cc.params(stride=2, pins=1, gate_abs=0.01, gate_rel=0.0, min_time_gap=10.0)
    recs, (c,) = builder.build([m_all], [m_old], [vf], [vt], cc.as_product(p))
    want = cr.build_entry(whole, tick, old, tick, vf, vt, p)
    assert_equal((recs, [c]), (want[0], [want[1]]), "doubled wall")
    pos_o, t_o = deform.sample_nodes(m_old, 0.5, deform.SOLVE_MAX_NODES // 2)
    m_new = uploaded(box, whole[whole[:, 6] >= 20], tick=tick)
    pos_n, t_n = deform.sample_nodes(m_new, 0.5, deform.SOLVE_MAX_NODES // 2)
    pos, times = np.concatenate([pos_o, pos_n]), np.concatenate([t_o, t_n])
    src, dst, ct, cw = closure.as_solve_arrays(recs)
    M, rep = deform.solve(pos, times, src, dst, ct, cw, params=deform.SolveParams(time_window=5.0, w_reg=10.0, iterations=4))
    assert rep["status"] == deform.OK and rep["n_bound"] == recs.shape[0] and rep["n_unbound"] == 0
    assert rep["energy"][rep["iterations_done"]] < rep["energy"][0]
    g = deform.Graph(box)
    g.set(pos, times, M)
    counts = deform.apply_maps([m_all], g, deform.Params(time_window=5.0))[0]
    assert counts["n_surfels"] == whole.shape[0]
    bent = m_all.download()
    recent = whole[:, 6] >= 20
    before = np.linalg.norm(whole[recent, 0:3] - old[:, 0:3], axis=1).mean()
    after = np.linalg.norm(bent[recent, 0:3] - old[:, 0:3], axis=1).mean()
    print("doubled wall: %d links, %d pins, energy %.3e -> %.3e; the recent copy lies %.4f m from the old one before, %.4f m after; apply %r"
          % (c["n_links"], c["n_pins"], rep["energy"][0], rep["energy"][rep["iterations_done"]], before, after, counts))
    for x in (g, m_all, m_old, m_new):
        x.close()
