"""The map registration on the GPU (include/sf_register.h, staticfusion_amd/register.py): every result, the system of every
iteration, every status, count and pair is held to tests/register_ref.py bit for bit -- the corner scene; sources of every size
around a wave and a workgroup; destinations of 0, 1 and 1587 surfels; sixteen entries in one call (eight starts on one shared
table, mixed iteration counts with zero records behind the shorter ones, a FEW_PAIRS at iteration 0, a DEGENERATE, two cells on
one destination, a table whose keys collide); an entry alone against the same entry in the batch; the same call twice; the
maps untouched; the lifetime of a registrar; every refusal; and a dry-run merge with the resulting transform."""
import ctypes as C

import numpy as np
import pytest

import join_ref
import register_cases as rc
import register_ref as rr
from staticfusion_amd import SfError, join, register
from test_gpu_view import small_solver, uploaded

pytestmark = pytest.mark.gpu

RESULT_KEYS = ("status", "iterations_done", "n_first", "ss_first", "n_last", "ss_last", "n_sampled", "n_outside")
EMPTY = np.zeros((0, 12), np.float32)


@pytest.fixture(scope="module")
def box(hip_auto):
    s = small_solver(hip_auto, 60, 80)
    yield s
    s.close()


@pytest.fixture(scope="module")
def reg(box):
    r = register.Registrar(box)
    yield r
    r.close()


@pytest.fixture(scope="module")
def scene():
    dst, src, R, t = rc.corner()
    return dict(dst=dst, src=src, R=R, t=t, tab=rr.table(dst, 0.1), want=rr.register(dst, src))


def state(m):
    i = m.info()
    try:
        index = m.index_map().tobytes()
    except SfError as e:
        index = str(e)
    return repr(i), m.download().tobytes(), index


def same_entry(res, systems, pairs, want, where):
    """one entry of a call against (result, systems, pairs, E) of the restatement"""
    w_res, w_sys, w_pairs, _ = want
    got = {k: int(res[k]) for k in RESULT_KEYS}
    assert got == {k: int(w_res[k]) for k in RESULT_KEYS}, (where, got, w_res)
    assert np.asarray(res["T"]).tobytes() == w_res["T"].tobytes(), where
    assert not np.asarray(res["reserved"]).any(), where
    assert np.array_equal(systems.view(np.int64).reshape(-1, 32), w_sys), where
    assert np.array_equal(pairs, w_pairs), where


def run(reg, box, entries, want=None):
    """entries: (dst surfels, src surfels, T0 or None, params); one call with systems and pairs, held to the restatement (want:
    what an earlier run of the same entries computed). Surfel arrays that are the same object share one map. Returns (results,
    systems, pairs, wanted)."""
    made = {}
    mp = lambda a: made.setdefault(id(a), uploaded(box, a))  # noqa: E731
    d, s = [mp(e[0]) for e in entries], [mp(e[1]) for e in entries]
    before = [state(m) for m in made.values()]
    slots = max(e[3].iterations for e in entries) + 1
    T0 = None if all(e[2] is None for e in entries) else [np.eye(4, dtype=np.float32) if e[2] is None else e[2] for e in entries]
    res, systems, pairs = reg.register_maps(d, s, T0, [rc.as_product(e[3]) for e in entries], systems=True, pairs=True)
    assert [state(m) for m in made.values()] == before  # both maps of every entry are only read
    tabs = {}
    if want is None:
        want = []
        for dd, ss, t0, p in entries:
            if (id(dd), p.cell) not in tabs:
                tabs[id(dd), p.cell] = rr.table(dd, p.cell)
            want.append(rr.register(dd, ss, t0, p, slots=slots, tab=tabs[id(dd), p.cell]))
    for q in range(len(entries)):
        same_entry(res[q], systems[q], pairs[q], want[q], q)
    for m in made.values():
        m.close()
    return res, systems, pairs, want


# ---- 1. the scene ------------------------------------------------------------------------------------------------------
def test_the_scene_against_the_restatement(box, reg, scene):
    res, systems, pairs, want = run(reg, box, [(scene["dst"], scene["src"], None, rr.Params())])
    assert res[0]["status"] == register.OK and res[0]["iterations_done"] == 10 and res[0]["n_last"] > 250
    E = register.transform_matrix(res[0])[:3].astype(np.float64).ravel()
    assert rc.estimate_error(E, scene["R"], scene["t"]) <= 1e-4  # (the restatement's own condition, carried over by the equality above)
    # without the systems and the pairs the result is the same: one record per entry that is cleared between linearisations
    d, s = uploaded(box, scene["dst"]), uploaded(box, scene["src"])
    plain = reg.register_maps([d], [s])
    assert plain.tobytes() == res.tobytes()
    d.close()
    s.close()


@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 256, 257, 529])
def test_source_counts_around_a_wave_and_a_workgroup(box, reg, scene, count):
    p = rr.Params(min_pairs=6, iterations=3)
    some = np.ascontiguousarray(scene["src"][np.random.default_rng(5).permutation(529)[:count]])  # (of all three planes)
    res, _, _, want = run(reg, box, [(scene["dst"], some, rc.as_matrix(*rc.motion(0.7)), p)])
    assert res[0]["n_sampled"] == count
    if count >= 63:
        assert res[0]["status"] == register.OK and res[0]["iterations_done"] == 3 and res[0]["n_last"] > count // 4


@pytest.mark.parametrize("count", [0, 1, 1587])
def test_destination_counts(box, reg, scene, count):
    p = rr.Params(min_pairs=6, iterations=2)
    dst = np.ascontiguousarray(scene["dst"][:count])
    res, _, pairs, _ = run(reg, box, [(dst, scene["src"], rc.as_matrix(scene["R"], scene["t"]), p)])
    if count < 1587:
        assert res[0]["status"] == register.FEW_PAIRS and res[0]["iterations_done"] == 0 and res[0]["n_sampled"] == 529 and (pairs[0] <= 0).all()
    else:
        assert res[0]["status"] == register.OK and res[0]["n_last"] > 250


def test_an_empty_source_and_strides(box, reg, scene):
    res, _, pairs, _ = run(reg, box, [(scene["dst"], EMPTY, None, rr.Params()), (scene["dst"], scene["src"], None, rr.Params(stride=3, min_pairs=6)),
                                      (scene["dst"], scene["src"], None, rr.Params(stride=1000, min_pairs=6)),
                                      (scene["dst"], scene["src"], None, rr.Params(min_confidence=0.5, min_pairs=6))])
    assert res[0]["status"] == register.FEW_PAIRS and res[0]["n_sampled"] == 0 and pairs[0].size == 0
    assert res[1]["n_sampled"] == 177 and (pairs[1][np.arange(529) % 3 != 0] == register.NOT_SAMPLED).all() and res[2]["n_sampled"] == 1
    assert 0 < res[3]["n_sampled"] < 529


# ---- 2. sixteen entries in one call ----------------------------------------------------------------------------------
def batch(scene):
    dst, src = scene["dst"], scene["src"]
    plane_d, plane_s, _, _ = rc.corner(axes=(2,))
    coll_d, coll_s = rc.colliding_pair()
    far = rc.moved_by_inverse(dst[::-1][::3], *rc.motion(1.0, 10.0))
    entries = []
    for k in range(8):  # eight starts on one destination: one table
        entries.append((dst, src, rc.as_matrix(*rc.motion(0.1 * k)), rr.Params(iterations=(10, 3, 7, 1)[k % 4])))
    entries.append((dst, far, None, rr.Params()))                                       # FEW_PAIRS at iteration 0
    entries.append((plane_d, plane_s, None, rr.Params(iterations=4)))                   # DEGENERATE
    entries.append((plane_d, plane_s, None, rr.Params(iterations=4, damping=1e-3)))     # ... and with damping it runs
    entries.append((dst, src, rc.as_matrix(*rc.motion(0.5)), rr.Params(cell=0.05, dist_max=0.025)))  # a second cell on the same destination
    entries.append((coll_d, coll_s, None, rr.Params(min_pairs=6, iterations=2)))        # the colliding-key table
    entries.append((src, dst, rc.as_matrix(scene["R"].T, -scene["R"].T @ scene["t"]), rr.Params(iterations=5, stride=2)))  # the other way round
    entries.append((dst, src, None, rr.Params(min_confidence=0.4, iterations=6)))
    entries.append((dst, src, None, rr.Params(iterations=64, min_cos=0.9)))
    assert len(entries) == 16
    return entries


def test_sixteen_entries_in_one_call(box, reg, scene):
    entries = batch(scene)
    res, systems, pairs, want = run(reg, box, entries)
    assert systems.shape == (16, 65)
    assert res[8]["status"] == register.FEW_PAIRS and res[8]["iterations_done"] == 0 and res[8]["n_first"] == 0
    assert res[9]["status"] == register.DEGENERATE and res[9]["iterations_done"] == 0 and res[10]["status"] == register.OK and res[10]["iterations_done"] == 4
    assert res[12]["n_last"] >= 8
    for q in (1, 3, 9, 12):  # zero records behind the shorter entries and behind a stop
        last = int(res[q]["iterations_done"]) + 1  # the linearisations the entry made
        assert not systems[q].view(np.int64).reshape(65, 32)[last:].any() and systems[q]["n"][last - 1] == res[q]["n_last"]
    # an entry alone against the same entry inside the batch, and the same call twice
    for q in (0, 5, 11, 13):
        per = entries[q][3].iterations + 1
        alone = (want[q][0], want[q][1][:per], want[q][2], want[q][3])
        r1, s1, p1, _ = run(reg, box, [entries[q]], [alone])
        assert r1[0].tobytes() == res[q].tobytes() and s1[0].tobytes() == systems[q][:per].tobytes() and np.array_equal(p1[0], pairs[q])
    again = run(reg, box, entries, want)
    assert again[0].tobytes() == res.tobytes() and again[1].tobytes() == systems.tobytes() and all(np.array_equal(a, b) for a, b in zip(again[2], pairs))


# ---- 3. what a result is good for ------------------------------------------------------------------------------------
def test_a_dry_run_merge_with_the_result(box, reg, scene):
    d, s = uploaded(box, scene["dst"]), uploaded(box, scene["src"])
    res = reg.register_maps([d], [s])
    T = register.transform_matrix(res[0])
    assert T.tobytes() == scene["want"][0]["T"].reshape(4, 4).T.tobytes()
    for M in (T, np.eye(4, dtype=np.float32)):
        counts = join.merge([d], [s], [M], join.Params(cell=0.02, dry_run=True))[0]
        want = join_ref.merge(scene["dst"], scene["src"], M, cell=0.02)[1]
        assert counts == want, (counts, want)
    assert join_ref.merge(scene["dst"], scene["src"], T, cell=0.02)[1]["n_shared"] > join_ref.merge(scene["dst"], scene["src"], None, cell=0.02)[1]["n_shared"]
    d.close()
    s.close()


# ---- 4. lifetime and refusals ----------------------------------------------------------------------------------------
def test_the_lifetime_of_a_registrar(hip_auto, scene):
    s = small_solver(hip_auto, 48, 64)
    r, d, m = register.Registrar(s), uploaded(s, scene["dst"]), uploaded(s, scene["src"])
    first = r.register_maps([d], [m])
    assert first[0]["n_last"] == scene["want"][0]["n_last"]
    gone = C.c_void_p(s.h.value)
    s.close()  # the handle goes first: the registrar is a shell
    with pytest.raises(SfError, match="failed with -3"):
        r.register_maps([d], [m])
    out = C.c_void_p()
    assert r.b.registrar_create(gone, C.byref(out)) == -3 and r.b.registrar_create(None, C.byref(out)) == -1
    r.close()  # (frees the shell)
    r.close()
    d.close()
    m.close()
    alive, dead = small_solver(hip_auto, 48, 64), small_solver(hip_auto, 48, 64)  # a live registrar handed a map whose handle is gone: SF_ERR_STATE too
    r2, orphan, d2, m2 = register.Registrar(alive), uploaded(dead, scene["src"]), uploaded(alive, scene["dst"]), uploaded(alive, scene["src"])
    dead.close()
    res = np.full(1, 0x5B, np.uint8).repeat(128)
    one = lambda x: (C.c_void_p * 1)(x.m.value)  # noqa: E731
    assert r2.b.register_maps(r2.r, 1, one(d2), one(orphan), None, C.byref(register.Params()), res.ctypes.data, None, None) == -3 and (res == 0x5B).all()
    # the registrar goes first: clean, and the handle goes on working with another one
    assert r2.register_maps([d2], [m2]).tobytes() == first.tobytes()
    r2.close()
    r3 = register.Registrar(alive)
    assert r3.register_maps([d2], [m2]).tobytes() == first.tobytes()
    for x in (orphan, d2, m2, r3):
        x.close()
    alive.close()


def test_refusals_change_nothing(box, reg, hip_auto, scene):
    other = small_solver(hip_auto, 48, 64)
    d, s, foreign = uploaded(box, scene["dst"]), uploaded(box, scene["src"]), uploaded(other, scene["src"])
    foreign_reg = register.Registrar(other)
    b = reg.b
    before = [state(m) for m in (d, s, foreign)]
    res = np.full(3, 0, register.RESULT_DTYPE)  # (one more than any call fills: a guard)
    res.view(np.uint8)[:] = 0xFB
    sentinel = res.tobytes()
    systems = np.full((2 * 11 + 1) * 32, -7, np.int64)
    pair_room = [np.full(529 + 4, -7, np.int32), np.full(1587 + 4, -7, np.int32)]
    two = lambda x, y: (C.c_void_p * 2)(x, y)  # noqa: E731
    pp = two(pair_room[0].ctypes.data, pair_room[1].ctypes.data)
    dst, src, pr = two(d.m.value, s.m.value), two(s.m.value, d.m.value), (register.SfgParams * 2)(register.Params(), register.Params())
    T0 = np.tile(np.eye(4, dtype=np.float32).ravel(), 2)
    fp = C.POINTER(C.c_float)

    def refused(code, r=reg.r, n=2, a_dst=dst, a_src=src, a_T0=T0.ctypes.data_as(fp), a_pr=pr, a_res=res.ctypes.data):
        assert b.register_maps(r, n, a_dst, a_src, a_T0, a_pr, a_res, systems.ctypes.data, pp) == code
        assert box.api.last_error()
        assert res.tobytes() == sentinel and (systems == -7).all() and all((p == -7).all() for p in pair_room) and [state(m) for m in (d, s, foreign)] == before

    refused(-1, r=None)                                         # a null registrar
    refused(-1, n=-1)
    refused(-1, n=65536)                                        # (the bound comes before anything is read)
    refused(-1, a_dst=None)                                     # null arguments
    refused(-1, a_src=None)
    refused(-1, a_pr=None)
    refused(-1, a_res=None)
    refused(-1, a_dst=two(d.m.value, None))                     # a null map
    refused(-1, a_src=two(s.m.value, s.m.value))                # dst[1] == src[1]
    refused(-1, a_src=two(s.m.value, foreign.m.value))          # a map of another handle than the registrar's
    refused(-1, r=foreign_reg.r)                                # ... and the registrar of another handle than the maps'
    for k, v in ((3, np.nan), (16 + 12, np.inf), (31, -np.inf)):
        bad = T0.copy()
        bad[k] = v
        refused(-1, a_T0=bad.ctypes.data_as(fp))                # a non-finite entry of T0
    nan, inf = float("nan"), float("inf")
    bad_params = [dict(cell=0.0), dict(cell=nan), dict(cell=1e-45), dict(dist_max=0.0), dict(dist_max=0.0501), dict(cell=4.0, dist_max=1.5), dict(min_cos=1.5),
                  dict(min_cos=-1.5), dict(min_cos=nan), dict(min_confidence=nan), dict(damping=-1.0), dict(damping=inf), dict(iterations=0), dict(iterations=65),
                  dict(stride=0), dict(min_pairs=5)]
    for kw in bad_params:
        refused(-1, a_pr=(register.SfgParams * 2)(register.Params(), register.Params(**kw)))  # ... in a later entry
    assert b.register_maps(reg.r, 0, None, None, None, None, None, None, None) == 0 and res.tobytes() == sentinel  # nothing at all: SF_OK
    # and the call still works: two entries, the second the other way round; a null T0 and a null pair pointer among the pairs
    pp[1] = None
    assert b.register_maps(reg.r, 2, dst, src, None, pr, res.ctypes.data, systems.ctypes.data, pp) == 0
    want = [rr.register(scene["dst"], scene["src"]), rr.register(scene["src"], scene["dst"])]
    for q in (0, 1):
        same_entry(res[q], systems[q * 11 * 32:(q + 1) * 11 * 32], pair_room[0][:529] if q == 0 else want[1][2], want[q], q)
    assert res[2:].tobytes() == sentinel[256:] and systems[-32:].tolist() == [-7] * 32 and (pair_room[0][529:] == -7).all() and (pair_room[1] == -7).all()
    assert [state(m) for m in (d, s, foreign)] == before
    for x in (d, s, foreign, foreign_reg):
        x.close()
    other.close()
