"""Moving regions (include/sf_regions.h, staticfusion_amd/regions.py) on the GPU. Every comparison is integer equality with
the NumPy statement of the header in tests/region_ref.py: image sizes below, at and one pixel past the 64 x 32 tile of the
labelling kernel, each with a random three-level frame, a checkerboard, one component, an empty mask, a serpentine, a spiral and
a frame of special values, under both connectivities and two min_pixels; a batch against single calls, max_regions around R,
labels on some entries only, the three forms against one another, the stream form after a walk past a moving sphere, the state
a label call must leave alone and every refusal.

Measured on one MI355X with the kernels as they are: every case equals the reference; nothing here asserts a time."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import region_cases as rc
import region_ref as rr
from conftest import ROOT, hip_runtime
from staticfusion_amd import SfError, SurfelMap, keyframes, regions, score, view
from staticfusion_amd.synth import Scene, se3_exp
from test_gpu_view import small_solver
from test_map_fusion import same_bits

pytestmark = pytest.mark.gpu

# rows, cols: one pixel; one row; one column; smaller than a tile; nothing a multiple of anything, two tile columns; exactly
# one tile high; three tile rows and three tile columns; an image edge one pixel past a tile edge in each direction
SHAPES = [(1, 1), (1, 9), (9, 1), (5, 7), (37, 53), (64, 48), (130, 66), (65, 33)]
COMBOS = [(4, 1), (8, 1), (4, 5), (8, 5)]  # connectivity, min_pixels
MAX_REGIONS = 24


@pytest.fixture(scope="module")
def box(hip_auto):
    s = small_solver(hip_auto, 60, 80)
    yield s
    s.close()


def to_params(p):
    return regions.Params(**{k: p[k] for k in ("z_max", "b_max", "dz_abs", "dz_rel", "connectivity", "min_pixels", "use_b")})


def same_as_reference(got_summary, got_records, got_labels, depth, b, p, max_regions, root=None):
    summ, rec, lab = rr.label(depth, b, p, max_regions, root=root)
    assert got_summary.tobytes() == summ.tobytes(), (got_summary, summ)
    assert got_records.tobytes() == rec[:int(summ["n_written"])].tobytes(), (got_records, rec[:int(summ["n_written"])])
    if got_labels is not None:
        assert got_labels.dtype == np.int32 and np.array_equal(got_labels, lab), np.argwhere(got_labels != lab)[:5]
    return summ


def entries_of(rows, cols):
    """(name, depth, b, reference parameters) of every frame under every combination, and the reference's roots per
    (frame, connectivity), which do not depend on min_pixels"""
    out, roots = [], {}
    for name, (z, b, b_max) in rc.frames_of(rows, cols).items():
        for conn, min_pixels in COMBOS:
            p = rr.params(b_max=b_max, connectivity=conn, min_pixels=min_pixels)
            if (name, conn) not in roots:
                roots[(name, conn)] = rr.components(z, rr.mask(z, b, p), p)
            out.append((name, z, b, p))
    return out, roots


def run_shape(box, rows, cols):
    entries, roots = entries_of(rows, cols)
    summ, rec, lab = regions.label_images(box, [e[1] for e in entries], [e[2] for e in entries], [to_params(e[3]) for e in entries], MAX_REGIONS,
                                          labels=True)
    seen = {}
    for q, (name, z, b, p) in enumerate(entries):
        want = same_as_reference(summ[q], rec[q], lab[q], z, b, p, MAX_REGIONS, roots[(name, p["connectivity"])])
        seen[(name, p["connectivity"], p["min_pixels"])] = want
    return seen


# ---- 1. shapes x frames x connectivities x min_pixels -------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_every_frame_equals_numpy(box, rows, cols):
    seen = run_shape(box, rows, cols)
    assert int(seen[("empty", 8, 1)]["n_mask"]) == 0 and int(seen[("one", 4, 1)]["n_components"]) == 1
    assert int(seen[("checkerboard", 4, 1)]["n_components"]) == (rows * cols + 1) // 2
    if (rows, cols) == (37, 53):
        assert int(seen[("random", 4, 1)]["n_components"]) == 454 and int(seen[("random", 8, 1)]["n_components"]) == 268
    if rows > 2 and cols > 2:
        assert int(seen[("serpentine", 4, 1)]["n_components"]) == 1 and int(seen[("spiral", 4, 1)]["n_components"]) == 1  # they chain
        assert int(seen[("special", 8, 1)]["n_mask"]) > 0


def test_qvga_once(box):
    seen = run_shape(box, 240, 320)
    assert int(seen[("serpentine", 8, 5)]["n_regions"]) == 1 and int(seen[("random", 8, 5)]["n_regions"]) > MAX_REGIONS


# ---- 2. a batch against single calls; a seventh record; max_regions; labels on some entries ------------------------------
def batch_case():
    rows, cols = 65, 33
    f = rc.frames_of(rows, cols)
    frames = [f["random"], f["special"], f["serpentine"], f["random"], f["checkerboard"], f["one"]]  # one frame twice
    ps = [rr.params(b_max=0.7, connectivity=4, min_pixels=1), rr.params(connectivity=8, min_pixels=2), rr.params(connectivity=4, min_pixels=5, dz_abs=0.001, dz_rel=0.0),
          rr.params(b_max=0.7, connectivity=4, min_pixels=1), rr.params(connectivity=8, min_pixels=1, use_b=0, z_max=0.999), rr.params(connectivity=4, min_pixels=3, b_max=-1.0)]
    return rows, cols, [(z, b) for z, b, _ in frames], ps


def raw_call(box, rows, cols, frames, ps, max_regions, want_labels, extra=1):
    """sfr_label_images at the C interface with sentinel-filled outputs one record longer than the call needs"""
    n = len(frames)
    b = regions._bind(box.api)
    col = [[np.ascontiguousarray(np.asarray(f[k], np.float32).T) for f in frames] for k in range(2)]
    dp, bp = [(C.c_void_p * n)(*[a.ctypes.data for a in col[k]]) for k in range(2)]
    summ = np.full(n + extra, -77, regions.SUMMARY_DTYPE)
    rec = np.full(n * max_regions + extra, -77, regions.REGION_DTYPE)
    labs = [np.full((cols, rows), -77, np.int32) for _ in range(n)]
    lp = (C.c_void_p * n)(*[a.ctypes.data if w else None for a, w in zip(labs, want_labels)])
    code = b.label_images(box.h, rows, cols, n, dp, bp, (regions.SfrParams * n)(*[to_params(p) for p in ps]), max_regions, summ.ctypes.data, rec.ctypes.data, lp)
    return code, summ, rec, labs


def test_a_batch_equals_single_calls(box):
    rows, cols, frames, ps = batch_case()
    m = 9
    want_labels = [True, False, True, True, False, True]
    code, summ, rec, labs = raw_call(box, rows, cols, frames, ps, m, want_labels)
    assert code == 0
    assert summ[6].tobytes() == np.full(1, -77, regions.SUMMARY_DTYPE).tobytes() and rec[6 * m].tobytes() == np.full(1, -77, regions.REGION_DTYPE).tobytes()
    for q in range(6):
        ref = rr.label(frames[q][0], frames[q][1], ps[q], m)
        assert summ[q].tobytes() == ref[0].tobytes() and rec[q * m:(q + 1) * m].tobytes() == ref[1].tobytes(), q  # the zeroed tail included
        assert (summ[q]["reserved"] == 0).all()
        if want_labels[q]:
            assert np.array_equal(labs[q].T, ref[2]), q
        else:
            assert (labs[q] == -77).all(), q
        one = regions.label_images(box, [frames[q][0]], [frames[q][1]], [to_params(ps[q])], m, labels=True)
        assert one[0][0].tobytes() == summ[q].tobytes() and one[1][0].tobytes() == rec[q * m:q * m + int(summ[q]["n_written"])].tobytes()
        assert np.array_equal(one[2][0], ref[2])
    assert summ[0].tobytes() == summ[3].tobytes() and rec[:m].tobytes() == rec[3 * m:4 * m].tobytes() and np.array_equal(labs[0], labs[3])
    assert int(summ[0]["n_regions"]) > m > int(summ[5]["n_regions"]) == 0 and int(summ[2]["n_written"]) < m  # both sides of max_regions
    again = raw_call(box, rows, cols, frames, ps, m, want_labels)
    assert again[1].tobytes() == summ.tobytes() and again[2].tobytes() == rec.tobytes() and all(a.tobytes() == c.tobytes() for a, c in zip(again[3], labs))
    # labels asked for through the module on some entries only
    some = regions.label_images(box, [f[0] for f in frames], [f[1] for f in frames], [to_params(p) for p in ps], m, labels=want_labels)
    assert [x is not None for x in some[2]] == want_labels and np.array_equal(some[2][2], labs[2].T)


def test_max_regions_around_r(box):
    z, b = rc.random_levels(37, 53)
    p = rr.params(b_max=rc.RANDOM_B_MAX, connectivity=8, min_pixels=5)
    r_total = int(rr.label(z, b, p, 0)[0]["n_regions"])
    assert r_total > 3
    full = rr.label(z, b, p, r_total)
    for m in (0, 1, r_total - 1, r_total, r_total + 3):
        code, summ, rec, labs = raw_call(box, 37, 53, [(z, b)], [p], m, [True])
        assert code == 0
        ref = rr.label(z, b, p, m)
        assert summ[0].tobytes() == ref[0].tobytes() and int(summ[0]["n_written"]) == min(m, r_total) and int(summ[0]["n_regions"]) == r_total
        assert rec[:m].tobytes() == ref[1].tobytes() and rec[m].tobytes() == np.full(1, -77, regions.REGION_DTYPE).tobytes()
        assert rec[:min(m, r_total)].tobytes() == full[1][:min(m, r_total)].tobytes() and rec[min(m, r_total):m].tobytes() == bytes(64 * max(m - r_total, 0))
        assert np.array_equal(labs[0].T, full[2]) and labs[0].max() == r_total  # the label image carries all R numbers
    # max_regions 0 with a null regions pointer
    bnd = regions._bind(box.api)
    col = [np.ascontiguousarray(a.T) for a in (z, b)]
    summ = np.zeros(1, regions.SUMMARY_DTYPE)
    assert bnd.label_images(box.h, 37, 53, 1, (C.c_void_p * 1)(col[0].ctypes.data), (C.c_void_p * 1)(col[1].ctypes.data), (regions.SfrParams * 1)(to_params(p)), 0,
                            summ.ctypes.data, None, None) == 0
    assert summ[0].tobytes() == rr.label(z, b, p, 0)[0].tobytes()


# ---- 3. the three forms -----------------------------------------------------------------------------------------------------
def test_the_three_forms_agree(box):
    rows, cols = box.rows, box.cols
    f = rc.frames_of(rows, cols)
    frames = [f["random"][:2], f["special"][:2], f["spiral"][:2]]
    ps = [rr.params(b_max=0.7, connectivity=4, min_pixels=2), rr.params(connectivity=8, min_pixels=1), rr.params(connectivity=8, min_pixels=1, use_b=0)]
    m = 7
    host = regions.label_images(box, [x[0] for x in frames], [x[1] for x in frames], [to_params(p) for p in ps], m, labels=True)
    for q in range(3):
        same_as_reference(host[0][q], host[1][q], host[2][q], frames[q][0], frames[q][1], ps[q], m)
    # device pointers (plain hipMalloc memory); the b image of the entry without use_b is missing
    rt = hip_runtime()
    blocks = []

    def dev(a):
        p = C.c_void_p()
        assert rt.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
        blocks.append(p)
        assert rt.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
        return p.value

    def back(ptr, like):
        out = np.zeros_like(like)
        assert rt.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0
        return out

    dd = [dev(np.ascontiguousarray(x[0].T)) for x in frames]
    db = [dev(np.ascontiguousarray(frames[0][1].T)), dev(np.ascontiguousarray(frames[1][1].T)), None]
    s_like, r_like, l_like = np.full(4, -77, regions.SUMMARY_DTYPE), np.full(3 * m + 1, -77, regions.REGION_DTYPE), np.full((cols, rows), -77, np.int32)
    ds, dr = dev(s_like), dev(r_like)
    dl = [dev(l_like), None, dev(l_like)]
    regions.label_images_device(box, rows, cols, dd, db, [to_params(p) for p in ps], m, ds, dr, dl)
    box.synchronize()
    gs, gr = back(ds, s_like), back(dr, r_like)
    assert gs[3].tobytes() == s_like[3].tobytes() and gr[3 * m].tobytes() == r_like[0].tobytes()
    for q in range(3):
        ref = rr.label(frames[q][0], frames[q][1], ps[q], m)
        assert gs[q].tobytes() == ref[0].tobytes() == host[0][q].tobytes() and gr[q * m:(q + 1) * m].tobytes() == ref[1].tobytes(), q
        if dl[q]:
            assert np.array_equal(back(dl[q], l_like).T, host[2][q]), q
    for p in blocks:
        rt.hipFree(p)
    # the stream form reads the stream's depth: use_b = 0, since the b image belongs to the solver
    p0 = rr.params(connectivity=8, min_pixels=3, use_b=0)
    for name in ("random", "spiral", "special"):
        z = f[name][0]
        box.set_current(0, z, np.zeros_like(z))
        assert box.current(0)[0].tobytes() == z.tobytes()
        got = regions.label_streams(box, [0, 0], [to_params(p0), to_params(dict(p0, connectivity=4))], m, labels=[False, True])
        same_as_reference(got[0][0], got[1][0], None, z, None, p0, m)
        same_as_reference(got[0][1], got[1][1], got[2][1], z, None, dict(p0, connectivity=4), m)
        assert got[2][0] is None


TORCH_CHILD = r"""
import sys
import numpy as np
import torch  # first, as bench.py does: the process then holds the HIP runtime torch brought
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import staticfusion_amd as sf
from staticfusion_amd import regions
import test_gpu_regions as t
s = t.small_solver(sf.load(), 60, 80)
rows, cols, frames, ps = t.batch_case()
m, n = 9, len(frames)
pp = [t.to_params(p) for p in ps]
host = regions.label_images(s, [f[0] for f in frames], [f[1] for f in frames], pp, m, labels=True)
dev = [[torch.from_numpy(np.ascontiguousarray(f[k].T)).cuda() for f in frames] for k in range(2)]  # column-major, like sf_get_current
summ = torch.full((n + 1, 8), -77, dtype=torch.int32, device="cuda")
rec = torch.full((n * m + 1, 8), -77, dtype=torch.int64, device="cuda")
lab = torch.full((n, cols, rows), -77, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
regions.label_images_device(s, rows, cols, [x.data_ptr() for x in dev[0]], [x.data_ptr() for x in dev[1]], pp, m, summ.data_ptr(), rec.data_ptr(),
                            [lab[q].data_ptr() if q % 2 == 0 else None for q in range(n)])
s.synchronize()
gs = summ.cpu().numpy().view(regions.SUMMARY_DTYPE).ravel()
gr = rec.cpu().numpy().view(regions.REGION_DTYPE).ravel()
gl = lab.cpu().numpy()
assert (summ.cpu().numpy()[n] == -77).all() and (rec.cpu().numpy()[n * m] == -77).all()
total = 0
for q in range(n):
    w = int(gs[q]["n_written"])
    total += w
    assert gs[q].tobytes() == host[0][q].tobytes() and gr[q * m:q * m + w].tobytes() == host[1][q].tobytes() and gr[q * m + w:(q + 1) * m].tobytes() == bytes(64 * (m - w)), q
    assert np.array_equal(gl[q].T, host[2][q]) if q % 2 == 0 else (gl[q] == -77).all(), q
print("torch tensors ok", total)
"""


def test_device_outputs_in_torch_tensors_in_a_fresh_process():
    """sfr_label_images_device on torch tensors equals the host form (a fresh process with torch imported first, for the
    reason test_gpu_view.py gives)"""
    out = subprocess.run([sys.executable, "-c", TORCH_CHILD, ROOT], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0 and "torch tensors ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert int(out.stdout.split("torch tensors ok")[1].split()[0]) > 10


# ---- 4. the stream form after real frames past a moving sphere ---------------------------------------------------------------
def sphere_walk(api, n_frames, rows=60, cols=80):
    """predict -> load -> solve -> fuse for n_frames past a sphere that moves a few centimetres a frame"""
    s = small_solver(api, rows, cols)
    m = SurfelMap(s, 4 * rows * cols)
    mp = s.default_model_params()
    scene = Scene(seed=77, sphere=True)
    xi = np.array([0.010, 0.004, 0.006, 0.002, -0.004, 0.003]) * 0.6
    frames, T = [], np.eye(4)
    for k in range(n_frames + 2):
        depth, inten = scene.render(T, 2 * cols, 2 * rows, sphere_offset=(0.04 * k, 0.0, 0.0))
        g = np.clip(np.rint(inten * 255), 1, 255).astype(np.uint8)
        frames.append((np.ascontiguousarray(np.repeat(g[::-1, :, None], 3, axis=2)), np.ascontiguousarray(np.clip(np.rint(depth[::-1] * 1000), 0, 65535).astype(np.uint16))))
        T = T @ se3_exp(xi)
    s.load_frame(0, *frames[0], 2)
    s.current_to_prediction()
    s.push_history(0)
    s.set_kb(1.05)
    s.load_frame(0, *frames[1], 2)
    s.process_frame(1)
    Tq = s.batch_results()[0]
    s.filter_depth()
    SurfelMap.fuse_frames(s, [0], [m], list(Tq), 1.0, mp)
    for k in range(2, n_frames + 2):
        s.set_kb(1.05 if k == 2 else 1.5)
        SurfelMap.predict_frames(s, [0], [m], mp)
        s.load_frame(0, *frames[k], 2)
        s.filter_depth()
        s.process_frame(k)
        Tq = s.batch_results()[0]
        SurfelMap.fuse_frames(s, [0], [m], list(Tq), 1.0, mp)
    return s, m


@pytest.fixture(scope="module")
def walked(hip_auto):
    s, m = sphere_walk(hip_auto, 5)
    yield s, m
    m.close()
    s.close()


def test_stream_form_after_a_walk_equals_image_form_and_numpy(walked):
    s, m = walked
    d, b = s.current(0)[0], s.b_image(0)
    assert (d > 0).mean() > 0.5 and b.shape == d.shape
    print("share of b < 0.5 after the walk: %.3f" % (b < 0.5).mean())
    for p in (rr.params(min_pixels=1), rr.params(connectivity=4, min_pixels=4), rr.params(b_max=0.8, min_pixels=16), rr.params(use_b=0, min_pixels=16, dz_abs=0.01)):
        a = regions.label_streams(s, [0, 0], to_params(p), 16, labels=True)
        c = regions.label_images(s, [d], [b], to_params(p), 16, labels=True)
        want = same_as_reference(a[0][0], a[1][0], a[2][0], d, b, p, 16)
        assert a[0][1].tobytes() == a[0][0].tobytes() == c[0][0].tobytes() and a[1][1].tobytes() == a[1][0].tobytes() == c[1][0].tobytes()
        assert np.array_equal(a[2][1], a[2][0]) and np.array_equal(c[2][0], a[2][0])
        assert p["use_b"] or int(want["n_mask"]) == int((d > 0).sum())
        print(p, want)
    v, u, z, w = regions.means(a[1][0])
    assert v.shape == (int(a[0][0]["n_written"]),) and (z > 0).all() and (w == 0).all()  # (the last p has use_b = 0)


# ---- 5. a label call leaves everything else alone --------------------------------------------------------------------------
def test_a_label_call_only_reads(walked):
    s, m = walked
    own = view.default_view(s, m)
    db = keyframes.KeyframeDb(s, 4, n_ferns=64, capacity=4)
    db.add_streams([0], np.eye(4)[None], [0], [1])
    view.render([m], [own])
    sprites = view.last_large_sprites(s, 1)

    def readable():
        i = m.info()
        return (s.current(0)[0].tobytes(), s.current(0)[1].tobytes(), s.b_image(0).tobytes(), i["count"], i["tick"], i["pose"].tobytes(), tuple(i["stats"]),
                m.download().tobytes(), m.index_map().tobytes(), s.prediction()[0].tobytes(), s.prediction()[1].tobytes(),
                score.score_streams([m], [own], [0]).tobytes(), db.query_streams([0], None, 2).tobytes(), db.encode_streams([0]).tobytes())

    before = readable()
    first = regions.label_streams(s, [0], None, 8, labels=True)
    z, b = rc.random_levels(130, 66)
    regions.label_images(s, [z, z], [b, None], [regions.Params(min_pixels=1), regions.Params(use_b=False)], 40, labels=True)  # grows the scratch
    again = regions.label_streams(s, [0], None, 8, labels=True)
    assert readable() == before and view.last_large_sprites(s, 1) == sprites
    assert first[0].tobytes() == again[0].tobytes() and first[1][0].tobytes() == again[1][0].tobytes() and np.array_equal(first[2][0], again[2][0])
    db.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(hip_auto):
    s = small_solver(hip_auto, 32, 40)
    b = regions._bind(s.api)
    rows, cols, n, m = 32, 40, 3, 4
    img = np.full((cols, rows), 1.0, np.float32)
    imgs = (C.c_void_p * 3)(*[img.ctypes.data] * 3)
    half = (C.c_void_p * 3)(img.ctypes.data, None, img.ctypes.data)
    good = (regions.SfrParams * 3)(*[regions.Params()] * 3)
    no_b = (regions.SfrParams * 3)(*[regions.Params(use_b=False)] * 3)
    st = (C.c_int32 * 3)(0, 0, 0)
    summ = np.full(n, -77, regions.SUMMARY_DTYPE)
    rec = np.full(n * m, -77, regions.REGION_DTYPE)
    lab = np.full((cols, rows), -77, np.int32)
    labs = (C.c_void_p * 3)(*[lab.ctypes.data] * 3)
    sp, rp = summ.ctypes.data, rec.ctypes.data
    big = 65536
    many_st = (C.c_int32 * big)()
    many_ptr = (C.c_void_p * big)(*[img.ctypes.data] * big)
    many_par = (regions.SfrParams * big)(*[regions.Params(use_b=False)] * big)
    huge_s = np.full(big, -77, regions.SUMMARY_DTYPE)
    getter = s.api.get_current(s.h, 1, img.ctypes.data_as(C.POINTER(C.c_float)), None)  # the getters' own code for a stream out of range
    assert getter != 0

    def bad_params(**kw):
        return (regions.SfrParams * 3)(regions.Params(), regions.Params(**kw), regions.Params())

    nan, inf = float("nan"), float("inf")
    cases = [
        # the stream form
        (b.label_streams, (None, n, st, good, m, sp, rp, labs), -1), (b.label_streams, (s.h, n, None, good, m, sp, rp, labs), -1),
        (b.label_streams, (s.h, n, st, None, m, sp, rp, labs), -1), (b.label_streams, (s.h, n, st, good, m, None, rp, labs), -1),
        (b.label_streams, (s.h, n, st, good, m, sp, None, labs), -1), (b.label_streams, (s.h, -1, st, good, m, sp, rp, labs), -1),
        (b.label_streams, (s.h, big, many_st, many_par, 0, huge_s.ctypes.data, None, None), -1),
        (b.label_streams, (s.h, n, st, good, -1, sp, rp, labs), -1), (b.label_streams, (s.h, n, st, good, 65536, sp, rp, labs), -1),
        (b.label_streams, (s.h, n, (C.c_int32 * 3)(0, 1, 0), good, m, sp, rp, labs), getter), (b.label_streams, (s.h, n, (C.c_int32 * 3)(0, 0, -1), good, m, sp, rp, labs), getter),
        # the host form
        (b.label_images, (None, rows, cols, n, imgs, imgs, good, m, sp, rp, labs), -1), (b.label_images, (s.h, rows, cols, n, None, imgs, good, m, sp, rp, labs), -1),
        (b.label_images, (s.h, rows, cols, n, half, imgs, good, m, sp, rp, labs), -1), (b.label_images, (s.h, rows, cols, n, imgs, None, good, m, sp, rp, labs), -1),
        (b.label_images, (s.h, rows, cols, n, imgs, half, good, m, sp, rp, labs), -1), (b.label_images, (s.h, rows, cols, n, imgs, imgs, None, m, sp, rp, labs), -1),
        (b.label_images, (s.h, rows, cols, n, imgs, imgs, good, m, None, rp, labs), -1), (b.label_images, (s.h, rows, cols, n, imgs, imgs, good, m, sp, None, labs), -1),
        (b.label_images, (s.h, rows, cols, -2, imgs, imgs, good, m, sp, rp, labs), -1),
        (b.label_images, (s.h, rows, cols, big, many_ptr, None, many_par, 0, huge_s.ctypes.data, None, None), -1),
        (b.label_images, (s.h, 0, cols, n, imgs, imgs, good, m, sp, rp, labs), -1), (b.label_images, (s.h, rows, 0, n, imgs, imgs, good, m, sp, rp, labs), -1),
        (b.label_images, (s.h, 4097, 1, n, imgs, imgs, good, m, sp, rp, labs), -1), (b.label_images, (s.h, 1, 4097, n, imgs, imgs, good, m, sp, rp, labs), -1),
        (b.label_images, (s.h, 4096, 4097, n, imgs, imgs, good, m, sp, rp, labs), -1), (b.label_images, (s.h, -rows, -cols, n, imgs, imgs, good, m, sp, rp, labs), -1),
        (b.label_images, (s.h, rows, cols, n, imgs, imgs, good, -1, sp, rp, labs), -1), (b.label_images, (s.h, rows, cols, n, imgs, imgs, good, 65536, sp, rp, labs), -1),
        # the device form (the checks come before any pointer is used)
        (b.label_images_device, (None, rows, cols, n, imgs, imgs, good, m, sp, rp, labs), -1), (b.label_images_device, (s.h, rows, cols, n, None, imgs, good, m, sp, rp, labs), -1),
        (b.label_images_device, (s.h, rows, cols, n, imgs, half, good, m, sp, rp, labs), -1), (b.label_images_device, (s.h, rows, cols, n, imgs, imgs, good, m, None, rp, labs), -1),
        (b.label_images_device, (s.h, rows, cols, n, imgs, imgs, good, m, sp, None, labs), -1), (b.label_images_device, (s.h, 4097, cols, n, imgs, imgs, good, m, sp, rp, labs), -1),
        (b.label_images_device, (s.h, rows, cols, big, many_ptr, None, many_par, 0, sp, None, None), -1), (b.label_images_device, (s.h, rows, cols, -1, imgs, imgs, good, m, sp, rp, labs), -1),
    ]
    for kw in (dict(z_max=0.0), dict(z_max=33.0), dict(z_max=nan), dict(z_max=inf), dict(b_max=nan), dict(b_max=inf), dict(dz_abs=-0.1), dict(dz_abs=nan),
               dict(dz_rel=-0.1), dict(dz_rel=inf), dict(connectivity=5), dict(min_pixels=0), dict(use_b=2)):
        cases.append((b.label_images, (s.h, rows, cols, n, imgs, imgs, bad_params(**kw), m, sp, rp, labs), -1))
        cases.append((b.label_streams, (s.h, n, st, bad_params(**kw), m, sp, rp, labs), -1))
    for q, (fn, args, want) in enumerate(cases):
        assert fn(*args) == want, (q, fn.__name__)
        assert s.api.last_error(), q
    # n == 0 is fine and touches nothing
    assert b.label_streams(s.h, 0, None, None, m, None, None, None) == 0 and b.label_images(s.h, rows, cols, 0, None, None, None, m, None, None, None) == 0
    assert b.label_images_device(s.h, rows, cols, 0, None, None, None, m, None, None, None) == 0
    with pytest.raises(SfError):
        regions.label_images(s, [np.zeros((32, 40), np.float32), np.zeros((40, 32), np.float32)], None, regions.Params(use_b=False))  # two sizes in one call
    with pytest.raises(SfError):
        regions.label_streams(s, [0], [regions.Params(), regions.Params()])
    # nothing was written
    assert (summ == np.full(1, -77, regions.SUMMARY_DTYPE)).all() and (rec == np.full(1, -77, regions.REGION_DTYPE)).all() and (lab == -77).all()
    assert (huge_s == np.full(1, -77, regions.SUMMARY_DTYPE)).all()
    # and the same arguments, valid, still work: b may be NULL when no entry sets use_b, and a null label pointer among others
    some = (C.c_void_p * 3)(None, lab.ctypes.data, None)
    assert b.label_images(s.h, rows, cols, n, imgs, None, no_b, m, sp, rp, some) == 0
    assert [int(x) for x in summ[1].tolist()[:4]] == [rows * cols, 1, 1, 1] and (lab == 1).all() and int(rec[m]["n"]) == rows * cols and int(rec[m + 1]["n"]) == 0
    s.close()


# ---- 7. the other two libraries link the same object -----------------------------------------------------------------------
@pytest.mark.parametrize("lib", ["libsf_hip_precise.so", "libsf_hip_reforder.so"])
def test_the_precise_and_reference_order_libraries_do_the_same(lib):
    import staticfusion_amd as sf

    api = sf.Api(os.path.join(os.path.dirname(sf.LIB), lib), "sf_")
    s = small_solver(api, 48, 64)
    rows, cols, frames, ps = batch_case()
    got = regions.label_images(s, [f[0] for f in frames], [f[1] for f in frames], [to_params(p) for p in ps], 9, labels=True)
    for q in range(len(frames)):
        same_as_reference(got[0][q], got[1][q], got[2][q], frames[q][0], frames[q][1], ps[q], 9)
    s.close()
