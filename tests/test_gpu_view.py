"""Free-view rendering (include/sf_view.h, staticfusion_amd/view.py) on the GPU, every comparison bit for bit: against the
CPU oracle's prediction where the oracle can be asked (the handle's resolution), against the brute-force NumPy renderer of
tests/view_ref.py everywhere else -- sizes around the wave and workgroup sizes of the splat, both shading modes, ties of the
confidence and age tests, NaNs, sprites on both sides of the large-sprite bound --, a batch against single calls, the state a
render must leave alone, every refusal, and a five-frame walk through predict / solve / fuse."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

import view_cases as vc
import view_ref
from conftest import ROOT, driver_params, hip_runtime, make_solver
from staticfusion_amd import SfError, SurfelMap, map_window, streams, view
from staticfusion_amd.synth import se3_exp
from test_map_fusion import same_bits

pytestmark = pytest.mark.gpu

TICK = 5


def small_solver(api, rows, cols):
    p = driver_params(api)
    p.ctf_levels = 2  # every pyramid level of a handle holds a multiple of 4 pixels
    return make_solver(api, rows, cols, p)


@pytest.fixture(scope="module")
def box(hip_auto):
    s = small_solver(hip_auto, 60, 80)
    yield s
    s.close()


def same_images(a, b):
    return same_bits(a["depth"], b["depth"]) and np.array_equal(a["rgb"], b["rgb"]) and np.array_equal(a["index"], b["index"])


def uploaded(s, surfels, pose=None, tick=TICK, capacity=0):
    m = SurfelMap(s, capacity or max(surfels.shape[0], s.rows * s.cols))  # (a map holds at least one frame)
    m.upload(surfels, np.eye(4, dtype=np.float32) if pose is None else pose, tick)
    return m


def random_surfels(n, cam, seed, ordered):
    """n surfels in front of the camera `cam` (a view at identity): sprites of one to a few pixels, confidences from a few
    values (exact ties with a threshold), last-seen times 1..TICK, normals tilted up to ~60 degrees; ordered: in the map's
    point order (x outer, y inner), so that a workgroup's sprites are neighbours; else shuffled"""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(-2, cam.cols + 2, n), rng.uniform(-2, cam.rows + 2, n)
    if ordered:
        o = np.lexsort((v, u))
        u, v = u[o], v[o]
    z = rng.uniform(0.5, 4.0, n)
    s = np.zeros((n, 12), np.float32)
    s[:, 0], s[:, 1], s[:, 2] = (u - cam.cx) * z / cam.fx, (v - cam.cy) * z / cam.fy, z
    s[:, 3] = rng.choice(np.array([0.1, 0.25, 0.3, 0.5], np.float32), n)
    s[:, 4] = (rng.integers(1, 256, n) << 16) + (rng.integers(1, 256, n) << 8) + rng.integers(1, 256, n)
    s[:, 6] = 1
    s[:, 7] = rng.integers(1, TICK + 1, n)
    nrm = np.stack([rng.uniform(-0.8, 0.8, n), rng.uniform(-0.8, 0.8, n), -np.ones(n)], -1)
    s[:, 8:11] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    s[:, 11] = z / abs(cam.fx) * rng.uniform(0.7, 2.5, n)
    if n > 8:
        s[3, 0] = np.nan  # a NaN position: never drawn
        s[5, 3] = np.nan  # a NaN confidence: !(NaN < threshold) draws it
        s[7, 7] = np.nan  # a NaN time: drawn unless the age test is on
    return s


# ---- 1. against the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", vc.SIZES)
def test_hip_equals_the_oracles_prediction(hip_auto, ora, rows, cols):
    so = make_solver(ora, rows, cols, driver_params(ora))
    vc.prime_pure_render(so, rows, cols)
    sh = small_solver(hip_auto, rows, cols)
    mp0 = sh.default_model_params()
    surf = vc.frame_surfels(rows, cols, mp0)
    m = SurfelMap(sh, rows * cols)
    for intr in (dict(cx=mp0.cx, cy=mp0.cy, fx=mp0.fx, fy=mp0.fy), vc.other_intrinsics(mp0)):
        mp = vc.pure_render_params(so, intr, 0.25, 20.0, time=3)
        for name, pose in vc.poses():
            so.predict_from_model(0, surf, pose, mp)
            d, inten = so.prediction()
            v = vc.view_of(mp, pose, rows, cols)
            m.upload(surf, pose, 3)
            got = view.render([m], [v])[0]
            assert same_bits(got["depth"], d) and same_bits(view_ref.grey(got["rgb"]), inten), name
            drawn = got["depth"] > 0
            assert np.array_equal(got["index"] == -1, ~drawn) and np.all(got["index"][drawn] < surf.shape[0])
            assert np.array_equal(got["rgb"][drawn], view_ref.decode_colour(surf[got["index"][drawn], 4]))
            assert not got["rgb"][~drawn].any()
            assert drawn.any() == (name != "away")
            assert same_images(view.render_surfels(sh, surf, v, tick=3), got), name  # the same buffer without a map
    m.close()
    sh.close()
    so.close()


def test_hip_equals_the_oracles_prediction_of_discs_that_cross_the_camera_plane(hip_auto, ora):
    """tilted discs with rad sqrt(2) above the depth of their centre, among 500 small surfels (surfel_cases.crossing): a corner
    of their diamond lies behind the camera, its projection is mirrored, and the bounding rectangle of the corners does not
    hold the disc's image -- the oracle, like the shaders, has no such rectangle"""
    import surfel_cases as sc

    case = sc.crossing()
    rows, cols = case.rows, case.cols
    so = make_solver(ora, rows, cols, driver_params(ora))
    sh = small_solver(hip_auto, rows, cols)
    preds = []
    for s in (so, sh):
        vc.prime_pure_render(s, rows, cols)
        mp = vc.pure_render_params(s, dict(cx=case.cx, cy=case.cy, fx=case.fx, fy=case.fy), case.min_confidence, case.max_depth, time=case.tick)
        s.predict_from_model(0, case.surfels, case.pose, mp)
        preds.append(s.prediction())
    (d, inten), (dh, ih) = preds
    assert same_bits(dh, d) and same_bits(ih, inten)
    v = vc.view_of(mp, case.pose, rows, cols)
    got = view.render_surfels(sh, case.surfels, v, tick=case.tick)
    assert view.last_large_sprites(sh, 1) == [len(case.big)]
    assert same_images(got, view_ref.render(case.surfels, v, tick=case.tick))
    assert same_bits(np.where(got["depth"] > 0, got["depth"], np.float32(0)), d) and same_bits(view_ref.grey(got["rgb"]), inten)  # (no clip at z <= 0 in a view)
    won = np.isin(got["index"], case.big)
    assert won.mean() > 0.5 and (got["index"] >= 0).mean() > 0.9 and (~won & (got["index"] >= 0)).any()
    sh.close()
    so.close()


# ---- 2. against NumPy, at sizes the oracle cannot take ---------------------------------------------------------------
VIEWS = [(1, 1, 0.5, 0.5, 1.3, 1.1), (37, 53, 25.25, 19.5, 47.0, -44.0), (48, 64, 30.5, 25.0, 61.0, 58.5)]  # rows, cols, cx, cy, fx, fy


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 511, 512, 513, 5003])
@pytest.mark.parametrize("geom", VIEWS, ids=lambda g: "%dx%d" % (g[1], g[0]))
def test_hip_equals_numpy(box, n, geom):
    rows, cols, cx, cy, fx, fy = geom
    pose = se3_exp(np.array([0.02, -0.03, 0.05, 0.03, -0.02, 0.05])).astype(np.float32)
    # three settings of one map in ONE call: a confidence threshold some s[3] equal exactly + age <= 1; normals + age 0
    # (only what was seen at the map's tick); everything, unstable surfels too
    settings = [dict(min_confidence=0.25, max_age=1), dict(min_confidence=0.3, max_age=0, shade=view.SHADE_NORMAL, max_depth=3.0),
                dict(min_confidence=0.0, max_age=-1)]
    views = [view.View(pose, cx, cy, fx, fy, rows, cols, **kw) for kw in settings]
    surf = random_surfels(n, view.View(np.eye(4), cx, cy, fx, fy, rows, cols), seed=n + rows, ordered=(n % 2 == 1))
    m = uploaded(box, surf)
    got = view.render([m] * 3, views)
    drawn = []
    for q, v in enumerate(views):
        ref = view_ref.render(surf, v, tick=TICK)
        assert same_images(got[q], ref), settings[q]
        assert np.array_equal(got[q]["index"] == -1, got[q]["depth"] == 0)
        drawn.append(int((ref["index"] >= 0).sum()))
    if n > 500 and rows > 1:  # the settings do select differently, and the ties are there
        assert 0 < drawn[1] < drawn[0] < drawn[2]
        won = surf[got[0]["index"][got[0]["index"] >= 0]]
        assert (won[:, 3] == np.float32(0.25)).any() and not (won[:, 3] < np.float32(0.25)).any()
        assert (won[:, 7] == TICK - 1).any() and not (won[:, 7] < TICK - 1).any()
    assert same_bits(m.download(), surf)
    m.close()


# ---- 3. large sprites ------------------------------------------------------------------------------------------------
def flat_surfel(x, y, z, r, rgb, conf=0.5):
    s = np.zeros(12, np.float32)
    s[:4] = (x, y, z, conf)
    s[4] = (rgb[0] << 16) + (rgb[1] << 8) + rgb[2]
    s[7] = TICK
    s[8:11] = (0, 0, -1)
    s[11] = r
    return s


def large_view(**kw):
    return view.View(np.eye(4), 32.0, 24.0, 64.0, 64.0, 48, 64, **kw)


@pytest.mark.parametrize("where", ["in front", "behind"])
def test_one_sprite_larger_than_the_image(box, where):
    v = large_view(min_confidence=0.0)
    small = random_surfels(500, v, seed=17, ordered=True)
    small[:, 2] = np.clip(small[:, 2], 1.0, 3.0)
    big = flat_surfel(0.01, -0.02, 0.45, 2.0, (9, 8, 7)) if where == "in front" else flat_surfel(0.01, -0.02, 3.5, 6.0, (9, 8, 7))
    surf = np.concatenate([small[:250], big[None], small[250:]])
    px = view_ref.sprite_pixels(surf, v, tick=TICK)
    assert px[250] == 64 * 48 and (px[np.arange(501) != 250] <= view_ref.LARGE_PIXELS).all()
    m = uploaded(box, surf)
    got = view.render([m], [v])[0]
    assert view.last_large_sprites(box, 1) == [1]
    ref = view_ref.render(surf, v, tick=TICK)
    assert same_images(got, ref)
    share = (got["index"] == 250).mean()
    assert share == 1.0 if where == "in front" else 0.0 < share < 1.0
    m.close()


def test_sprites_on_both_sides_of_the_bound(box):
    """half of the surfels above the bound of 32 x 32 pixels, some exactly at it: both kernels write the same keys"""
    v = large_view()
    radii = np.linspace(0.15, 0.25, 401).astype(np.float32)
    cand = np.stack([flat_surfel(0.0, 0.0, 1.0, r, (1 + k % 250, 2, 3)) for k, r in enumerate(radii)])
    px = view_ref.sprite_pixels(cand, v, tick=TICK)
    at, below, above = np.flatnonzero(px == 1024), np.flatnonzero(px < 1024), np.flatnonzero(px > 1024)
    assert at.size and below.size and above.size, "the radii reach a sprite of exactly 32 x 32 pixels"
    pick = np.concatenate([below[-8:], at[:4], above[:12]])
    rng = np.random.default_rng(5)
    centred = cand[rng.permutation(pick)]
    # the same radii away from the centre, tilted and at other depths: sprites cut by the image border
    rest = []
    for k in range(24):
        s = flat_surfel(rng.uniform(-0.5, 0.5), rng.uniform(-0.35, 0.35), rng.uniform(0.8, 1.4), rng.uniform(0.12, 0.4), (50 + k, 60, 70))
        n = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), -1.0])
        s[8:11] = n / np.linalg.norm(n)
        rest.append(s)
    surf = np.concatenate([centred, np.stack(rest)])
    px = view_ref.sprite_pixels(surf, v, tick=TICK)
    n_large = int((px > view_ref.LARGE_PIXELS).sum())
    assert (px == 1024).any() and 0.35 * len(px) <= n_large <= 0.65 * len(px)
    m = uploaded(box, surf)
    for shade in (view.SHADE_COLOUR, view.SHADE_NORMAL):
        v.shade = shade
        got = view.render([m], [v])[0]
        assert view.last_large_sprites(box, 1) == [n_large]
        assert same_images(got, view_ref.render(surf, v, tick=TICK))
    winners = np.unique(got["index"][got["index"] >= 0])
    assert (px[winners] > 1024).any() and (px[winners] <= 1024).any()  # both paths won pixels
    m.close()


# ---- 4. batch --------------------------------------------------------------------------------------------------------
def batch_case(s):
    va = view.View(np.eye(4), 30.5, 25.0, 61.0, 58.5, 48, 64, min_confidence=0.0)
    data = [random_surfels(n, va, seed=40 + q, ordered=(q != 1)) for q, n in enumerate((1500, 700, 513))]
    maps = [uploaded(s, d, tick=TICK + q) for q, d in enumerate(data)] + [uploaded(s, np.zeros((0, 12), np.float32))]
    p1 = se3_exp(np.array([0.1, 0.0, -0.1, 0.0, 0.1, 0.0])).astype(np.float32)
    p2 = view.look_at((0.6, -0.4, -0.3), (0.0, 0.0, 2.0))
    views = [va, view.View(p1, 30.5, 25.0, 61.0, 58.5, 48, 64, min_confidence=0.25, max_age=2),
             view.View(p2, 12.0, 9.5, 20.0, 20.0, 19, 23, min_confidence=0.0, shade=view.SHADE_NORMAL),
             view.View(p1, 30.5, 25.0, 61.0, 58.5, 48, 64), view.View(np.eye(4), 17.0, 20.0, 33.0, 35.0, 37, 31, max_depth=2.5), va]
    order = [0, 0, 0, 1, 2, 3]  # the same map three times, two other maps, an empty one
    return maps, data + [np.zeros((0, 12), np.float32)], views, order


def test_a_batch_equals_single_calls_and_numpy(box):
    maps, data, views, order = batch_case(box)
    batch = view.render([maps[o] for o in order], views)
    assert view.last_large_sprites(box, 6) == [0] * 6
    for q, o in enumerate(order):
        single = view.render([maps[o]], [views[q]])[0]
        ref = view_ref.render(data[o], views[q], tick=maps[o].info()["tick"])
        assert same_images(batch[q], single) and same_images(batch[q], ref), q
    assert not (batch[5]["index"] >= 0).any() and (batch[4]["index"] >= 0).any()
    # a NULL entry is skipped without disturbing its neighbours; a NULL array is no output at all
    b = view._bind(box.api)
    n = 6
    mp = (C.c_void_p * n)(*[maps[o].m.value for o in order])
    va = (view.SfvView * n)(*views)
    d = [np.full((v.rows, v.cols), -7.5, np.float32) for v in views]
    i = [np.full((v.rows, v.cols), -7, np.int32) for v in views]
    dp = (C.c_void_p * n)(*[None if q == 2 else a.ctypes.data for q, a in enumerate(d)])
    ip = (C.c_void_p * n)(*[None if q in (0, 5) else a.ctypes.data for q, a in enumerate(i)])
    assert b.render_maps(box.h, n, mp, va, dp, None, ip) == 0
    for q in range(n):
        assert np.all(d[q] == np.float32(-7.5)) if q == 2 else same_bits(d[q], batch[q]["depth"]), q
        assert np.all(i[q] == -7) if q in (0, 5) else np.array_equal(i[q], batch[q]["index"]), q
    assert b.render_maps(box.h, n, mp, va, None, None, None) == 0
    # device pointers (plain hipMalloc memory): the same images, after the handle's stream has drained
    rt = hip_runtime()
    sizes = [(v.rows * v.cols * 4, v.rows * v.cols * 3, v.rows * v.cols * 4) for v in views]
    dev = []
    for sz in sizes:
        ptrs = []
        for nbytes in sz:
            p = C.c_void_p()
            assert rt.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
            ptrs.append(p)
        dev.append(ptrs)
    view.render_device([maps[o] for o in order], views, [p[0].value for p in dev], [p[1].value for p in dev], [p[2].value for p in dev])
    box.synchronize()
    for q, v in enumerate(views):
        out = dict(depth=np.zeros((v.rows, v.cols), np.float32), rgb=np.zeros((v.rows, v.cols, 3), np.uint8), index=np.zeros((v.rows, v.cols), np.int32))
        for p, k in zip(dev[q], ("depth", "rgb", "index")):
            assert rt.hipMemcpy(out[k].ctypes.data_as(C.c_void_p), p, C.c_size_t(out[k].nbytes), 2) == 0
            rt.hipFree(p)
        assert same_images(out, batch[q]), q
    for m in maps:
        m.close()


TORCH_CHILD = r"""
import sys
import numpy as np
import torch  # first, as bench.py does: the process then holds the HIP runtime torch brought
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import staticfusion_amd as sf
from staticfusion_amd import view
import test_gpu_view as t
s = t.small_solver(sf.load(), 60, 80)
maps, data, views, order = t.batch_case(s)
host = view.render([maps[o] for o in order], views)
dev = [(torch.full((v.rows, v.cols), -1.0, dtype=torch.float32, device="cuda"), torch.full((v.rows, v.cols, 3), 9, dtype=torch.uint8, device="cuda"),
        torch.full((v.rows, v.cols), -9, dtype=torch.int32, device="cuda")) for v in views]
torch.cuda.synchronize()
view.render_device([maps[o] for o in order], views, *[[d[k].data_ptr() for d in dev] for k in range(3)])
s.synchronize()
for q in range(len(views)):
    got = dict(depth=dev[q][0].cpu().numpy(), rgb=dev[q][1].cpu().numpy(), index=dev[q][2].cpu().numpy())
    assert t.same_images(got, host[q]), q
print("torch tensors ok", sum(int((h["index"] >= 0).sum()) for h in host))
"""


def test_render_into_torch_tensors_in_a_fresh_process():
    """sfv_render_maps_device into torch tensors equals the host variant. A fresh process, torch imported first as in
    bench.py: a process that loads the product library first and torch afterwards holds two copies of the HIP runtime
    (conftest.hip_runtime), which is no setting a user of both would be in."""
    out = subprocess.run([sys.executable, "-c", TORCH_CHILD, ROOT], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0 and "torch tensors ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert int(out.stdout.split("torch tensors ok")[1].split()[0]) > 1000


# ---- 5. nothing else moves -------------------------------------------------------------------------------------------
def walk(api, n_frames, render_between, rows=60, cols=80):
    """predict -> load -> solve -> fuse for n_frames of a synthetic walk (tools/full_pipeline_bench.py's loop, host frames); with
    render_between, free views of the map are drawn before every predict and every fuse. Returns what every frame left."""
    from staticfusion_amd.synth import Scene

    s = small_solver(api, rows, cols)
    m = SurfelMap(s, 4 * rows * cols)
    mp = s.default_model_params()
    scene = Scene(seed=77, sphere=False)
    xi = np.array([0.010, 0.004, 0.006, 0.002, -0.004, 0.003]) * 0.6
    frames, T = [], np.eye(4)
    for k in range(n_frames + 2):
        depth, inten = scene.render(T, 2 * cols, 2 * rows)
        g = np.clip(np.rint(inten * 255), 1, 255).astype(np.uint8)
        frames.append((np.ascontiguousarray(np.repeat(g[::-1, :, None], 3, axis=2)), np.ascontiguousarray(np.clip(np.rint(depth[::-1] * 1000), 0, 65535).astype(np.uint16))))
        T = T @ se3_exp(xi)
    orbit = view.View(view.look_at((0.5, -0.3, -0.5), (0.0, 0.0, 2.0)), 50.0, 40.0, 90.0, 90.0, 77, 101, min_confidence=0.0)

    def peek():
        if render_between:
            view.render([m, m], [orbit, view.default_view(s, m)])

    s.load_frame(0, *frames[0], 2)
    s.current_to_prediction()
    s.push_history(0)
    s.set_kb(1.05)
    s.load_frame(0, *frames[1], 2)
    s.process_frame(1)
    Tq = s.batch_results()[0]
    s.filter_depth()
    SurfelMap.fuse_frames(s, [0], [m], list(Tq), 1.0, mp)
    out = []
    for k in range(2, n_frames + 2):
        s.set_kb(1.05 if k == 2 else 1.5)
        peek()
        SurfelMap.predict_frames(s, [0], [m], mp)
        pred, dense = s.prediction(), s.prediction_dense_stream(0)
        s.load_frame(0, *frames[k], 2)
        s.filter_depth()
        s.process_frame(k)
        Tq = s.batch_results()[0]
        peek()
        SurfelMap.fuse_frames(s, [0], [m], list(Tq), 1.0, mp)
        out.append(dict(pred=pred, dense=dense, T=np.array(Tq), info=m.info(), surfels=m.download(), index=m.index_map()))
    return s, m, out


def same_walk(a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        assert same_bits(x["pred"][0], y["pred"][0]) and same_bits(x["pred"][1], y["pred"][1]) and x["dense"] == y["dense"], k
        assert same_bits(x["T"], y["T"]) and x["info"]["count"] == y["info"]["count"] and x["info"]["stats"] == y["info"]["stats"], k
        assert same_bits(x["surfels"], y["surfels"]) and np.array_equal(x["index"], y["index"]), k


def test_a_render_moves_nothing_else(hip_auto):
    s, m, plain = walk(hip_auto, 3, render_between=False)
    s2, m2, peeked = walk(hip_auto, 3, render_between=True)
    same_walk(plain, peeked)  # predict, solve and fuse give what they give without the renders
    m2.close()
    s2.close()
    # the state a caller can read, before and after a render
    SurfelMap.predict_frames(s, [0], [m], s.default_model_params())

    def readable():
        i = m.info()
        return (i["count"], i["tick"], i["pose"].tobytes(), tuple(i["stats"]), m.download().tobytes(), m.index_map().tobytes(),
                s.prediction()[0].tobytes(), s.prediction()[1].tobytes(), s.prediction_dense_stream(0))

    assert m.info()["tick"] > 1
    before = readable()
    surf = m.download()
    v = view.View(view.look_at((0.4, 0.2, -0.6), (0.0, 0.0, 2.0)), 300.0, 200.0, 500.0, 500.0, 400, 600, min_confidence=0.0)
    got = view.render([m, m], [v, view.default_view(s, m)])
    assert (got[0]["index"] >= 0).mean() > 0.3
    view.render_surfels(s, surf, v, tick=m.info()["tick"])
    assert readable() == before
    # straight after a cull (surfel indices have moved) and after the map has followed its stream to another handle
    f = map_window.Filter(min_confidence=0.25)
    kept = map_window.cull([m], [f])[0]
    assert 0 < kept < surf.shape[0]
    small = view.View(view.view_pose(view.default_view(s, m)), 20.0, 15.0, 33.0, 33.0, 30, 40, min_confidence=0.0)
    after_cull = m.download()
    assert same_images(view.render([m], [small])[0], view_ref.render(after_cull, small, tick=m.info()["tick"]))
    s3 = small_solver(hip_auto, 60, 80)
    streams.rebind_map(m, s3)
    assert same_images(view.render([m], [small])[0], view_ref.render(after_cull, small, tick=m.info()["tick"]))
    b = view._bind(hip_auto)
    assert b.render_maps(s.h, 1, (C.c_void_p * 1)(m.m.value), C.byref(small), None, None, None) == -1  # the old handle no longer owns it
    m.close()
    s3.close()
    s.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(box, hip_auto):
    b = view._bind(box.api)
    good = view.View(np.eye(4), 20.0, 15.0, 33.0, 33.0, 30, 40, min_confidence=0.0)
    surf = random_surfels(300, good, seed=1, ordered=True)
    m1, m2 = uploaded(box, surf), uploaded(box, surf[:65])
    other = small_solver(hip_auto, 60, 80)
    mo = uploaded(other, surf)
    d = [np.full((30, 40), -7.5, np.float32) for _ in range(2)]
    c = [np.full((30, 40, 3), 201, np.uint8) for _ in range(2)]
    i = [np.full((30, 40), -7, np.int32) for _ in range(2)]
    dp, cp, ip = ((C.c_void_p * 2)(*[a.ctypes.data for a in arr]) for arr in (d, c, i))
    two = (C.c_void_p * 2)(m1.m.value, m2.m.value)
    foreign = (C.c_void_p * 2)(m1.m.value, mo.m.value)
    with_null = (C.c_void_p * 2)(m1.m.value, None)
    vs = (view.SfvView * 2)(good, good)
    nan, inf = float("nan"), float("inf")
    bad_pose = np.eye(4)
    bad_pose[2, 3] = nan
    bad_views = [dict(pose=bad_pose), dict(cx=inf), dict(cy=nan), dict(fx=nan), dict(fy=inf), dict(min_confidence=nan), dict(max_depth=inf),
                 dict(rows=0), dict(rows=4097), dict(cols=0), dict(cols=4097), dict(fx=0.0), dict(fy=0.0), dict(max_depth=0.4), dict(max_depth=-2.0),
                 dict(shade=2), dict(shade=-1)]

    def bad(**kw):
        base = dict(pose=np.eye(4), cx=20.0, cy=15.0, fx=33.0, fy=33.0, rows=30, cols=40, min_confidence=0.0)
        base.update(kw)
        return (view.SfvView * 2)(good, view.View(**base))

    big = (C.c_void_p * 65536)(*([m1.m.value] * 65536))
    many = (view.SfvView * 65536)(*([good] * 65536))
    for fn in (b.render_maps, b.render_maps_device):
        cases = [(None, 2, two, vs, dp, cp, ip), (box.h, 2, None, vs, dp, cp, ip), (box.h, 2, two, None, dp, cp, ip), (box.h, -1, two, vs, dp, cp, ip),
                 (box.h, 2, foreign, vs, dp, cp, ip), (other.h, 2, two, vs, dp, cp, ip), (box.h, 2, with_null, vs, dp, cp, ip),
                 (box.h, 65536, big, many, None, None, None)]
        cases += [(box.h, 2, two, bad(**kw), dp, cp, ip) for kw in bad_views]
        for q, args in enumerate(cases):
            if fn is b.render_maps_device and q >= 8:
                continue  # (host addresses in the output arrays: a refused call never looks at them, the first eight show it)
            assert fn(*args) == -1, q
            assert box.api.last_error(), q
        assert fn(box.h, 0, None, None, None, None, None) == 0  # an empty batch is fine
    sp = surf.ctypes.data_as(C.POINTER(C.c_float))
    args = (d[0].ctypes.data, c[0].ctypes.data, i[0].ctypes.data)
    assert b.render_surfels(None, sp, 300, 1, C.byref(good), *args) == -1 and b.render_surfels(box.h, None, 300, 1, C.byref(good), *args) == -1
    assert b.render_surfels(box.h, sp, -1, 1, C.byref(good), *args) == -1 and b.render_surfels(box.h, sp, 300, 1, None, *args) == -1
    for kw in bad_views:
        assert b.render_surfels(box.h, sp, 300, 1, C.byref(bad(**kw)[1]), *args) == -1, kw
    v = view.SfvView()
    assert b.default_view(None, None, C.byref(v)) == -1 and b.default_view(box.h, None, None) == -1 and b.default_view(box.h, mo.m, C.byref(v)) == -1
    with pytest.raises(SfError):
        view.render([m1, mo], [good, good])  # maps of two solvers
    with pytest.raises(SfError):
        view.render([m1], [good, good])
    for arr, fill in ((d, np.float32(-7.5)), (c, 201), (i, -7)):
        assert all(np.all(a == fill) for a in arr)
    # the handle goes first: the map is an empty shell that fails cleanly
    other.close()
    one = (C.c_void_p * 1)(mo.m.value)
    assert b.render_maps(box.h, 1, one, C.byref(good), dp, cp, ip) == -3 and b.default_view(box.h, mo.m, C.byref(v)) == -3  # SF_ERR_STATE
    assert all(np.all(a == np.float32(-7.5)) for a in d)
    # and the live maps still render; the default view is what the header says
    assert (view.render([m1, m2], [good, good])[1]["index"] >= 0).any()
    dv = view.default_view(box, m1)
    mp = box.default_model_params()
    assert (dv.rows, dv.cols, dv.cx, dv.cy, dv.fx, dv.fy) == (60, 80, mp.cx, mp.cy, mp.fx, mp.fy)
    assert (dv.min_confidence, dv.max_depth, dv.max_age, dv.shade) == (0.25, 20.0, -1, view.SHADE_COLOUR)
    assert np.array_equal(view.view_pose(dv), m1.info()["pose"]) and np.array_equal(view.view_pose(view.default_view(box)), np.eye(4))
    for m in (m1, m2, mo):
        m.close()


# ---- 7. end to end ---------------------------------------------------------------------------------------------------
def test_five_frame_walk_rendered_at_the_maps_own_pose(hip_auto):
    s, m, out = walk(hip_auto, 5, render_between=False)
    assert len(out) == 5 and out[-1]["info"]["tick"] == 7
    mp = s.default_model_params()
    v = view.default_view(s, m)
    v.min_confidence = mp.conf_high
    got = view.render([m], [v])[0]
    surf = m.download()
    assert same_images(got, view_ref.render(surf, v, tick=m.info()["tick"]))
    drawn = got["index"] >= 0
    assert drawn.mean() > 0.5 and np.all(surf[got["index"][drawn], 3] >= np.float32(mp.conf_high))
    truth = out[-1]["pred"][0]  # the prediction the last solve started from: the same scene one frame earlier
    both = drawn & (truth > 0)
    assert both.mean() > 0.5 and np.median(np.abs(got["depth"] - truth)[both]) < 0.05
    m.close()
    s.close()
