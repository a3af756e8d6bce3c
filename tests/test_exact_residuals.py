"""computeResidualsAgainstPreviousImage (stage_residuals, sf_residuals.h) and buildSegmImage against EXACT fp64 references
(tests/exact_ref.py, section E): the mean residual of every cluster recomputed from what the ABI shows -- the images fed, T()
after every frame (bit for bit what the ring's poses hold), labels(0) -- and held to a bound that is a COUNT of float roundings
(the table above section E), not to the distance from the float oracle, whose own sequential sum is off by 1e-4 relative.

Frames are driven through process_frame(k) as the drivers do; from k = 5 on every frame is checked, k = 5 .. 11 on the first
scene, so that every ring slot has been warped from and pushed to. The scenes are the smallest at which each path of the stage can
go wrong (the table at SCENES); none is a quiet walk, for the reason given there.

A source of the five-frame warp whose centi-pixel truncation could fall on either side moves a few 1e-6 of a cluster's mean: the
reference carries every such source through the sum under each of its candidate positions and the check is the ADMISSIBLE
INTERVAL [s_lo / (2 (c_max + 1)) - bound, s_hi / (2 (c_min + 1)) + bound]. What that interval can see is stated per cluster by
the SENSITIVITY condition: half its width is at most a quarter of what dropping the cluster's median-term pixel changes. Clusters
that miss it are printed and not counted as asserted (they are still held to their interval); the caps on them are asserted.

CPU part: the oracle inside the float-order interval on every scene; the reference against the fixture solver_160x120.npz; seven
perturbations that the older 1e-3 bar accepts. GPU part (marked one by one): the three product builds and libsf_hip_reforder.so
on the same scenes, one launch of several frames, the separate entry points, eight streams in one handle.
"""
import os

import numpy as np
import pytest

import exact_ref as E
from conftest import GOLDEN, config2_params, driver_params, make_solver
from staticfusion_amd.synth import Scene, quantise_and_decimate, se3_exp
from test_exact_references import ORDERED_MAX_PIXELS, tan_half_fovh

PRODUCT = ("throughput", "latency", "cluster")
FIRST, LAST = 5, 11  # frames whose residuals are checked


# ------------------------------------------------------------------------------------------------------------------------------
#  scenes: name -> (rows, cols, params(api), frames factory, last checked frame)
# ------------------------------------------------------------------------------------------------------------------------------
def _walk(seed, rows, cols, n, xi, sphere_step=(0.0, 0.0, 0.0), edit=None, room=None):
    scene = Scene(seed=seed, sphere=True, sphere_seed=seed + 17, **(room or {}))
    frames, T = [], np.eye(4)
    for k in range(n):
        d, i = quantise_and_decimate(*scene.render(T, 2 * cols, 2 * rows, sphere_offset=tuple(k * s for s in sphere_step)))
        d, i = d.copy(), i.copy()
        if edit is not None:
            edit(k, d, i)
        frames.append((d, i))
        T = T @ se3_exp(xi)
    return frames


def _ripple(amplitude, period=9.0):
    """the depth of every odd frame grows by amplitude p(u, v), p = max(0, sin sin)^2: a quarter of the pixels of EVERY cluster
    differ from the frame warped from (five frames back: the other parity) like something that moved, so that a cluster's terms
    are skewed and its mean is far from its median term -- what lets a single pixel be seen"""
    def edit(k, d, i):
        v, u = np.mgrid[0:d.shape[0], 0:d.shape[1]]
        p = np.maximum(0.0, np.sin(2 * np.pi * u / period) * np.sin(2 * np.pi * v / period)) ** 2
        d[...] = np.where(d > 0, d + np.float32((k % 2) * amplitude) * p.astype(np.float32), d)

    return edit


def _panel(delta, box=(0.2, 0.8, 0.1, 0.65)):
    """the same drift, k delta, for a rectangle of the image (fractions of rows and columns): flat inside, so only its edges add to
    what the ambiguous sources can move -- the skew a single cluster of every pixel needs"""
    def edit(k, d, i):
        r, c = d.shape
        sub = d[int(box[0] * r):int(box[1] * r), int(box[2] * c):int(box[3] * c)]
        sub[...] = np.where(sub > 0, sub + np.float32(k * delta), sub)

    return edit


def _both(*edits):
    def edit(k, d, i):
        for e in edits:
            e(k, d, i)

    return edit


XI_WALK = (0.006, -0.004, 0.005, 0.003, -0.004, 0.002)


def _holes(k, d, i):
    """depth holes in every frame (pixels without a cluster), a band that is zero in the frames warped FROM but not in the frames
    five later (old depth 0 under a current depth: idiff = 0 there)"""
    d[60:90, 150:190] = 0
    d[::19, ::11] = 0
    if k <= 3:
        d[:, 40:70] = 0


def _left_third_empty(k, d, i):
    """the left part of the frames that are warped from in frames 7 .. 9 is zero: the clusters there receive nothing"""
    if 2 <= k <= 4:
        d[:, :56] = 0


SEG = lambda **over: (lambda a: driver_params(a, kb=1.5, **over))
# A quiet walk through a static room does NOT meet the sensitivity condition: the terms of a cluster are then a few millimetres,
# all alike, and dropping one of 800 moves the mean by 1e-8 .. 1e-6, while the warp's own float evaluation (e_depth: six roundings
# on a depth of 3 m, 1e-6 m) alone allows 9e-7 -- measured on the oracle: 121 of 168 clusters insensitive. What a single pixel can
# show therefore depends on the SCENE: every scene below gives a quarter of the pixels of every cluster a depth that differs from
# the frame warped from (_ripple; its period is long against a pixel, because what the ambiguous sources can move grows with the
# depth gradient), and the two scenes with one cluster of every pixel use a drifting rectangle, the larger one in a room five
# times nearer (bounds in units of the depth's ulp: five times tighter). Measured on the oracle with the product's bound, clusters
# not sensitive / non-empty clusters: 4 / 168, 0 / 3, 1 / 72, 2 / 71, 1 / 72, 0 / 3, 4 / 72, 4 / 105 in the order below.
NEAR_ROOM = dict(wall_z=0.6, floor_y=0.2, side_x=-0.32)
XI_NEAR = (0.0012, -0.0008, 0.001, 0.003, -0.004, 0.002)
# 0.06 rad about the optical axis per frame: 0.3 rad over the five-frame chain
XI_ROLL = (0.006, -0.004, 0.005, 0.003, -0.004, 0.06)
SCENES = {
    "walk_120x160": (120, 160, SEG(), lambda: _walk(77, 120, 160, LAST + 1, XI_WALK, edit=_ripple(0.2, 20.0)), LAST),
    "odometry_120x160": (120, 160, lambda a: config2_params(a, levels=3), lambda: _walk(78, 120, 160, 8, XI_NEAR, edit=_panel(0.08), room=NEAR_ROOM), 7),
    "tiny_32x48": (32, 48, SEG(ctf_levels=2), lambda: _walk(41, 32, 48, 8, XI_WALK, (0.02, 0, 0), edit=_ripple(0.2, 6.0)), 7),
    "tiny_20x52": (20, 52, SEG(ctf_levels=2), lambda: _walk(42, 20, 52, 8, XI_WALK, edit=_ripple(0.2, 6.0)), 7),
    "odd_40x42": (40, 42, SEG(ctf_levels=3), lambda: _walk(43, 40, 42, 8, XI_WALK, edit=_ripple(0.2, 6.0)), 7),
    "odometry_48x43": (48, 43, lambda a: config2_params(a, levels=2), lambda: _walk(6, 48, 43, 8, XI_WALK, edit=_panel(0.05)), 7),
    "holes_roll_200x264": (200, 264, SEG(ctf_levels=3), lambda: _walk(31, 200, 264, 8, XI_ROLL, (0.02, 0, 0), _both(_ripple(0.5, 30.0), _holes)), 7),
    "moving_sphere_120x160": (120, 160, SEG(), lambda: _walk(79, 120, 160, 10, XI_WALK, (0.03, 0.0, 0.0), _both(_ripple(0.2), _left_third_empty)), 9),
}
SEG_OFF = ("odometry_120x160", "odometry_48x43")
_frames_cache = {}


def frames_of(name):
    if name not in _frames_cache:
        _frames_cache[name] = SCENES[name][3]()
    return _frames_cache[name]


# ------------------------------------------------------------------------------------------------------------------------------
#  driving and checking
# ------------------------------------------------------------------------------------------------------------------------------
def path_of(s, kind):
    """the summation path of the stage at level 0 (exact_ref.residuals_reference): the oracle and the reference-order build sum
    in the reference's float order; a product build splats in fixed point unless the image has at most 2048 pixels AND one
    workgroup serves the stream (sf_reforder.h: splat_ordered), and always sums the terms in fixed point"""
    if kind in ("oracle", "reforder"):
        return "float"
    assert kind in PRODUCT, kind
    G = s.variant()[2]
    return "ordered+integer" if G == 1 and s.rows * s.cols <= ORDERED_MAX_PIXELS else "integer"


def product_path(rows, cols):
    return "ordered+integer" if rows * cols <= ORDERED_MAX_PIXELS else "integer"


def reference_of(s, old, cur, Ts, k, stream=0):
    """the exact residuals of frame k of `stream`: `old` the images pushed at frame k - 5, `cur` those of frame k, Ts[i] = T() after
    frame i (what stage_push_history stored in the ring)"""
    T = E.history_transform({i % E.HISTORY: Ts[i] for i in range(k - E.HISTORY + 1, k)}, Ts[k], k)
    seg = bool(s.params.segmentation_enabled)
    return E.residuals_reference(*old, *cur, s.labels(0, stream) if seg else None, T, tan_half_fovh(s), s.params.k_photometric_res, seg)


def dropped_pixel(ref, l):
    """the mean of cluster l without its median-term pixel (sum and count)"""
    c = int(ref["c"][l])
    t = np.sort(ref["terms"][ref["counted"] & (ref["labels"] == l)])
    assert t.size == c and c >= 2
    return (ref["sum_abs"][l] - t[c // 2]) / (2.0 * c)


def sensitivity(ref, path):
    """per cluster of at least two counted pixels: (half-width of the admissible interval, change made by dropping the
    median-term pixel)"""
    return {l: (0.5 * (ref["hi"][path][l] - ref["lo"][path][l]), abs(dropped_pixel(ref, l) - ref["value"][l]))
            for l in range(E.N_LABELS) if ref["c"][l] >= 2}


def check_frame(s, kind, old, cur, Ts, k, tally, stream=0, sens_path=None):
    """residuals and b image of frame k of `stream` against the exact references; adds to `tally`"""
    ref = reference_of(s, old, cur, Ts, k, stream)
    path = path_of(s, kind)
    fails, ratio = E.check_residuals(ref, s.cluster_residuals(stream), path)
    assert not fails, (kind, path, "frame %d" % k, fails)
    sens = sensitivity(ref, sens_path or path)
    weak = [l for l, (half, change) in sens.items() if not half <= 0.25 * change]
    for l in weak:
        print("frame %d cluster %d (%d pixels): half-width %.3g against a dropped pixel's %.3g -- not counted as asserted" % (k, l, ref["c"][l], *sens[l]))
    # buildSegmImage, exactly, from the build's own b and labels and the exact residual intervals
    uncertain = (ref["c_min"] == 0) & (ref["c_max"] > 0)
    img, chk, n_open = E.segm_image_reference(ref["labels"], s.b(stream), (ref["lo"][path], ref["hi"][path]), uncertain)
    b_img = s.b_image(stream)
    assert n_open <= 1, ("clusters whose interval straddles 0.017", kind, k, n_open)
    assert np.array_equal(b_img[chk].view(np.uint32), img[chk].view(np.uint32)), (kind, "b_image", k, np.argwhere(chk & (b_img != img))[:3])
    tally["ratio"] = max(tally.get("ratio", 0.0), ratio)
    for q, v in (("clusters", len(sens)), ("weak", len(weak)), ("open", n_open), ("frames", 1), ("empty", int((ref["c_max"] == 0).sum()))):
        tally[q] = tally.get(q, 0) + v
    for q in ("n_ambiguous", "n_ambiguous_cells", "n_capped_cells", "n_idiff_zero", "n_invalid_label", "n_untouched", "n_sources"):
        tally[q] = tally.get(q, 0) + ref[q]
    with np.errstate(invalid="ignore"):
        tally["below"] = tally.get("below", 0) + int((ref["hi"][path] < E.STATIC_RESIDUAL).sum())
        tally["above"] = tally.get("above", 0) + int((ref["lo"][path] >= E.STATIC_RESIDUAL).sum())
    return ref


def run_frame(s, k, fused=True):
    if fused:
        s.process_frame(k)
    else:  # the drivers' sequence call by call (sf.h: process_frame): stage_push_history copies the ring's images itself
        s.build_pyramid(True)
        s.run_solver(True)
        if k >= E.HISTORY:
            s.residuals_vs_history(k)
        s.build_segm_image()
        s.push_history(k)


def drive(api, kind, name, fused=True, check=True, last=None, keep=None):
    """-> (tally, cluster residuals of every checked frame, solver, Ts)"""
    rows, cols, mk, _, scene_last = SCENES[name]
    last = last or scene_last
    frames = frames_of(name)
    s = make_solver(api, rows, cols, mk(api))
    s.set_current(0, *frames[0])
    s.current_to_prediction()
    s.push_history(0)
    Ts, tally, res = {0: s.T()}, {}, []
    for k in range(1, last + 1):
        s.set_prediction(0, *frames[k - 1])
        s.set_current(0, *frames[k])
        run_frame(s, k, fused)
        Ts[k] = s.T()
        if k >= FIRST:
            res.append(s.cluster_residuals().copy())
            if check:
                check_frame(s, kind, frames[k - E.HISTORY], frames[k], Ts, k, tally, sens_path=product_path(rows, cols) if kind in ("oracle", "reforder") else None)
    return tally, res, s, Ts


def conclude(name, kind, tally):
    print("residuals %s %s: %d frames, %d clusters asserted, %d not sensitive, %d left out of the image check; max |got - exact| / bound %.3g; "
          "%d of %d sources ambiguous (%d cells, %d capped)"
          % (name, kind, tally["frames"], tally["clusters"] - tally["weak"], tally["weak"], tally["open"], tally["ratio"], tally["n_ambiguous"],
             tally["n_sources"], tally["n_ambiguous_cells"], tally["n_capped_cells"]))
    assert tally["weak"] * 10 <= tally["clusters"], ("more than 1 in 10 clusters not sensitive to a dropped pixel", name, tally["weak"], tally["clusters"])
    if name in SEG_OFF:
        assert tally["weak"] == 0, (name, "a segmentation-off scene with an insensitive cluster")
    if name == "holes_roll_200x264":
        assert tally["n_idiff_zero"] > 0 and tally["n_invalid_label"] > 0 and tally["n_untouched"] > 0, tally
    if name == "moving_sphere_120x160":
        assert tally["below"] > 0 and tally["above"] > 0 and tally["empty"] > 0, tally
    return tally


# ------------------------------------------------------------------------------------------------------------------------------
#  CPU part
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_oracle_residuals_meet_the_bounds(ora, name):
    """the oracle inside the float-order interval; the caps on insensitive clusters (here and for the reference-order build) with
    the PRODUCT's bound (the geometry decides
    them, and the oracle's poses are the product's to 1e-6): the scenes are fit for the GPU part"""
    conclude(name, "oracle", drive(ora, "oracle", name)[0])


def test_oracle_separate_entry_points(ora):
    fused, split = (drive(ora, "oracle", "odd_40x42", fused=f, check=not f) for f in (True, False))
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(fused[1], split[1]))


def test_reference_on_the_golden_history(ora):
    """the fixture's ring (hist_depth / hist_intensity / hist_T / hist_labels0 of solver_160x120.npz, ring index 5) through the
    reference: the oracle, driven as test_golden.check_history_residuals drives it, lies inside the float-order interval computed
    from the FIXTURE's arrays, and so do the recorded residuals"""
    import test_golden

    w = np.load(os.path.join(GOLDEN, "solver_160x120.npz"))
    s = test_golden.check_history_residuals(ora)
    Ts = {k: w["hist_T"][k - 1].astype(np.float32) for k in range(1, 6)}
    assert all(np.array_equal(Ts[k], w["hist_T"][k - 1]) for k in Ts), "the fixture's poses are not float32 values"
    T = E.history_transform({i % E.HISTORY: Ts[i] for i in range(1, 5)}, Ts[5], 5)
    ref = E.residuals_reference(w["hist_depth"][0], w["hist_intensity"][0], w["hist_depth"][5], w["hist_intensity"][5], w["hist_labels0"], T,
                                tan_half_fovh(s), s.params.k_photometric_res, True)
    fails, ratio = E.check_residuals(ref, w["hist_cluster_res"], "float")
    print("golden history: max |recorded - exact| / bound %.3g" % ratio)
    assert not fails, fails
    if np.array_equal(s.T(), Ts[5]):
        fails, ratio = E.check_residuals(ref, s.cluster_residuals(), "float")
        print("golden history: max |oracle - exact| / bound %.3g" % ratio)
        assert not fails, fails


# ------------------------------------------------------------------------------------------------------------------------------
#  the bound rejects what the 1e-3 bar accepts
# ------------------------------------------------------------------------------------------------------------------------------
def old_bar_accepts(bad, good):
    """np.allclose(got, oracle, rtol=1e-3, atol=1e-6) of test_frame_sequence_with_history, with the correct answer for the oracle's"""
    return bool(abs(bad - good) <= 1e-6 + 1e-3 * abs(good))


def rejected(ref, l, bad, path):
    return not ref["lo"][path][l] <= bad <= ref["hi"][path][l]


@pytest.fixture(scope="module")
def holes_frame(ora):
    """frame 5 of holes_roll_200x264 on the oracle: inputs of the reference and the reference"""
    name, k = "holes_roll_200x264", 5
    _, _, s, Ts = drive(ora, "oracle", name, check=False, last=k)
    frames = frames_of(name)
    args = dict(labels0=s.labels(0), tan_half_fovh=tan_half_fovh(s), k_photometric_res=s.params.k_photometric_res, segmentation_enabled=True)
    ref = reference_of(s, frames[0], frames[k], Ts, k)
    sens = sensitivity(ref, "integer")
    good = [l for l, (half, change) in sens.items() if half <= 0.25 * change]
    return dict(frames=frames, Ts=Ts, k=k, args=args, ref=ref, sensitive=good, got=s.cluster_residuals())


def _verdicts(tag, ref, l, bad, expect_old_bar, expect_float):
    """the product's bound must refuse `bad` for cluster l; what the 1e-3 bar and the float-order bound make of it is asserted as
    stated (a wrong statement fails: nothing is hidden)"""
    good = ref["value"][l]
    verdict = (old_bar_accepts(bad, good), rejected(ref, l, bad, "integer"), rejected(ref, l, bad, "float"))
    print("%s: cluster %d (%d pixels) exact %.9g, perturbed %.9g (relative %.3g); bound integer %.3g, float order %.3g; 1e-3 bar accepts: %s, "
          "product bound rejects: %s, float-order bound rejects: %s"
          % (tag, l, ref["c"][l], good, bad, abs(bad - good) / good, ref["bound"]["integer"][l], ref["bound"]["float"][l], *verdict))
    assert verdict[1], (tag, "the product's bound accepts the perturbation")
    assert verdict[0] == expect_old_bar, (tag, "1e-3 bar", verdict[0])
    assert verdict[2] == expect_float, (tag, "float-order bound", verdict[2])


def test_rejects_a_dropped_pixel(holes_frame):
    """1. the median-term pixel of the largest sensitive cluster dropped from sum and count: 2.3e-4 relative. (The float-order bound
    of this cluster, gamma_c sum |t| = 1.9e-4 relative for its 3216 pixels, happens to see it too.)"""
    ref = holes_frame["ref"]
    l = max(holes_frame["sensitive"], key=lambda q: ref["c"][q])
    _verdicts("dropped pixel", ref, l, dropped_pixel(ref, l), True, True)


def test_rejects_2c_for_2c_plus_2(holes_frame):
    """2. sum / 2c in place of sum / 2 (c + 1): 1 / c relative, inside 1e-3 for the clusters of more than 1000 pixels"""
    ref = holes_frame["ref"]
    l = max(holes_frame["sensitive"], key=lambda q: ref["c"][q])
    assert ref["c"][l] > 1000
    _verdicts("2c", ref, l, ref["sum_abs"][l] / (2.0 * ref["c"][l]), True, True)


def test_rejects_k_photometric_off_by_a_thousandth(holes_frame):
    """3. k_photometric_res x 1.001: 8e-5 relative here -- inside the float-order bound (1.9e-4 relative), which therefore cannot see
    it: only the builds that sum in fixed point are held to this"""
    h = holes_frame
    args = dict(h["args"], k_photometric_res=h["args"]["k_photometric_res"] * 1.001)
    T = E.history_transform({i % 5: h["Ts"][i] for i in range(1, 5)}, h["Ts"][5], 5)
    bad = E.residuals_reference(*h["frames"][0], *h["frames"][5], args["labels0"], T, args["tan_half_fovh"], args["k_photometric_res"], True)
    ref = h["ref"]
    # the cluster with the largest photometric share among the sensitive ones
    l = max(h["sensitive"], key=lambda q: (bad["value"][q] - ref["value"][q]) / ref["bound"]["integer"][q])
    _verdicts("k x 1.001", ref, l, bad["value"][l], True, False)


def test_rejects_idiff_not_zeroed(holes_frame):
    """4. intensity_diff = intensityCurrent also where the old depth of the pixel is 0"""
    ref = holes_frame["ref"]
    i_cur = np.asarray(holes_frame["frames"][5][1], np.float64)
    d_cur = np.asarray(holes_frame["frames"][5][0], np.float64)
    zeroed = ref["counted"] & (ref["idiff"] == 0.0) & (i_cur != 0.0)
    assert zeroed.any()
    l = int(np.argmax(np.bincount(ref["labels"][zeroed], minlength=E.N_LABELS)[:E.N_LABELS]))
    m = ref["counted"] & (ref["labels"] == l)
    t = np.abs(d_cur[m] - ref["depth_w"][m]) + ref["k"] * np.abs(i_cur[m] - ref["intensity_w"][m])
    assert np.allclose(np.sort(np.where(zeroed[m], ref["terms"][m], t)), np.sort(ref["terms"][m]), rtol=0, atol=1e-15)  # (the planes reproduce the terms)
    _verdicts("idiff kept", ref, l, t.sum() / (2.0 * (ref["c"][l] + 1)), False, True)


def test_rejects_the_wrong_ring_slot(holes_frame):
    """5. the images of slot (index - 4) % 5 warped in place of those of (index - 5) % 5"""
    h = holes_frame
    a = h["args"]
    T = E.history_transform({i % 5: h["Ts"][i] for i in range(1, 5)}, h["Ts"][5], 5)
    bad = E.residuals_reference(*h["frames"][1], *h["frames"][5], a["labels0"], T, a["tan_half_fovh"], a["k_photometric_res"], True)
    ref = h["ref"]
    l = max(h["sensitive"], key=lambda q: ref["c"][q])
    _verdicts("ring slot", ref, l, bad["value"][l], False, True)


def test_rejects_a_chain_without_T_odometry(holes_frame):
    """6. the product of the ring's poses without the current T_odometry"""
    h = holes_frame
    a = h["args"]
    T = E.history_transform({i % 5: h["Ts"][i] for i in range(1, 5)}, np.eye(4, dtype=np.float32), 5)
    bad = E.residuals_reference(*h["frames"][0], *h["frames"][5], a["labels0"], T, a["tan_half_fovh"], a["k_photometric_res"], True)
    ref = h["ref"]
    l = max(h["sensitive"], key=lambda q: ref["c"][q])
    _verdicts("no T_odometry", ref, l, bad["value"][l], False, True)


def test_rejects_a_term_truncated_to_20_bits(ora):
    """7. one term cut to a multiple of 2^-20 (a slip of FIX_RES). A term is known to e_t = bd + k bi + ... only -- 1.7e-6 at a depth
    of 3 m, 3.5e-7 at 0.6 m, more than the 2^-20 it can lose at 3 m -- and the sum of a cluster to c times that: ONE truncated
    term shows where the cluster is one or two pixels and the depth small. So: frame 5 of the near room, every pixel but one taken
    out of the only cluster (label 24), the pixel chosen for the largest loss against its own e_t. For a cluster of hundreds of
    pixels no derived bound sees one such term, the product's included: asserted on the full cluster."""
    name, k = "odometry_120x160", 5
    _, _, s, Ts = drive(ora, "oracle", name, check=False, last=k)
    frames = frames_of(name)
    T = E.history_transform({i % 5: Ts[i] for i in range(1, 5)}, Ts[5], 5)
    run = lambda labels: E.residuals_reference(*frames[0], *frames[k], labels, T, tan_half_fovh(s), s.params.k_photometric_res, True)
    full = run(np.zeros((120, 160), np.int64))
    t = full["terms"]
    lost = np.where(full["counted"], t - np.floor(t * 2.0 ** 20) / 2.0 ** 20, 0.0)
    lost[2:-2, 2:-2][~(full["counted"][2:-2, 2:-2])] = 0.0
    # candidates: the largest losses; the one whose single-pixel cluster has the tightest bound
    best = None
    for flat in np.argsort(lost.ravel())[-12:]:
        v, u = np.unravel_index(flat, lost.shape)
        labels = np.full((120, 160), E.N_LABELS, np.int64)
        labels[v, u] = 0
        one = run(labels)
        if one["c"][0] == 1 and one["c_min"][0] == one["c_max"][0] == 1:
            margin = lost[v, u] / 4.0 - one["bound"]["integer"][0]
            if best is None or margin > best[0]:
                best = (margin, one, lost[v, u])
    assert best is not None
    _, one, loss = best
    _verdicts("2^-20 term, cluster of one pixel", one, 0, (one["sum_abs"][0] - loss) / 4.0, True, True)
    bad = (full["sum_abs"][0] - lost.max()) / (2.0 * (full["c"][0] + 1))
    assert not rejected(full, 0, bad, "integer"), "the bound of a cluster of 19000 pixels now sees one truncated term: update the docstring"


# ------------------------------------------------------------------------------------------------------------------------------
#  GPU part
# ------------------------------------------------------------------------------------------------------------------------------
from test_exact_linearisation import ro  # noqa: E402,F401  (the reference-order library bound to the throughput / latency build)


def hip_scene(api, kind, name):
    tally, _, s, _ = drive(api, kind, name)
    rows, cols = SCENES[name][:2]
    if kind in PRODUCT and rows * cols <= ORDERED_MAX_PIXELS:
        # at most 2048 pixels: one workgroup per stream sums level 0 in the reference's order, a cluster of workgroups in fixed point
        G = s.variant()[2]
        assert path_of(s, kind) == ("ordered+integer" if G == 1 else "integer") and (G == 1) == (kind != "cluster"), (kind, G)
        print("ordered_fallbacks %d" % s.ordered_fallbacks())
    conclude(name, kind, tally)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_hip_residuals_against_exact_references(hip, name):
    hip_scene(hip, hip.default_variant, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_reference_order_residuals_against_exact_references(ro, name):
    hip_scene(ro, "reforder", name)


def batched_launch(api, kind):
    """frames 0 .. 6 of one pair in ONE launch (sf_process_frames) against the same frames call by call: the final residuals bit
    for bit, and against the reference (the image pushed five frames ago is the current one: the chain of five poses warps it)"""
    name, n = "moving_sphere_120x160", 7
    rows, cols, mk, _, _ = SCENES[name]
    frames = frames_of(name)
    runs = []
    for many in (False, True):
        s = make_solver(api, rows, cols, mk(api))
        s.set_prediction(0, *frames[0])
        s.set_current(0, *frames[1])
        if many:
            traj = s.process_frames(0, n, trajectory=True)
            Ts = {k: traj[k, 0].astype(np.float32) for k in range(n)}
        else:
            Ts = {}
            for k in range(n):
                s.process_frame(k)
                Ts[k] = s.T()
        runs.append((s, Ts))
    (one, Ts_one), (many, Ts_many) = runs
    assert all(np.array_equal(Ts_one[k], Ts_many[k]) for k in range(n))
    assert np.array_equal(one.cluster_residuals(), many.cluster_residuals(), equal_nan=True) and np.array_equal(one.b_image(), many.b_image())
    tally = {}
    check_frame(many, kind, frames[1], frames[1], Ts_many, n - 1, tally)
    print("batched launch %s: max |got - exact| / bound %.3g" % (kind, tally["ratio"]))


def test_oracle_batched_launch(ora):
    batched_launch(ora, "oracle")


@pytest.mark.gpu
def test_hip_batched_launch(hip):
    batched_launch(hip, hip.default_variant)


@pytest.mark.gpu
def test_hip_separate_entry_points(hip):
    """push_history(k) and residuals_vs_history(k) as calls of their own: stage_push_history copies the images into the ring
    (copy_images = true) instead of the residual pass; the ring filled that way gives the same residuals bit for bit, and they are
    checked against the reference"""
    kind = hip.default_variant
    fused, split = (drive(hip, kind, "odd_40x42", fused=f) for f in (True, False))
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(fused[1], split[1]))
    conclude("odd_40x42 call by call", kind, split[0])


@pytest.mark.gpu
def test_reference_order_separate_entry_points(ro):
    fused, split = (drive(ro, "reforder", "odd_40x42", fused=f) for f in (True, False))
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(fused[1], split[1]))


def eight_streams(api, kind):
    rows, cols, B, k_last = 120, 160, 8, 5
    seqs = [_walk(500 + b, rows, cols, k_last + 1, tuple(np.array(XI_WALK) * (0.6 + 0.1 * b)), (0.01 * b, 0, 0), _ripple(0.2, 20.0)) for b in range(B)]
    s = make_solver(api, rows, cols, driver_params(api, kb=1.5), batch=B)
    for b in range(B):
        s.set_current(b, *seqs[b][0])
    s.current_to_prediction()
    s.push_history(0)
    Ts = [{0: s.T(b)} for b in range(B)]
    for k in range(1, k_last + 1):
        for b in range(B):
            s.set_prediction(b, *seqs[b][k - 1])
            s.set_current(b, *seqs[b][k])
        s.process_frame(k)
        for b in range(B):
            Ts[b][k] = s.T(b)
    tally = {}
    for b in range(B):
        check_frame(s, kind, seqs[b][0], seqs[b][k_last], Ts[b], k_last, tally, stream=b)
    assert len({s.cluster_residuals(b).tobytes() for b in range(B)}) == B, "the streams did not get different inputs"
    print("eight streams %s: %d clusters, %d not sensitive, max |got - exact| / bound %.3g" % (kind, tally["clusters"], tally["weak"], tally["ratio"]))


def test_oracle_eight_streams(ora):
    eight_streams(ora, "oracle")


@pytest.mark.gpu
def test_hip_eight_streams_in_one_handle(hip):
    eight_streams(hip, hip.default_variant)
