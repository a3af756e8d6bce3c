"""The restatement of the carve (tests/carve_ref.py) on the scene of tests/carve_cases.py, no GPU: a wall at z = 3, a floor at
y = 1 seen at a grazing angle and a box face at z = 1.6, at 64 x 48 (fx = fy = 52.8, cx = 31.5, cy = 23.5). The map is made from
view A with the box present; the frames are from the three displaced views A, B and E with the box gone, and the same three with
it present. What is asserted are conditions on the REFERENCE ALONE, not measurements: what the rule must do on this scene for
the GPU tests to mean anything. The figures are printed (run with -s) and recorded in DESIGN.md section 34."""
import numpy as np

import carve_cases as cc
import carve_ref as cr

_SCENE = {}


def scene():
    """the map, the kind of every surfel and the six frames, computed once"""
    if not _SCENE:
        views = {k: cc.scene_view(k) for k in "ABE"}
        surf, kind = cc.scene_map(views["A"], cc.scene_depth(views["A"], box=True))
        _SCENE.update(views=views, surf=surf, kind=kind, gone={k: cc.scene_depth(v, box=False) for k, v in views.items()},
                      present={k: cc.scene_depth(v, box=True) for k, v in views.items()})
    return _SCENE


def test_the_scene_is_the_one_described():
    sc = scene()
    kind = sc["kind"]
    assert sc["surf"].shape[0] == kind.shape[0] and (kind == 2).sum() == 208 and (kind == 1).sum() == 384 and (kind == 0).sum() == 64 * 42 - 208
    assert (cc.SCENE["rows"], cc.SCENE["cols"], cc.SCENE["fx"], cc.SCENE["fy"], cc.SCENE["cx"], cc.SCENE["cy"]) == (48, 64, 52.8, 52.8, 31.5, 23.5)
    for k in "ABE":
        assert (sc["gone"][k] > 0).all() and (sc["present"][k] <= sc["gone"][k]).all() and (sc["present"][k] < sc["gone"][k]).sum() > 150, k


def test_with_the_box_gone_exactly_the_box_is_carved():
    sc = scene()
    kind, p = sc["kind"], cc.params()  # the defaults: window 1, min_pixels 5, min_votes 2, max_support 0
    for noise in (0.0, 0.003):
        frames = {k: cc.scene_depth(v, box=False, noise=noise, seed=11) for k, v in sc["views"].items()}
        through = {}
        for k, v in sc["views"].items():
            cls, _ = cr.observe(sc["surf"], cc.TICK, v, frames[k], p)
            through[k] = cls == cr.THROUGH
            assert not through[k][kind != 2].any(), (k, noise)  # no wall or floor surfel is THROUGH in any view
            judged = cls != cr.UNSEEN
            assert (cls[(kind == 2) & judged] == cr.THROUGH).all() and ((kind == 2) & judged).sum() > 150, (k, noise)  # every judged box surfel is
            print("noise %g view %s: box THROUGH %d of %d, floor THROUGH %d, wall THROUGH %d" % (noise, k, through[k][kind == 2].sum(), (kind == 2).sum(),
                                                                                                  through[k][kind == 1].sum(), through[k][kind == 0].sum()))
        res = cr.carve_map(sc["surf"], cc.TICK, p, [(sc["views"][k], frames[k]) for k in "ABE"])
        assert np.array_equal(res["carved"], kind == 2), noise  # with min_votes = 2, exactly the box surfels
        assert res["counts"]["n_carved"] == 208 and res["counts"]["n_out"] == kind.shape[0] - 208 and np.array_equal(res["out"], sc["surf"][kind != 2])
        print("noise %g: counts %r" % (noise, res["counts"]))


def test_the_centre_depth_would_carve_the_floor():
    """why zp is the depth of the pixel's ray on the surfel's plane: with h.z in its place the grazing floor is seen through"""
    sc = scene()
    kind, p = sc["kind"], cc.params()
    wrong = {k: (cr.observe(sc["surf"], cc.TICK, v, sc["gone"][k], p, centre_depth=True)[0] == cr.THROUGH)[kind == 1].sum() for k, v in sc["views"].items()}
    print("floor surfels THROUGH with the centre depth:", wrong)
    assert wrong["B"] > 0 and wrong["E"] > 0


def test_with_the_box_present_nothing_is_carved():
    sc = scene()
    kind, p = sc["kind"], cc.params()
    res = cr.carve_map(sc["surf"], cc.TICK, p, [(sc["views"][k], sc["present"][k]) for k in "ABE"])
    assert not res["carved"].any() and res["out"] is not None and res["counts"]["n_carved"] == 0 and res["counts"]["n_out"] == kind.shape[0]
    box = res["classes"][:, kind == 2]
    assert ((box == cr.SUPPORTED) | (box == cr.UNSEEN)).all() and (box == cr.SUPPORTED).sum() > 3 * 150  # every judged box surfel is SUPPORTED
    assert not (res["classes"] == cr.THROUGH).any()
    print("box present: counts %r" % (res["counts"],))


def test_votes_and_partition_of_the_restatement():
    sc = scene()
    kind = sc["kind"]
    entries = [(sc["views"][k], sc["gone"][k]) for k in "ABE"]
    res = cr.carve_map(sc["surf"], cc.TICK, cc.params(), entries)
    vt, vs = res["votes"] & 0xffff, res["votes"] >> 16
    assert np.array_equal(vt, (res["classes"] == cr.THROUGH).sum(0)) and np.array_equal(vs, (res["classes"] == cr.SUPPORTED).sum(0))
    assert (vt[kind == 2] >= 2).all() and vs.max() <= 3
    dry = cr.carve_map(sc["surf"], cc.TICK, cc.params(dry_run=1), entries)
    assert dry["counts"] == res["counts"] and dry["out"] is not res["out"] and np.array_equal(dry["out"], sc["surf"])
    one = cr.carve_map(sc["surf"], cc.TICK, cc.params(min_votes=1, max_support=3), entries[:1])
    assert one["counts"]["n_carved"] == 208
    none = cr.carve_map(sc["surf"], cc.TICK, cc.params(), [])
    assert none["counts"] == dict(n_in=kind.shape[0], n_judged=0, n_through=0, n_supported=0, n_occluded=0, n_carved=0, n_out=kind.shape[0])
    many = cr.carve([(sc["surf"], cc.TICK), (sc["surf"][kind != 1], cc.TICK)], [cc.params(), cc.params(min_votes=1)],
                    [(1, sc["views"]["B"], sc["gone"]["B"]), (0, sc["views"]["A"], sc["gone"]["A"]), (0, sc["views"]["E"], sc["gone"]["E"])])
    assert many[0]["counts"]["n_carved"] == 208 and many[1]["counts"]["n_carved"] == 208
