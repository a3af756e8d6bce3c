"""The walk the end-to-end test of the bounded maps runs on the GPU (tests/test_gpu_map_window.py), pinned on the CPU oracle:
the camera of test_map_fusion.py's capacity test turns 0.12 rad per frame in front of the QVGA room, the map has room for
80 000 surfels. Unfiltered, the third fuse overflows it. With everything the camera has not seen for more than one tick
dropped before every fuse (here: download, NumPy, upload -- the route sfw_cull_maps replaces) the map stays inside its budget.
The GPU test's premise is checked where it can be."""
import numpy as np

from staticfusion_amd import SfError, SurfelMap
from staticfusion_amd.synth import se3_exp
from conftest import driver_params, make_solver
from test_map_fusion import COLS, ROWS, load_view
from test_model_prediction import synthetic_view

TURN = np.array([0.0, 0.0, 0.0, 0.0, 0.12, 0.0])
CAPACITY = 80000
FRAMES = 5
MAX_AGE = 1


def age_mask(surfels, tick, max_age):
    """test B of include/sf_map_window.h in fp32: (float)tick - s[7] <= (float)max_age"""
    return (np.float32(tick) - surfels[:, 7].astype(np.float32)) <= np.float32(max_age)


def numpy_age_cull(m):
    info, s = m.info(), m.download()
    m.upload(s[age_mask(s, info["tick"], MAX_AGE)], info["pose"], info["tick"])


def turn_walk(api, cull=None, n_frames=FRAMES, capacity=CAPACITY, images=True):
    """the walk; cull(map) runs before every fuse from the second frame on. Per frame: info, surfels, err and, with
    `images`, the index image and the prediction."""
    s = make_solver(api, ROWS, COLS, driver_params(api))
    m = SurfelMap(s, capacity)
    b = np.full(24, 0.9, np.float32)
    T = np.eye(4)
    out = []
    for k in range(n_frames):
        depth, rgb = synthetic_view(T, sphere=False)
        load_view(s, depth, rgb, b)
        if k and cull is not None:
            cull(m)
        err = None
        try:
            m.fuse_frame(0, None if k == 0 else se3_exp(TURN))
        except SfError as e:
            err = str(e)
        o = dict(info=m.info(), surfels=m.download(), err=err)
        if images:
            m.predict(0)
            o.update(index=m.index_map() if k else None, pred=s.prediction())
        out.append(o)
        T = T @ se3_exp(TURN)
    m.close()
    s.close()
    return out


def test_the_age_window_keeps_the_turning_walk_inside_its_capacity(ora):
    plain = turn_walk(ora, None, images=False)
    counts = [o["info"]["count"] for o in plain]
    assert counts[0] == ROWS * COLS and counts[0] < counts[1] < CAPACITY and all(c <= CAPACITY for c in counts)
    assert plain[0]["err"] is None and plain[1]["err"] is None
    assert plain[2]["err"] is not None and "capacity" in plain[2]["err"] and counts[2] == CAPACITY  # truncated
    assert all(o["err"] is not None for o in plain[2:])  # and every later fuse does the same

    windowed = turn_walk(ora, numpy_age_cull, images=False)
    counts = [o["info"]["count"] for o in windowed]
    assert all(o["err"] is None for o in windowed)
    # (this oracle: 76 800, 79 195, 23 198, 23 308, 23 574 -- the peak is the second frame, before the window first bites)
    assert counts[:2] == [o["info"]["count"] for o in plain[:2]] and max(counts) == counts[1] < CAPACITY
    assert all(c < CAPACITY // 2 for c in counts[2:])
    # the window did drop something, and what is left is what the camera saw during the last two ticks
    for o in windowed[2:]:
        assert np.all(o["info"]["tick"] - o["surfels"][:, 7] <= MAX_AGE + 1)
