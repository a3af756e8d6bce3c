"""Frames for the region tests (tests/test_regions_reference_cpu.py, tests/test_gpu_regions.py): (depth, b) pairs of
(rows, cols) float32 images, each a function of its size (and a seed) alone."""
import numpy as np

F = np.float32
RANDOM_B_MAX = 0.7  # the b_max the random three-level frame is labelled with
RANDOM_SEED = 7    # at 37 x 53 this seed has 454 components under connectivity 4 and 268 under 8


def hand_frame():
    """the 4 x 5 frame of the first hand case"""
    inf = np.inf
    z = np.array([[1.00, 1.04, 1.08, 0, 2.0], [1.00, 0, 1.12, 0, 2.0], [0, 0, 1.16, 0, 2.2], [3.0, 3.0, 0, 0, inf]], F)
    b = np.zeros((4, 5), F)
    b[3, 1] = np.nan
    b[0, 4] = 0.5
    return z, b


def random_levels(rows, cols, seed=RANDOM_SEED):
    """55 % filled with the depths 1.0, 1.03 (linked to 1.0) and 2.0 (not linked), random b: label with b_max 0.7"""
    rng = np.random.default_rng(seed)
    filled = rng.random((rows, cols)) < 0.55
    z = np.array([1.0, 1.03, 2.0], F)[rng.integers(0, 3, (rows, cols))]
    return np.where(filled, z, F(0)).astype(F), rng.random((rows, cols)).astype(F)


def checkerboard(rows, cols):
    v, u = np.mgrid[0:rows, 0:cols]
    return np.where((v + u) % 2 == 0, F(1), F(0)).astype(F), np.zeros((rows, cols), F)


def one_component(rows, cols):
    return np.full((rows, cols), 1.5, F), np.zeros((rows, cols), F)


def empty(rows, cols):
    return np.zeros((rows, cols), F), np.zeros((rows, cols), F)


def _along(path, rows, cols):
    """depth 1 m at the start of a path of pixels, rising by at most 2 cm a step and by 2 m in all when it is long enough"""
    z = np.zeros((rows, cols), F)
    step = min(0.02, 2.0 / max(len(path), 1))
    for t, (v, u) in enumerate(path):
        z[v, u] = 1.0 + step * t
    return z, np.zeros((rows, cols), F)


def serpentine(rows, cols):
    """one pixel wide: every second column top to bottom, joined in turn at the bottom and at the top"""
    path = []
    for k, u in enumerate(range(0, cols, 2)):
        col = list(range(rows)) if k % 2 == 0 else list(range(rows - 1, -1, -1))
        path += [(v, u) for v in col]
        if u + 2 < cols:
            path.append((col[-1], u + 1))
    return _along(path, rows, cols)


def spiral(rows, cols):
    """one pixel wide with a gap of one pixel between its arms, from the middle outwards: depth 1 m lies in the middle, and
    pixel 0, the first of the component, is the last of the path"""
    seen = np.zeros((rows, cols), bool)
    dirs = [(0, 1), (1, 0), (0, -1), (-1, 0)]
    v, u, d = 0, 0, 0
    path = [(0, 0)]
    seen[0, 0] = True

    def free(a, c):
        return 0 <= a < rows and 0 <= c < cols and not seen[a, c]

    def may(a, c, dd):  # the next pixel is free and so is the one behind it (or that one is outside)
        dv, du = dirs[dd]
        n1, n2 = (a + dv, c + du), (a + 2 * dv, c + 2 * du)
        return free(*n1) and (free(*n2) or not (0 <= n2[0] < rows and 0 <= n2[1] < cols))

    while True:
        if not may(v, u, d):
            d = (d + 1) % 4
            if not may(v, u, d):
                break
        v, u = v + dirs[d][0], u + dirs[d][1]
        seen[v, u] = True
        path.append((v, u))
    return _along(path[::-1], rows, cols)


def u_shape(rows, cols):
    """two bars down the first and the last column, joined along the last row"""
    path = [(v, 0) for v in range(rows)] + [(rows - 1, u) for u in range(1, cols)] + [(v, cols - 1) for v in range(rows - 2, -1, -1)]
    return _along(list(dict.fromkeys(path)), rows, cols)


DEPTHS = [np.nan, np.inf, -np.inf, 0.0, -1.0, 1.0, 1.02, 8.0, 8.5, 2.0, 1.04]  # 8.0 is z_max itself
WEIGHTS = [np.nan, -0.5, 0.2, 0.5, 1.5, 0.1, np.inf, -np.inf, 0.45]            # 0.5 is b_max itself


def special(rows, cols, seed=0):
    """NaN, +-inf, 0 and negative depth, depth at and beyond z_max; NaN, out-of-range and limit-valued b: by position, with
    two periods that share no factor"""
    i = np.arange(rows * cols) + seed
    z = np.array(DEPTHS, F)[(i * 3) % len(DEPTHS)].reshape(cols, rows).T
    b = np.array(WEIGHTS, F)[(i * 2) % len(WEIGHTS)].reshape(cols, rows).T
    return np.ascontiguousarray(z), np.ascontiguousarray(b)


def frames_of(rows, cols):
    """name -> (depth, b, b_max): the frames every shape of the GPU tests gets"""
    return {"random": random_levels(rows, cols) + (RANDOM_B_MAX,), "checkerboard": checkerboard(rows, cols) + (0.5,),
            "one": one_component(rows, cols) + (0.5,), "empty": empty(rows, cols) + (0.5,), "serpentine": serpentine(rows, cols) + (0.5,),
            "spiral": spiral(rows, cols) + (0.5,), "special": special(rows, cols) + (0.5,)}
