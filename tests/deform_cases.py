"""Scene builders for the deformation-graph tests (include/sf_deform.h): graphs on an integer lattice whose query points tie at
every rank, duplicate nodes, nodes with NaN and inf, time windows, random and rigid transforms, surfel sets of a given count,
and the constraint sets of the solver cases."""
import numpy as np

F = np.float32
STEP = 0.5  # lattice spacing in metres: dyadic, so differences and squares of lattice coordinates are exact in fp32


def lattice_nodes(G, times_mod=7):
    """the first G points of a cubic lattice (x fastest), times j % times_mod"""
    k = 1
    while k ** 3 < G:
        k += 1
    j = np.arange(G)
    pos = np.stack([j % k, (j // k) % k, j // (k * k)], axis=1).astype(F) * F(STEP)
    return pos, (j % times_mod).astype(F)


def lattice_queries(G):
    """points on the lattice of lattice_nodes(G): the nodes themselves (d2 == 0), edge midpoints (2 nodes tie), face centres
    (4 tie: the fifth is farther), cell centres (8 tie: fourth against fifth), and points just off them"""
    pos, _ = lattice_nodes(G)
    offs = np.array([[0, 0, 0], [.5, 0, 0], [0, .5, 0], [.5, .5, 0], [0, .5, .5], [.5, .5, .5], [.25, .5, .5], [.5, .5, .375], [.125, .25, .0625]], F) * F(STEP)
    return (pos[:, None, :] + offs[None, :, :]).reshape(-1, 3)


def duplicate_nodes(G, copies=5):
    """a lattice whose first node exists `copies` times (dmax2 == 0 for a query on it) and whose second exists twice"""
    pos, times = lattice_nodes(G)
    pos[:min(copies, G)] = pos[0]
    if G > copies + 1:
        pos[copies + 1] = pos[copies]
    return pos, times


def special_nodes(G):
    """a lattice with a NaN, a +inf and a -inf coordinate, a NaN time and an inf time among its nodes"""
    pos, times = lattice_nodes(G)
    pos, times = pos.copy(), times.copy()
    for j, (c, v) in enumerate([(0, np.nan), (1, np.inf), (2, -np.inf)]):
        if 2 * j + 1 < G:
            pos[2 * j + 1, c] = v
    if G > 8:
        times[6] = np.nan
        times[8] = np.inf
    return pos, times


def random_affine(G, seed, scale=0.2):
    rng = np.random.default_rng(seed)
    M = np.tile(np.eye(3, 4, dtype=F), (G, 1, 1))
    return (M + rng.uniform(-scale, scale, (G, 3, 4))).astype(F)


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def rigid_M(pos, R, t):
    """the node transforms under which every node carries the world motion x -> R x + t: A = R, t_j = R g_j + t - g_j"""
    pos = np.asarray(pos, np.float64)
    M = np.zeros((pos.shape[0], 3, 4))
    M[:, :, :3] = R
    M[:, :, 3] = pos @ R.T + t - pos
    return M.astype(F)


def surfels(n, seed, lo=-0.5, hi=2.5, times_mod=7, queries=None):
    """n surfels: the rows of `queries` (positions) first, as far as they reach, then random positions in the box; unit normals,
    init times k % times_mod, a few confidences"""
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 12), F)
    s[:, 0:3] = rng.uniform(lo, hi, (n, 3))
    if queries is not None:
        k = min(n, queries.shape[0])
        s[:k, 0:3] = queries[:k]
    s[:, 3] = rng.choice(np.array([0.1, 0.5, 0.9, 1.0], F), n)
    s[:, 4] = rng.integers(0, 1 << 24, n).astype(F)
    s[:, 5] = rng.integers(1, 30, n).astype(F)
    s[:, 6] = (np.arange(n) % times_mod).astype(F)
    s[:, 7] = s[:, 6] + 3
    nrm = rng.normal(size=(n, 3))
    s[:, 8:11] = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    s[:, 11] = rng.uniform(0.002, 0.02, n)
    return np.ascontiguousarray(s, F)


def graph_scene(G, seed):
    """(pos, times, M) for a GPU case: a lattice graph with duplicates and special values when it is large enough"""
    pos, times = duplicate_nodes(G) if G >= 5 else lattice_nodes(G)
    if G >= 65:
        sp, st = special_nodes(G)
        pos[40:60], times[40:60] = sp[1:21], st[1:21]
    return pos, times, random_affine(G, seed)


# ---- the solver cases -------------------------------------------------------------------------------------------------------
def plane_nodes(k=5, spacing=0.25):
    """k x k nodes on the plane z = 1, time 0"""
    u, v = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
    pos = np.stack([u.ravel() * spacing, v.ravel() * spacing, np.ones(k * k)], axis=1).astype(F)
    return pos, np.zeros(k * k, F)


def plane_pull(k=5, spacing=0.25, pull=0.05):
    """25 nodes on a plane; the points of the edge u = k - 1 pulled by `pull` along z, those of the edge u = 0 pinned"""
    pos, times = plane_nodes(k, spacing)
    far, near = pos[pos[:, 0] == F((k - 1) * spacing)], pos[pos[:, 0] == 0]
    src = np.concatenate([far, near])
    dst = np.concatenate([far + np.array([0, 0, pull], F), near])
    return pos, times, src, dst.astype(F)


def rigid_case(seed=5):
    """12 nodes, 40 constraints that are one rigid motion, no pins: (pos, times, src, dst, R, t)"""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0, 1, (12, 3)).astype(F)
    src = rng.uniform(-0.1, 1.1, (40, 3)).astype(F)
    R, t = rotation([1, 2, -1], 0.12), np.array([0.03, -0.02, 0.05])
    dst = (src.astype(np.float64) @ R.T + t).astype(F)
    return pos, np.zeros(12, F), src, dst, R, t
