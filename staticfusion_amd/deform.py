"""Deformation graphs: surfel maps bent by the nodes of a graph -- bind, solve, apply (include/sf_deform.h, symbols ``sfd_*``).

The functions here take `SurfelMap` objects, as `join.py` does. Like the symbols of the other companion modules, the ``sfd_*``
symbols are not part of the ABI of include/sf.h -- the CPU oracle does not have them -- so they have a table of their own, bound
to the HIP library a map's solver was created from (the very ``ctypes.CDLL`` object of its `Api`). Nothing here computes anything.

Node positions are (G, 3) float32 arrays, times (G,), transforms (G, 3, 4) row-major ``[A | t]``; poses are 4x4 (row, col)
arrays as everywhere in this package, and the library gets them column-major.
"""
import ctypes as C

import numpy as np

from ._capi import SfError
from ._companion import HandleChild, binder, map_array, one_solver

_H = C.c_void_p
_pp = C.POINTER(C.c_void_p)
_ip = C.POINTER(C.c_int32)
_fp = C.POINTER(C.c_float)

MAX_NODES = 1024        # SFD_MAX_NODES
SOLVE_MAX_NODES = 256   # SFD_SOLVE_MAX_NODES
MAX_ITERATIONS = 32     # SFD_MAX_ITERATIONS
OK, DEGENERATE = 0, 2   # SFD_OK, SFD_DEGENERATE


class SfdParams(C.Structure):
    """struct sfd_params of include/sf_deform.h"""

    _fields_ = [("time_window", C.c_float), ("reserved", C.c_int32 * 7)]


class SfdCounts(C.Structure):
    """struct sfd_counts of include/sf_deform.h"""

    _fields_ = [("n_surfels", C.c_int32), ("n_bound", C.c_int32), ("n_unbound", C.c_int32), ("n_short", C.c_int32), ("reserved", C.c_int32 * 4)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in COUNT_FIELDS}


COUNT_FIELDS = ("n_surfels", "n_bound", "n_unbound", "n_short")


class SfdInfo(C.Structure):
    """struct sfd_info of include/sf_deform.h"""

    _fields_ = [("max_nodes", C.c_int32), ("n_nodes", C.c_int32), ("reserved", C.c_int32 * 2)]


class SfdConstraint(C.Structure):
    """struct sfd_constraint of include/sf_deform.h"""

    _fields_ = [("src", C.c_float * 3), ("dst", C.c_float * 3), ("time", C.c_float), ("weight", C.c_float)]


class SfdSolveParams(C.Structure):
    """struct sfd_solve_params of include/sf_deform.h"""

    _fields_ = [("time_window", C.c_float), ("w_reg", C.c_float), ("damping", C.c_float), ("iterations", C.c_int32), ("reserved", C.c_int32 * 4)]


class SfdReport(C.Structure):
    """struct sfd_report of include/sf_deform.h"""

    _fields_ = [("status", C.c_int32), ("iterations_done", C.c_int32), ("n_bound", C.c_int32), ("n_unbound", C.c_int32), ("energy", C.c_double * 33)]


_sp, _op, _np, _cp, _vp, _rp = (C.POINTER(t) for t in (SfdParams, SfdCounts, SfdInfo, SfdConstraint, SfdSolveParams, SfdReport))

# name -> (restype, argtypes); every function include/sf_deform.h declares
SIGNATURES = {
    "sfd_version": (C.c_int, []),
    "sfd_params_bytes": (C.c_size_t, []),
    "sfd_counts_bytes": (C.c_size_t, []),
    "sfd_info_bytes": (C.c_size_t, []),
    "sfd_constraint_bytes": (C.c_size_t, []),
    "sfd_solve_params_bytes": (C.c_size_t, []),
    "sfd_report_bytes": (C.c_size_t, []),
    "sfd_default_params": (C.c_int, [_sp]),
    "sfd_default_solve_params": (C.c_int, [_vp]),
    "sfd_check_params": (C.c_int, [_sp]),
    "sfd_check_solve_params": (C.c_int, [_vp]),
    "sfd_graph_create": (C.c_int, [_H, C.c_int, _pp]),
    "sfd_graph_destroy": (None, [_H]),
    "sfd_graph_info": (C.c_int, [_H, _np]),
    "sfd_graph_set": (C.c_int, [_H, C.c_int, _fp, _fp, _fp]),
    "sfd_graph_get": (C.c_int, [_H, _fp, _fp, _fp]),
    "sfd_sample_nodes": (C.c_int, [_H, C.c_float, C.c_int, _fp, _fp, _ip]),
    "sfd_bind_point": (C.c_int, [C.c_int, _fp, _fp, C.c_float, _fp, C.c_float, _ip, _fp]),
    "sfd_deform_surfel": (C.c_int, [C.c_int, _fp, _fp, _fp, C.c_float, _fp, _fp]),
    "sfd_edges": (C.c_int, [C.c_int, _fp, _fp, C.c_float, _ip]),
    "sfd_deform_poses": (C.c_int, [C.c_int, _fp, _fp, _fp, C.c_float, C.c_int, _fp, _fp, _fp]),
    "sfd_bind_maps": (C.c_int, [_H, C.c_int, _pp, _pp, _sp, _ip, _fp]),
    "sfd_apply_maps": (C.c_int, [_H, C.c_int, _pp, _pp, _sp, _op]),
    "sfd_solve": (C.c_int, [C.c_int, _fp, _fp, C.c_int, _cp, _vp, _fp, _rp]),
}

VERSION = 1  # sfd_version() of the header this table restates
INF = float("inf")


def Params(time_window=INF):
    """a sfd_params; the defaults are those of sfd_default_params: parameter defaults, not tuned values"""
    return SfdParams(float(time_window), (C.c_int32 * 7)())


def SolveParams(time_window=INF, w_reg=1.0, damping=1e-6, iterations=8):
    """a sfd_solve_params; the defaults are those of sfd_default_solve_params: parameter defaults, not tuned values"""
    return SfdSolveParams(float(time_window), float(w_reg), float(damping), int(iterations), (C.c_int32 * 4)())


_bind, _product = binder("sfd_", "deformation graphs are", SIGNATURES, VERSION,
                         [("params_bytes", "sfd_params", C.sizeof(SfdParams)), ("counts_bytes", "sfd_counts", C.sizeof(SfdCounts)),
                          ("info_bytes", "sfd_info", C.sizeof(SfdInfo)), ("constraint_bytes", "sfd_constraint", C.sizeof(SfdConstraint)),
                          ("solve_params_bytes", "sfd_solve_params", C.sizeof(SfdSolveParams)), ("report_bytes", "sfd_report", C.sizeof(SfdReport))])


def version():
    return _product().version()


def default_params():
    b = _product()
    p = SfdParams()
    b.check(b.default_params(C.byref(p)), "default_params")
    return p


def default_solve_params():
    b = _product()
    p = SfdSolveParams()
    b.check(b.default_solve_params(C.byref(p)), "default_solve_params")
    return p


def check_params(p):
    """raises SfError for parameters the library refuses (pure host: no handle, no GPU)"""
    b = _product()
    b.check(b.check_params(C.byref(p)), "check_params")


def check_solve_params(p):
    b = _product()
    b.check(b.check_solve_params(C.byref(p)), "check_solve_params")


def _f(a, shape):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(shape))


def _nodes(pos, times, M=None):
    """(G, pos, times, M or None) as contiguous float32 arrays"""
    pos = _f(pos, (-1, 3))
    G = pos.shape[0]
    times = _f(times, (-1,))
    if times.shape[0] != G:
        raise SfError("%d node positions and %d times" % (G, times.shape[0]))
    if M is not None:
        M = _f(M, (-1, 3, 4))
        if M.shape[0] != G:
            raise SfError("%d node positions and %d transforms" % (G, M.shape[0]))
    return G, pos, times, M


def _p(a):
    return None if a is None else a.ctypes.data_as(_fp)


class Graph(HandleChild):
    """one sfd_graph on a solver's handle: `set(pos, times, M=None)`, `get()`, `info()`, `close()`"""

    _ptr, _destroy = "g", "graph_destroy"

    def __init__(self, solver, max_nodes=MAX_NODES):
        super().__init__(solver, _bind(solver.api))
        self.b.check(self.b.graph_create(solver.h, int(max_nodes), C.byref(self.g)), "graph_create")

    def info(self):
        i = SfdInfo()
        self.b.check(self.b.graph_info(self.g, C.byref(i)), "graph_info")
        return dict(max_nodes=int(i.max_nodes), n_nodes=int(i.n_nodes))

    def set(self, pos, times, M=None):
        G, pos, times, M = _nodes(pos, times, M)
        self.b.check(self.b.graph_set(self.g, G, _p(pos), _p(times), _p(M)), "graph_set")

    def get(self):
        G = self.info()["n_nodes"]
        pos, times, M = np.zeros((max(G, 1), 3), np.float32), np.zeros(max(G, 1), np.float32), np.zeros((max(G, 1), 3, 4), np.float32)
        self.b.check(self.b.graph_get(self.g, _p(pos), _p(times), _p(M)), "graph_get")
        return pos[:G].copy(), times[:G].copy(), M[:G].copy()


def sample_nodes(surfel_map, spacing, max_nodes=MAX_NODES):
    """sfd_sample_nodes: (positions (k, 3), init times (k,)) of the most confident surfel of every voxel of edge `spacing`, in
    surfel order; SfError when there are more than max_nodes (the message has the count)"""
    b = _bind(surfel_map.api)
    pos, times = np.zeros((max(int(max_nodes), 1), 3), np.float32), np.zeros(max(int(max_nodes), 1), np.float32)
    k = C.c_int32(0)
    b.check(b.sample_nodes(surfel_map.m, C.c_float(float(spacing)), int(max_nodes), _p(pos), _p(times), C.byref(k)), "sample_nodes")
    return pos[:k.value].copy(), times[:k.value].copy()


def bind_point(pos, times, p, tau, time_window=INF):
    """sfd_bind_point (pure host): (m, indices (4,), weights (4,))"""
    b = _product()
    G, pos, times, _ = _nodes(pos, times)
    idx, w = np.zeros(4, np.int32), np.zeros(4, np.float32)
    m = b.bind_point(G, _p(pos), _p(times), C.c_float(float(time_window)), _p(_f(p, (3,))), C.c_float(float(tau)), idx.ctypes.data_as(_ip), _p(w))
    if m < 0:
        b.check(m, "bind_point")
    return int(m), idx, w


def deform_surfel(pos, times, M, s, time_window=INF):
    """sfd_deform_surfel (pure host): (m, the 12 floats of the deformed surfel)"""
    b = _product()
    G, pos, times, M = _nodes(pos, times, M)
    out = np.zeros(12, np.float32)
    m = b.deform_surfel(G, _p(pos), _p(times), _p(M), C.c_float(float(time_window)), _p(_f(s, (12,))), _p(out))
    if m < 0:
        b.check(m, "deform_surfel")
    return int(m), out


def edges(pos, times, time_window=INF):
    """sfd_edges (pure host): (G, 4) int32, -1 for a missing edge"""
    b = _product()
    G, pos, times, _ = _nodes(pos, times)
    out = np.zeros((max(G, 1), 4), np.int32)
    b.check(b.edges(G, _p(pos), _p(times), C.c_float(float(time_window)), out.ctypes.data_as(_ip)), "edges")
    return out[:G].copy()


def deform_poses(pos, times, M, poses, taus, time_window=INF):
    """sfd_deform_poses (pure host): n poses (4x4 (row, col)) with their times under the graph, as (n, 4, 4)"""
    b = _product()
    G, pos, times, M = _nodes(pos, times, M)
    P = np.asarray(poses, np.float32).reshape(-1, 4, 4)
    n = P.shape[0]
    cm = np.ascontiguousarray(np.transpose(P, (0, 2, 1))).reshape(-1)  # column-major
    t = _f(taus, (-1,))
    if t.shape[0] != n:
        raise SfError("%d poses and %d times" % (n, t.shape[0]))
    out = np.zeros(max(n, 1) * 16, np.float32)
    b.check(b.deform_poses(G, _p(pos), _p(times), _p(M), C.c_float(float(time_window)), n, _p(cm), _p(t), _p(out)), "deform_poses")
    return np.transpose(out[:n * 16].reshape(n, 4, 4), (0, 2, 1)).copy()


def _call(maps, graphs, params):
    maps = list(maps)
    n = len(maps)
    one_solver(maps)
    graphs = [graphs] * n if isinstance(graphs, Graph) else list(graphs)
    if len(graphs) != n:
        raise SfError("%d maps and %d graphs" % (n, len(graphs)))
    params = Params() if params is None else params
    params = [params] * n if isinstance(params, SfdParams) else list(params)
    if len(params) != n:
        raise SfError("%d maps and %d parameter sets" % (n, len(params)))
    garr = (C.c_void_p * max(n, 1))(*[g.g.value for g in graphs])
    return maps, n, garr, (SfdParams * max(n, 1))(*params)


def bind_maps(maps, graphs, params=None):
    """sfd_bind_maps: per map (indices (count, 4) int32, weights (count, 4) float32) of its surfels under graphs[q] (one Graph
    serves every map); no map changes"""
    maps, n, garr, pr = _call(maps, graphs, params)
    if n == 0:
        return []
    counts = [m.info()["count"] for m in maps]
    total = sum(counts)
    idx, w = np.zeros((max(total, 1), 4), np.int32), np.zeros((max(total, 1), 4), np.float32)
    b = _bind(maps[0].api)
    b.check(b.bind_maps(maps[0].solver.h, n, map_array(maps), garr, pr, idx.ctypes.data_as(_ip), _p(w)), "bind_maps")
    out, first = [], 0
    for k in counts:
        out.append((idx[first:first + k].copy(), w[first:first + k].copy()))
        first += k
    return out


def apply_maps(maps, graphs, params=None):
    """sfd_apply_maps: every surfel of maps[q] deformed under graphs[q] in place. Returns the counts, one dict per map."""
    maps, n, garr, pr = _call(maps, graphs, params)
    if n == 0:
        return []
    out = (SfdCounts * n)()
    b = _bind(maps[0].api)
    b.check(b.apply_maps(maps[0].solver.h, n, map_array(maps), garr, pr, out), "apply_maps")
    return [c.as_dict() for c in out]


def constraints(src, dst, times, weights=1.0):
    """an array of sfd_constraint from (C, 3) sources and destinations, times and weights (scalars are repeated)"""
    src, dst = _f(src, (-1, 3)), _f(dst, (-1, 3))
    n = src.shape[0]
    t = np.broadcast_to(np.asarray(times, np.float32), (n,))
    w = np.broadcast_to(np.asarray(weights, np.float32), (n,))
    out = (SfdConstraint * max(n, 1))()
    for c in range(n):
        out[c] = SfdConstraint((C.c_float * 3)(*src[c]), (C.c_float * 3)(*dst[c]), float(t[c]), float(w[c]))
    return out, n


def solve(pos, times, src, dst, con_times, weights=1.0, M=None, params=None):
    """sfd_solve (pure host): (M (G, 3, 4), report dict(status, iterations_done, n_bound, n_unbound, energy (iterations_done + 1,)))
    from constraints src -> dst; M: the transforms to start from (None: identities)"""
    b = _product()
    G, pos, times, M = _nodes(pos, times, M)
    if M is None:
        M = np.ascontiguousarray(np.tile(np.eye(3, 4, dtype=np.float32), (G, 1, 1)))
    else:
        M = M.copy()
    cons, n = constraints(src, dst, con_times, weights)
    p = SolveParams() if params is None else params
    r = SfdReport()
    b.check(b.solve(G, _p(pos), _p(times), n, cons, C.byref(p), _p(M), C.byref(r)), "solve")
    return M, dict(status=int(r.status), iterations_done=int(r.iterations_done), n_bound=int(r.n_bound), n_unbound=int(r.n_unbound),
                   energy=np.array(r.energy[:r.iterations_done + 1], np.float64))
