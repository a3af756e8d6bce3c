"""Surfel maps carved by what later frames saw through them (include/sf_carve.h, symbols ``sfe_*``).

`Carver(solver).carve(maps, params, entries)` takes `SurfelMap` objects, one `SfeParams` per map (or one for all) and entries
``(map index, view, frame)``, where a frame is a stream index of the solver or a (rows, cols) float32 depth image, and returns
one dict of counts per map (with ``votes=True`` also the packed vote words per map). Like the symbols of the other companion
modules, the ``sfe_*`` symbols are not part of the ABI of include/sf.h -- the CPU oracle does not have them -- so they have a
table of their own, bound to the HIP library a solver was created from (the very ``ctypes.CDLL`` object of its `Api`). Nothing
here computes anything.
"""
import ctypes as C

import numpy as np

from ._capi import SfError
from ._companion import HandleChild, binder, map_array, one_solver, ptr_array
from .view import SfvView

_H = C.c_void_p
_pp = C.POINTER(C.c_void_p)
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)
_vp = C.POINTER(SfvView)

MAX_WINDOW = 3  # SFE_MAX_WINDOW
# SFE_CLASS_*: what `observe` returns
CLASS_UNSEEN, CLASS_THROUGH, CLASS_SUPPORTED, CLASS_OCCLUDED = range(4)


class SfeParams(C.Structure):
    """struct sfe_params of include/sf_carve.h"""

    _fields_ = [("tol_abs", C.c_float), ("tol_rel", C.c_float), ("z_max", C.c_float), ("min_cos", C.c_float), ("window", C.c_int32),
                ("min_pixels", C.c_int32), ("min_votes", C.c_int32), ("max_support", C.c_int32), ("dry_run", C.c_int32), ("reserved", C.c_int32 * 3)]


class SfeCounts(C.Structure):
    """struct sfe_counts of include/sf_carve.h"""

    _fields_ = [("n_in", C.c_int32), ("n_judged", C.c_int32), ("n_through", C.c_int32), ("n_supported", C.c_int32), ("n_occluded", C.c_int32),
                ("n_carved", C.c_int32), ("n_out", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in COUNT_FIELDS}


COUNT_FIELDS = ("n_in", "n_judged", "n_through", "n_supported", "n_occluded", "n_carved", "n_out")

_sp, _op = C.POINTER(SfeParams), C.POINTER(SfeCounts)

# name -> (restype, argtypes); every function include/sf_carve.h declares
SIGNATURES = {
    "sfe_version": (C.c_int, []),
    "sfe_params_bytes": (C.c_size_t, []),
    "sfe_counts_bytes": (C.c_size_t, []),
    "sfe_default_params": (C.c_int, [_sp]),
    "sfe_check_params": (C.c_int, [_sp]),
    "sfe_observe": (C.c_int, [_fp, C.c_int, _vp, _fp, _sp, _ip]),
    "sfe_decide": (C.c_int, [C.c_int, C.c_int, _sp]),
    "sfe_carver_create": (C.c_int, [_H, _pp]),
    "sfe_carver_destroy": (None, [_H]),
    "sfe_carve_streams": (C.c_int, [_H, C.c_int, _pp, _sp, C.c_int, _ip, _vp, _ip, _op, _pp]),
    "sfe_carve_images": (C.c_int, [_H, C.c_int, _pp, _sp, C.c_int, _ip, _vp, _pp, _op, _pp]),
}

VERSION = 1  # sfe_version() of the header this table restates


def Params(tol_abs=0.02, tol_rel=0.01, z_max=8.0, min_cos=0.2, window=1, min_pixels=5, min_votes=2, max_support=0, dry_run=False):
    """a sfe_params; the defaults are those of sfe_default_params: parameter defaults, not tuned values"""
    return SfeParams(float(tol_abs), float(tol_rel), float(z_max), float(min_cos), int(window), int(min_pixels), int(min_votes), int(max_support), int(dry_run))


_bind, _product = binder("sfe_", "carves are", SIGNATURES, VERSION,
                         [("params_bytes", "sfe_params", C.sizeof(SfeParams)), ("counts_bytes", "sfe_counts", C.sizeof(SfeCounts))])


def version():
    return _product().version()


def default_params():
    b = _product()
    p = SfeParams()
    b.check(b.default_params(C.byref(p)), "default_params")
    return p


def check_params(p):
    """raises SfError for parameters the library refuses (pure host: no handle, no GPU)"""
    b = _product()
    b.check(b.check_params(C.byref(p)), "check_params")


def _column_major(image, view):
    a = np.asarray(image, np.float32)
    if a.shape != (view.rows, view.cols):
        raise SfError("depth image of shape %r for a view of %d x %d" % (a.shape, view.rows, view.cols))
    return np.ascontiguousarray(a.T)


def observe(surfel, tick, view, depth, params=None):
    """sfe_observe (pure host): (class, (through, near, front)) of one surfel (12 floats) of a map at `tick` against `view`
    and the (rows, cols) depth image `depth`"""
    b = _product()
    s = np.ascontiguousarray(np.asarray(surfel, np.float32).reshape(12))
    d = _column_major(depth, view)
    found = (C.c_int32 * 3)()
    p = Params() if params is None else params
    cls = b.observe(s.ctypes.data_as(_fp), int(tick), C.byref(view), d.ctypes.data_as(_fp), C.byref(p), found)
    if cls < 0:
        b.check(cls, "observe")
    return int(cls), tuple(int(x) for x in found)


def decide(v_through, v_support, params=None):
    """sfe_decide (pure host): whether a surfel with these votes is carved"""
    b = _product()
    p = Params() if params is None else params
    r = b.decide(int(v_through), int(v_support), C.byref(p))
    if r < 0:
        b.check(r, "decide")
    return bool(r)


class Carver(HandleChild):
    """one sfe_carver on a solver's handle: `carve(maps, params, entries)`, `close()`"""

    _ptr, _destroy = "c", "carver_destroy"

    def __init__(self, solver):
        super().__init__(solver, _bind(solver.api))
        self.b.check(self.b.carver_create(solver.h, C.byref(self.c)), "carver_create")

    def carve(self, maps, params, entries, votes=False):
        """sfe_carve_streams / sfe_carve_images. maps: distinct `SurfelMap`s of the carver's solver; params: one `SfeParams`
        for all maps, a list with one per map, or None for the defaults; entries: (map index, view, frame) triples whose
        frames are either all stream indices (the level-0 depth of that stream, read on the device) or all (rows, cols)
        float32 depth images. Returns one dict of counts per map; with votes=True (counts, [uint32 array per map]), each word
        v_through | v_support << 16 in the map's old order."""
        maps, entries = list(maps), list(entries)
        n_maps, n = len(maps), len(entries)
        one_solver(maps)
        if n_maps and maps[0].solver is not self.solver:
            raise SfError("the maps of a carve belong to the carver's solver")
        params = Params() if params is None else params
        params = [params] * n_maps if isinstance(params, SfeParams) else list(params)
        if len(params) != n_maps:
            raise SfError("%d maps and %d parameter sets" % (n_maps, len(params)))
        if n_maps == 0 and n == 0:
            return ([], []) if votes else []
        streams = [isinstance(e[2], (int, np.integer)) for e in entries]
        if any(streams) and not all(streams):
            raise SfError("the frames of one carve are all streams or all images")
        map_of = (C.c_int32 * max(n, 1))(*[int(e[0]) for e in entries])
        views = (SfvView * max(n, 1))(*[e[1] for e in entries])
        counts = (SfeCounts * max(n_maps, 1))()
        words = [np.zeros(m.info()["count"], np.uint32) for m in maps] if votes else None
        vp = ptr_array([w if w.size else None for w in words], n_maps) if votes and n_maps else None
        head = (self.c, n_maps, map_array(maps), (SfeParams * max(n_maps, 1))(*params), n, map_of, views)
        if n and all(streams):
            code = self.b.carve_streams(*head, (C.c_int32 * n)(*[int(e[2]) for e in entries]), counts, vp)
            what = "carve_streams"
        else:
            frames = [_column_major(e[2], e[1]) for e in entries]
            code = self.b.carve_images(*head, ptr_array(frames, n) if n else None, counts, vp)
            what = "carve_images"
        self.b.check(code, what)
        out = [counts[m].as_dict() for m in range(n_maps)]
        return (out, words) if votes else out
