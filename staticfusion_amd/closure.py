"""Loop-closure constraints from two sightings of a place, built on the device (include/sf_closure.h, symbols ``sfc_*``).

`Builder(solver).build(...)` takes `SurfelMap` objects and views (`view.View`), as `score.py` does, and returns the records as a
structured array with the fields ``src`` / ``dst`` / ``time`` / ``weight`` -- the point constraints `deform.solve` takes, which
`as_solve_arrays` hands over. Like the symbols of the other companion modules, the ``sfc_*`` symbols are not part of the ABI of
include/sf.h -- the CPU oracle does not have them -- so they have a table of their own, bound to the HIP library a solver was
created from (the very ``ctypes.CDLL`` object of its `Api`). Nothing here computes anything.
"""
import ctypes as C

import numpy as np

from ._capi import SfError
from ._companion import HandleChild, binder, map_array, one_solver
from .view import SfvView

_H = C.c_void_p
_pp = C.POINTER(C.c_void_p)
_fp = C.POINTER(C.c_float)
_vp = C.POINTER(SfvView)

MAX_STRIDE = 4096  # SFC_MAX_STRIDE
# SFC_FOUND_*: the bits `link_sample` returns
FOUND_BOTH, FOUND_NEAR, FOUND_APART, FOUND_LINK, FOUND_PIN, FOUND_LINK_DROPPED, FOUND_PIN_DROPPED = 1, 2, 4, 8, 16, 32, 64

# struct sfc_record of include/sf_closure.h
RECORD = np.dtype([("src", np.float32, 3), ("dst", np.float32, 3), ("time", np.float32), ("weight", np.float32)])


class SfcParams(C.Structure):
    """struct sfc_params of include/sf_closure.h"""

    _fields_ = [("stride", C.c_int32), ("pins", C.c_int32), ("gate_abs", C.c_float), ("gate_rel", C.c_float), ("min_time_gap", C.c_float),
                ("w_link", C.c_float), ("w_pin", C.c_float), ("reserved", C.c_int32)]


class SfcCounts(C.Structure):
    """struct sfc_counts of include/sf_closure.h"""

    _fields_ = [("n_samples", C.c_int32), ("n_new", C.c_int32), ("n_old", C.c_int32), ("n_both", C.c_int32), ("n_near", C.c_int32), ("n_apart", C.c_int32),
                ("n_links", C.c_int32), ("n_pins", C.c_int32), ("n_dropped", C.c_int32), ("first", C.c_int32), ("reserved", C.c_int32 * 2),
                ("sum_dz", C.c_int64), ("sum_shift", C.c_int64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in COUNT_FIELDS}


COUNT_FIELDS = ("n_samples", "n_new", "n_old", "n_both", "n_near", "n_apart", "n_links", "n_pins", "n_dropped", "first", "sum_dz", "sum_shift")

_sp, _op = C.POINTER(SfcParams), C.POINTER(SfcCounts)

# name -> (restype, argtypes); every function include/sf_closure.h declares
SIGNATURES = {
    "sfc_version": (C.c_int, []),
    "sfc_params_bytes": (C.c_size_t, []),
    "sfc_counts_bytes": (C.c_size_t, []),
    "sfc_default_params": (C.c_int, [_sp]),
    "sfc_check_params": (C.c_int, [_sp]),
    "sfc_max_records": (C.c_int, [_vp, C.c_int]),
    "sfc_link_sample": (C.c_int, [_fp, _fp, C.c_float, C.c_float, _fp, _fp, _sp, C.c_void_p, C.POINTER(C.c_int32)]),
    "sfc_builder_create": (C.c_int, [_H, _pp]),
    "sfc_builder_destroy": (None, [_H]),
    "sfc_build": (C.c_int, [_H, C.c_int, _pp, _pp, _vp, _vp, _sp, C.c_void_p, C.c_int, _op]),
}

VERSION = 1  # sfc_version() of the header this table restates
INF = float("inf")


def Params(stride=4, pins=1, gate_abs=0.1, gate_rel=0.05, min_time_gap=0.0, w_link=1.0, w_pin=1.0):
    """a sfc_params; the defaults are those of sfc_default_params: parameter defaults, not tuned values"""
    return SfcParams(int(stride), int(pins), float(gate_abs), float(gate_rel), float(min_time_gap), float(w_link), float(w_pin), 0)


_bind, _product = binder("sfc_", "closure constraints are", SIGNATURES, VERSION,
                         [("params_bytes", "sfc_params", C.sizeof(SfcParams)), ("counts_bytes", "sfc_counts", C.sizeof(SfcCounts))])


def version():
    return _product().version()


def default_params():
    b = _product()
    p = SfcParams()
    b.check(b.default_params(C.byref(p)), "default_params")
    return p


def check_params(p):
    """raises SfError for parameters the library refuses (pure host: no handle, no GPU)"""
    b = _product()
    b.check(b.check_params(C.byref(p)), "check_params")


def max_records(view, stride):
    """sfc_max_records (pure host): 2 x the samples of `view` at `stride`"""
    b = _product()
    k = b.max_records(C.byref(view), int(stride))
    if k < 0:
        b.check(k, "max_records")
    return int(k)


def _f(a, n):
    return None if a is None else np.ascontiguousarray(np.asarray(a, np.float32).reshape(n))


def _p(a):
    return None if a is None else a.ctypes.data_as(_fp)


def _pose(T):
    """a 4x4 (row, col) pose as the 16 column-major floats the library takes"""
    T = np.asarray(T, np.float32)
    if T.shape != (4, 4):
        raise SfError("a pose is 4 x 4")
    return np.ascontiguousarray(T.T.ravel())


def link_sample(sa, so, zA, zO, pose_from, pose_to, params=None):
    """sfc_link_sample (pure host): (the SFC_FOUND_* bits, the records made -- the LINK before the PIN -- as a RECORD array).
    sa, so: the 12 floats of the two winning surfels, or None where nothing is drawn; the poses are 4x4 (row, col)."""
    b = _product()
    sa, so = _f(sa, 12), _f(so, 12)
    out = np.zeros(2, RECORD)
    k = C.c_int32(0)
    p = Params() if params is None else params
    mask = b.link_sample(_p(sa), _p(so), C.c_float(float(zA)), C.c_float(float(zO)), _p(_pose(pose_from)), _p(_pose(pose_to)), C.byref(p), out.ctypes.data,
                         C.byref(k))
    if mask < 0:
        b.check(mask, "link_sample")
    return int(mask), out[:k.value].copy()


class Builder(HandleChild):
    """one sfc_builder on a solver's handle: `build(maps_new, maps_old, views_from, views_to, params)`, `close()`"""

    _ptr, _destroy = "c", "builder_destroy"

    def __init__(self, solver):
        super().__init__(solver, _bind(solver.api))
        self.b.check(self.b.builder_create(solver.h, C.byref(self.c)), "builder_create")

    def _arguments(self, maps_new, maps_old, views_from, views_to, params):
        maps_new, maps_old, views_from, views_to = list(maps_new), list(maps_old), list(views_from), list(views_to)
        n = len(maps_new)
        if not (len(maps_old) == len(views_from) == len(views_to) == n):
            raise SfError("%d new maps, %d old maps, %d views from and %d views to" % (n, len(maps_old), len(views_from), len(views_to)))
        one_solver(maps_new + maps_old)
        if n and maps_new[0].solver is not self.solver:
            raise SfError("the maps of a build belong to the builder's solver")
        params = Params() if params is None else params
        params = [params] * n if isinstance(params, SfcParams) else list(params)
        if len(params) != n:
            raise SfError("%d entries and %d parameter sets" % (n, len(params)))
        m = max(n, 1)
        return n, map_array(maps_new), map_array(maps_old), (SfvView * m)(*views_from), (SfvView * m)(*views_to), (SfcParams * m)(*params), views_from, params

    def sizes(self, maps_new, maps_old, views_from, views_to, params=None):
        """the counts of a build without its records (out == NULL, max_records == 0): one dict per entry"""
        n, mn, mo, vf, vt, pr, _, _ = self._arguments(maps_new, maps_old, views_from, views_to, params)
        if n == 0:
            return []
        counts = (SfcCounts * n)()
        self.b.check(self.b.build(self.c, n, mn, mo, vf, vt, pr, None, 0, counts), "build")
        return [c.as_dict() for c in counts]

    def build(self, maps_new, maps_old, views_from, views_to, params=None):
        """sfc_build: (records, counts) -- the records of all entries one after the other as a RECORD array (entry q's are
        records[counts[q]["first"]:][:n_links + n_pins]), the counts one dict per entry. The buffer is sized by sfc_max_records."""
        n, mn, mo, vf, vt, pr, views, params = self._arguments(maps_new, maps_old, views_from, views_to, params)
        if n == 0:
            return np.zeros(0, RECORD), []
        room = 0
        for v, p in zip(views, params):
            k = self.b.max_records(C.byref(v), int(p.stride))
            if k < 0:
                self.b.check(k, "max_records")
            room += k
        out = np.empty(max(room, 1), RECORD)  # (not cleared: the library writes the records it counts, and only those are handed back)
        counts = (SfcCounts * n)()
        self.b.check(self.b.build(self.c, n, mn, mo, vf, vt, pr, out.ctypes.data, room, counts), "build")
        total = sum(c.n_links + c.n_pins for c in counts)
        recs = out[:total]
        return (recs if 2 * total >= room else recs.copy()), [c.as_dict() for c in counts]  # a mostly empty buffer is not kept alive


def as_solve_arrays(records):
    """(c_src (C, 3), c_dst (C, 3), c_time (C,), c_weight (C,)) of a RECORD array: the constraint arguments of `deform.solve`"""
    r = np.asarray(records, RECORD)
    return (np.ascontiguousarray(r["src"]), np.ascontiguousarray(r["dst"]), np.ascontiguousarray(r["time"]), np.ascontiguousarray(r["weight"]))
