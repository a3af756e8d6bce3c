"""Surfel maps registered against each other on a voxel table (include/sf_register.h, symbols ``sfg_*``).

`Registrar(solver).register_maps(dst, src, T0, params)` takes `SurfelMap` objects of one solver and returns one record of
RESULT_DTYPE per entry (with ``systems=True`` also the systems of every linearisation, with ``pairs=True`` also the partner of
every source surfel at the last one). Like the symbols of the other companion modules, the ``sfg_*`` symbols are not part of
the ABI of include/sf.h -- the CPU oracle does not have them -- so they have a table of their own, bound to the HIP library a
solver was created from (the very ``ctypes.CDLL`` object of its `Api`). Nothing here computes anything.
"""
import ctypes as C

import numpy as np

from ._capi import SfError
from ._companion import HandleChild, binder, map_array, one_solver, ptr_array

_H = C.c_void_p
_pp = C.POINTER(C.c_void_p)
_fp = C.POINTER(C.c_float)
_dp = C.POINTER(C.c_double)

OK, FEW_PAIRS, DEGENERATE = 0, 1, 2  # SFG_*
NOT_PAIRED, NOT_SAMPLED = -1, -2     # what a pair says beside a destination index


class SfgParams(C.Structure):
    """struct sfg_params of include/sf_register.h"""

    _fields_ = [("cell", C.c_float), ("dist_max", C.c_float), ("min_cos", C.c_float), ("min_confidence", C.c_float), ("damping", C.c_float),
                ("iterations", C.c_int32), ("stride", C.c_int32), ("min_pairs", C.c_int32)]


# struct sfg_system: 256 bytes of int64
SYSTEM_DTYPE = np.dtype([("n", np.int64), ("ss", np.int64), ("g", np.int64, (6,)), ("H", np.int64, (21,)), ("reserved", np.int64, (3,))])
# struct sfg_result: 128 bytes
RESULT_DTYPE = np.dtype([("T", np.float32, (16,)), ("status", np.int32), ("iterations_done", np.int32), ("n_first", np.int64), ("ss_first", np.int64),
                         ("n_last", np.int64), ("ss_last", np.int64), ("n_sampled", np.int32), ("n_outside", np.int32), ("reserved", np.int32, (4,))])

_sp = C.POINTER(SfgParams)

# name -> (restype, argtypes); every function include/sf_register.h declares
SIGNATURES = {
    "sfg_version": (C.c_int, []),
    "sfg_params_bytes": (C.c_size_t, []),
    "sfg_system_bytes": (C.c_size_t, []),
    "sfg_result_bytes": (C.c_size_t, []),
    "sfg_default_params": (C.c_int, [_sp]),
    "sfg_check_params": (C.c_int, [_sp]),
    "sfg_linearise": (C.c_int, [_fp, C.c_int, _fp, C.c_int, _sp, _dp, C.c_void_p, C.c_void_p]),
    "sfg_registrar_create": (C.c_int, [_H, _pp]),
    "sfg_registrar_destroy": (None, [_H]),
    "sfg_register_maps": (C.c_int, [_H, C.c_int, _pp, _pp, _fp, _sp, C.c_void_p, C.c_void_p, _pp]),
}

VERSION = 1  # sfg_version() of the header this table restates


def Params(cell=0.1, dist_max=0.05, min_cos=0.5, min_confidence=0.0, damping=0.0, iterations=10, stride=1, min_pairs=64):
    """a sfg_params; the defaults are those of sfg_default_params: parameter defaults, not tuned values"""
    return SfgParams(float(cell), float(dist_max), float(min_cos), float(min_confidence), float(damping), int(iterations), int(stride), int(min_pairs))


_bind, _product = binder("sfg_", "map registration is", SIGNATURES, VERSION,
                         [("params_bytes", "sfg_params", C.sizeof(SfgParams)), ("system_bytes", "sfg_system", SYSTEM_DTYPE.itemsize),
                          ("result_bytes", "sfg_result", RESULT_DTYPE.itemsize)])


def version():
    return _product().version()


def default_params():
    b = _product()
    p = SfgParams()
    b.check(b.default_params(C.byref(p)), "default_params")
    return p


def check_params(p):
    """raises SfError for parameters the library refuses (pure host: no handle, no GPU)"""
    b = _product()
    b.check(b.check_params(C.byref(p)), "check_params")


def transform_matrix(result):
    """the 4 x 4 transform of one record of RESULT_DTYPE"""
    return np.array(result["T"], np.float32).reshape(4, 4).T


def linearise(dst, src, params=None, E=None, pairs=False):
    """sfg_linearise (pure host: no handle, no GPU): one record of SYSTEM_DTYPE for the source surfels `src` (n x 12) against
    the table of the destination surfels `dst` at the estimate E (12 float64, row-major 3 x 4; None: the identity); with
    pairs=True also the int32 pair of every source surfel"""
    b = _product()
    d = np.ascontiguousarray(np.asarray(dst, np.float32).reshape(-1, 12))
    s = np.ascontiguousarray(np.asarray(src, np.float32).reshape(-1, 12))
    p = Params() if params is None else params
    e = np.ascontiguousarray(np.asarray([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0] if E is None else E, np.float64).reshape(12))
    rec = np.zeros(1, SYSTEM_DTYPE)
    out = np.zeros(s.shape[0], np.int32) if pairs else None
    b.check(b.linearise(d.ctypes.data_as(_fp) if d.shape[0] else None, d.shape[0], s.ctypes.data_as(_fp) if s.shape[0] else None, s.shape[0], C.byref(p),
                        e.ctypes.data_as(_dp), rec.ctypes.data, out.ctypes.data if pairs and out.size else None), "linearise")
    return (rec[0], out) if pairs else rec[0]


class Registrar(HandleChild):
    """one sfg_registrar on a solver's handle: `register_maps(dst, src, ...)`, `close()`"""

    _ptr, _destroy = "r", "registrar_destroy"

    def __init__(self, solver):
        super().__init__(solver, _bind(solver.api))
        self.b.check(self.b.registrar_create(solver.h, C.byref(self.r)), "registrar_create")

    def register_maps(self, dst, src, T0=None, params=None, systems=False, pairs=False):
        """sfg_register_maps. dst, src: lists of `SurfelMap`s of the registrar's solver, entry q registers src[q] against
        dst[q]; T0: None for identities or n 4 x 4 matrices (source world -> destination world); params: one `SfgParams` for
        all entries, a list with one per entry, or None for the defaults. Returns the records of RESULT_DTYPE; with
        systems=True also an (n, I + 1) array of SYSTEM_DTYPE, I the largest `iterations` of the call; with pairs=True also
        one int32 array per entry (the partner's destination index, NOT_PAIRED or NOT_SAMPLED per source surfel)."""
        dst, src = list(dst), list(src)
        n = len(dst)
        if len(src) != n:
            raise SfError("%d destinations and %d sources" % (n, len(src)))
        one_solver(dst + src)
        if n and dst[0].solver is not self.solver:
            raise SfError("the maps of a registration belong to the registrar's solver")
        params = Params() if params is None else params
        params = [params] * n if isinstance(params, SfgParams) else list(params)
        if len(params) != n:
            raise SfError("%d entries and %d parameter sets" % (n, len(params)))
        t0 = None
        if T0 is not None:
            t0 = np.ascontiguousarray(np.asarray(T0, np.float32).reshape(n, 4, 4).transpose(0, 2, 1))  # column-major
        res = np.zeros(n, RESULT_DTYPE)
        per = max([p.iterations for p in params] + [0]) + 1
        sys_rec = np.zeros((n, per), SYSTEM_DTYPE) if systems else None
        out = [np.zeros(m.info()["count"], np.int32) for m in src] if pairs else None
        if n:
            self.b.check(self.b.register_maps(self.r, n, map_array(dst), map_array(src), None if t0 is None else t0.ctypes.data_as(_fp), (SfgParams * n)(*params),
                                              res.ctypes.data, sys_rec.ctypes.data if systems else None,
                                              ptr_array([a if a.size else None for a in out], n) if pairs else None), "register_maps")
        got = (res,)
        if systems:
            got += (sys_rec,)
        if pairs:
            got += (out,)
        return got if len(got) > 1 else res
