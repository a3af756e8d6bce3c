"""Poses refined against surfel maps: damped point-to-plane steps (include/sf_align.h, symbols ``sfa_*``).

Like the ``sfs_*`` symbols of `score.py`, the ``sfa_*`` symbols are not part of the ABI of include/sf.h -- the CPU oracle does
not have them -- so they have a table of their own, bound to the HIP library a map's solver was created from (the very
``ctypes.CDLL`` object of its `Api`). Systems, steps and poses are computed on the device; nothing is computed here.
"""
import ctypes as C

import numpy as np

from ._capi import SfError
from ._companion import binder, map_array, one_solver, ptr_array
from .view import SfvView

_H = C.c_void_p
_pp = C.POINTER(C.c_void_p)
_vp = C.POINTER(SfvView)

OK, FEW_PAIRS, DEGENERATE = 0, 1, 2


class SfaParams(C.Structure):
    """struct sfa_params of include/sf_align.h"""

    _fields_ = [("dist_max", C.c_float), ("z_max", C.c_float), ("b_min", C.c_float), ("damping", C.c_float),
                ("iterations", C.c_int32), ("stride", C.c_int32), ("min_pairs", C.c_int32), ("use_b", C.c_int32)]


# struct sfa_system: 256 bytes of int64
SYSTEM_DTYPE = np.dtype([("n", np.int64), ("ss", np.int64), ("g", np.int64, (6,)), ("H", np.int64, (21,)), ("reserved", np.int64, (3,))])
# struct sfa_result: 128 bytes
RESULT_DTYPE = np.dtype([("pose", np.float32, (16,)), ("status", np.int32), ("iterations_done", np.int32), ("n_first", np.int64),
                         ("ss_first", np.int64), ("n_last", np.int64), ("ss_last", np.int64), ("reserved", np.int64, (3,))])

_sp = C.POINTER(SfaParams)
_dp = C.POINTER(C.c_double)

# name -> (restype, argtypes); every function include/sf_align.h declares
SIGNATURES = {
    "sfa_version": (C.c_int, []),
    "sfa_params_bytes": (C.c_size_t, []),
    "sfa_result_bytes": (C.c_size_t, []),
    "sfa_system_bytes": (C.c_size_t, []),
    "sfa_default_params": (C.c_int, [_sp]),
    "sfa_check_params": (C.c_int, [_sp]),
    "sfa_step": (C.c_int, [C.c_void_p, C.c_float, _dp, _dp]),
    "sfa_refine_streams": (C.c_int, [_H, C.c_int, _pp, _vp, C.POINTER(C.c_int32), _sp, C.c_void_p, C.c_void_p]),
    "sfa_refine_images": (C.c_int, [_H, C.c_int, _pp, _vp, _pp, _pp, _sp, C.c_void_p, C.c_void_p]),
    "sfa_refine_images_device": (C.c_int, [_H, C.c_int, _pp, _vp, _pp, _pp, _sp, C.c_void_p, C.c_void_p]),
}

VERSION = 1  # sfa_version() of the header this table restates


def Params(dist_max=0.15, z_max=8.0, b_min=0.5, damping=0.0, iterations=10, stride=1, min_pairs=64, use_b=True):
    """a sfa_params; the defaults are those of sfa_default_params: parameter defaults, not tuned values"""
    return SfaParams(float(dist_max), float(z_max), float(b_min), float(damping), int(iterations), int(stride), int(min_pairs), int(use_b))


_bind, _product = binder("sfa_", "pose refinement is", SIGNATURES, VERSION,
                         [("params_bytes", "sfa_params", C.sizeof(SfaParams)), ("result_bytes", "sfa_result", RESULT_DTYPE.itemsize),
                          ("system_bytes", "sfa_system", SYSTEM_DTYPE.itemsize)])


def version():
    return _product().version()


def default_params():
    b = _product()
    p = SfaParams()
    b.check(b.default_params(C.byref(p)), "default_params")
    return p


def check_params(p):
    """raises SfError for parameters the library refuses (pure host: no handle, no GPU)"""
    b = _product()
    b.check(b.check_params(C.byref(p)), "check_params")


def step(system, damping, D):
    """sfa_step (pure host: no handle, no GPU): (status, the updated 3 x 4 estimate as 12 float64, or None when the step is
    refused). system: one record of SYSTEM_DTYPE; D: 12 float64, row-major"""
    b = _product()
    rec = np.ascontiguousarray(np.asarray(system, SYSTEM_DTYPE).reshape(1))
    d_in = np.ascontiguousarray(np.asarray(D, np.float64).reshape(12))
    d_out = np.zeros(12, np.float64)
    code = b.step(rec.ctypes.data, float(damping), d_in.ctypes.data_as(_dp), d_out.ctypes.data_as(_dp))
    if code < 0:
        b.check(code, "step")
    return code, (d_out if code == OK else None)


def pose_matrix(result):
    """the refined 4 x 4 pose of one record of RESULT_DTYPE"""
    return np.array(result["pose"], np.float32).reshape(4, 4).T


def _entries(maps, views, params):
    maps, views = list(maps), list(views)
    n = len(maps)
    if len(views) != n:
        raise SfError("%d maps and %d views" % (n, len(views)))
    if params is None:
        params = Params()
    params = [params] * n if isinstance(params, SfaParams) else list(params)
    if len(params) != n:
        raise SfError("%d maps and %d parameter sets" % (n, len(params)))
    one_solver(maps)
    return maps, views, params, n


def _systems_room(params, n, systems):
    """(array, address or None, I + 1)"""
    per = max([p.iterations for p in params] + [0]) + 1
    if not systems:
        return None, None, per
    rec = np.zeros((n, per), SYSTEM_DTYPE)
    return rec, rec.ctypes.data, per


def refine_streams(maps, views, streams, params=None, systems=False):
    """entry q: views[q].pose refined against maps[q] with the current frame of stream streams[q] of the maps' solver (and
    with use_b the b image of its last solve). Returns the records of RESULT_DTYPE; with systems=True also an
    (n, I + 1) array of SYSTEM_DTYPE, I the largest `iterations` of the call."""
    maps, views, params, n = _entries(maps, views, params)
    streams = [int(x) for x in streams]
    if len(streams) != n:
        raise SfError("%d maps and %d streams" % (n, len(streams)))
    res = np.zeros(n, RESULT_DTYPE)
    sys_rec, sys_ptr, _ = _systems_room(params, n, systems)
    if n:
        b = _bind(maps[0].api)
        b.check(b.refine_streams(maps[0].solver.h, n, map_array(maps), (SfvView * n)(*views), (C.c_int32 * n)(*streams), (SfaParams * n)(*params),
                                 res.ctypes.data, sys_ptr), "refine_streams")
    return (res, sys_rec) if systems else res


def _column_major(images, views, what):
    out = []
    for a, v in zip(images, views):
        if a is None:
            out.append(None)
            continue
        a = np.asarray(a, np.float32)
        if a.shape != (v.rows, v.cols):
            raise SfError("%s image of shape %r for a view of %d x %d" % (what, a.shape, v.rows, v.cols))
        out.append(np.ascontiguousarray(a.T))
    return out


def refine_images(maps, views, depth, b=None, params=None, systems=False):
    """the same with frames in host memory: depth[q], b[q] are (rows, cols) float32 arrays of the size of views[q] (b: a list
    that may hold None, or None)"""
    maps, views, params, n = _entries(maps, views, params)
    res = np.zeros(n, RESULT_DTYPE)
    sys_rec, sys_ptr, _ = _systems_room(params, n, systems)
    if n:
        bd = _bind(maps[0].api)
        d = _column_major(depth, views, "depth")
        w = None if b is None else _column_major(b, views, "b")
        if len(d) != n or any(a is None for a in d):
            raise SfError("one depth image per entry")
        bd.check(bd.refine_images(maps[0].solver.h, n, map_array(maps), (SfvView * n)(*views), ptr_array(d, n), ptr_array(w, n), (SfaParams * n)(*params),
                                  res.ctypes.data, sys_ptr), "refine_images")
    return (res, sys_rec) if systems else res


def refine_images_device(maps, views, depth_ptrs, b_ptrs, params, results_ptr, systems_ptr=None):
    """sfa_refine_images_device: lists of device addresses (ints; b_ptrs may be None or hold None) of column-major images,
    results_ptr the device address of n records of RESULT_DTYPE, systems_ptr None or that of n * (I + 1) records of
    SYSTEM_DTYPE; asynchronous on the solver's stream"""
    maps, views, params, n = _entries(maps, views, params)
    if n == 0:
        return
    b = _bind(maps[0].api)
    b.check(b.refine_images_device(maps[0].solver.h, n, map_array(maps), (SfvView * n)(*views), ptr_array(depth_ptrs, n), ptr_array(b_ptrs, n),
                                   (SfaParams * n)(*params), C.c_void_p(int(results_ptr)), None if systems_ptr is None else C.c_void_p(int(systems_ptr))),
            "refine_images_device")
