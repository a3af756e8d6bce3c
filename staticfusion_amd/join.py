"""Surfel maps joined and thinned on a voxel grid: merge, decimate (include/sf_join.h, symbols ``sfj_*``).

The functions here take `SurfelMap` objects. Like the ``sfw_*`` symbols of `map_window.py`, the ``sfj_*`` symbols are not part
of the ABI of include/sf.h -- the CPU oracle does not have them -- so they have a table of their own, bound to the HIP
library a map's solver was created from (the very ``ctypes.CDLL`` object of its `Api`). Nothing here computes anything.
"""
import ctypes as C

import numpy as np

from ._capi import SfError
from ._companion import binder, map_array, one_solver

_H = C.c_void_p
_pp = C.POINTER(C.c_void_p)
_fp = C.POINTER(C.c_float)


class SfjParams(C.Structure):
    """struct sfj_params of include/sf_join.h"""

    _fields_ = [("cell", C.c_float), ("min_confidence", C.c_float), ("stamp", C.c_int32), ("dry_run", C.c_int32), ("reserved", C.c_int32 * 4)]


class SfjCounts(C.Structure):
    """struct sfj_counts of include/sf_join.h"""

    _fields_ = [("n_in", C.c_int32), ("n_outside", C.c_int32), ("n_voxels", C.c_int32), ("n_below", C.c_int32), ("n_shared", C.c_int32),
                ("n_out", C.c_int32), ("reserved", C.c_int32 * 2)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in COUNT_FIELDS}


COUNT_FIELDS = ("n_in", "n_outside", "n_voxels", "n_below", "n_shared", "n_out")

_jp = C.POINTER(SfjParams)
_cp = C.POINTER(SfjCounts)

# name -> (restype, argtypes); every function include/sf_join.h declares
SIGNATURES = {
    "sfj_version": (C.c_int, []),
    "sfj_params_bytes": (C.c_size_t, []),
    "sfj_counts_bytes": (C.c_size_t, []),
    "sfj_default_params": (C.c_int, [_jp]),
    "sfj_check_params": (C.c_int, [_jp]),
    "sfj_table_slots": (C.c_int, [C.c_int]),
    "sfj_voxel_key": (C.c_int, [_jp, _fp, C.POINTER(C.c_uint64)]),
    "sfj_hash_slot": (C.c_int, [C.c_uint64, C.c_int]),
    "sfj_thin_maps": (C.c_int, [_H, C.c_int, _pp, _jp, _cp]),
    "sfj_thin_extract": (C.c_int, [C.c_void_p, _jp, _fp, C.c_int, _cp]),
    "sfj_merge_maps": (C.c_int, [_H, C.c_int, _pp, _pp, _fp, _jp, _cp]),
}

VERSION = 1  # sfj_version() of the header this table restates


def Params(cell=0.02, min_confidence=0.0, stamp=-1, dry_run=False):
    """a sfj_params; the defaults are those of sfj_default_params: parameter defaults, not tuned values"""
    return SfjParams(float(cell), float(min_confidence), int(stamp), int(dry_run), (C.c_int32 * 4)())


_bind, _product = binder("sfj_", "joined and thinned maps are", SIGNATURES, VERSION,
                         [("params_bytes", "sfj_params", C.sizeof(SfjParams)), ("counts_bytes", "sfj_counts", C.sizeof(SfjCounts))])


def version():
    return _product().version()


def default_params():
    b = _product()
    p = SfjParams()
    b.check(b.default_params(C.byref(p)), "default_params")
    return p


def check_params(p):
    """raises SfError for parameters the library refuses (pure host: no handle, no GPU)"""
    b = _product()
    b.check(b.check_params(C.byref(p)), "check_params")


def table_slots(count):
    """the slots of a table for `count` surfels (pure host)"""
    b = _product()
    slots = b.table_slots(int(count))
    if slots < 0:
        b.check(slots, "table_slots")
    return int(slots)


def voxel_key(p, pos):
    """the voxel key of a position as a Python int, or None for a position outside the grid (pure host)"""
    b = _product()
    xyz = np.ascontiguousarray(np.asarray(pos, np.float32).reshape(3))
    key = C.c_uint64(0)
    code = b.voxel_key(C.byref(p), xyz.ctypes.data_as(_fp), C.byref(key))
    if code < 0:
        b.check(code, "voxel_key")
    return int(key.value) if code == 1 else None


def hash_slot(key, slots):
    """the first slot of a key in a table of `slots` slots (pure host)"""
    b = _product()
    slot = b.hash_slot(C.c_uint64(int(key)), int(slots))
    if slot < 0:
        b.check(slot, "hash_slot")
    return int(slot)


def _params_list(params, n):
    if params is None:
        params = Params()
    params = [params] * n if isinstance(params, SfjParams) else list(params)
    if len(params) != n:
        raise SfError("%d entries and %d parameter sets" % (n, len(params)))
    return (SfjParams * max(n, 1))(*params)


def thin(maps, params=None):
    """every map keeps one surfel per occupied voxel, the most confident one, and every surfel outside the grid, in order:
    one set of launches. Returns the counts, one dict per map (n_out: kept)."""
    maps = list(maps)
    n = len(maps)
    one_solver(maps)
    pr = _params_list(params, n)
    if n == 0:
        return []
    out = (SfjCounts * n)()
    b = _bind(maps[0].api)
    b.check(b.thin_maps(maps[0].solver.h, n, map_array(maps), pr, out), "thin_maps")
    return [c.as_dict() for c in out]


def thin_extract(surfel_map, params=None):
    """(the surfels a thin would keep (k x 12), in order; the counts); the map is unchanged"""
    b = _bind(surfel_map.api)
    p = Params() if params is None else params
    counts = SfjCounts()
    counts.n_out = -1
    code = b.thin_extract(surfel_map.m, C.byref(p), None, 0, C.byref(counts))  # the size first: refused with the count when there is any
    if code != 0 and counts.n_out <= 0:
        b.check(code, "thin_extract")
    k = int(counts.n_out)
    out = np.zeros((max(k, 1), 12), np.float32)
    if k > 0:
        b.check(b.thin_extract(surfel_map.m, C.byref(p), out.ctypes.data_as(_fp), k, C.byref(counts)), "thin_extract")
        assert counts.n_out == k
    return out[:k].copy(), counts.as_dict()


def merge(dst, src, T=None, params=None):
    """entry q: the surfels of src[q], moved by T[q] (4 x 4, source world frame -> destination world frame; None: identities),
    whose voxel dst[q] does not occupy go behind dst[q]'s own, in order. Returns the counts, one dict per entry (n_out:
    added)."""
    dst, src = list(dst), list(src)
    n = len(dst)
    if len(src) != n:
        raise SfError("%d destinations and %d sources" % (n, len(src)))
    one_solver(dst + src)
    pr = _params_list(params, n)
    if n == 0:
        return []
    t_ptr = None
    if T is not None:
        t = np.asarray(T, np.float32).reshape(n, 4, 4)
        t = np.ascontiguousarray(np.transpose(t, (0, 2, 1))).reshape(-1)  # column-major
        t_ptr = t.ctypes.data_as(_fp)
    out = (SfjCounts * n)()
    b = _bind(dst[0].api)
    b.check(b.merge_maps(dst[0].solver.h, n, map_array(dst), map_array(src), t_ptr, pr, out), "merge_maps")
    return [c.as_dict() for c in out]
