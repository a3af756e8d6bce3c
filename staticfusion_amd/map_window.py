"""Bounded surfel maps: count, cull, extract, page out and append (include/sf_map_window.h, symbols ``sfw_*``).

The functions here take `SurfelMap` objects. Like the ``sfm_*`` symbols of `streams.py`, the ``sfw_*`` symbols are not part
of the ABI of include/sf.h -- the CPU oracle does not have them -- so they have a table of their own, bound to the HIP
library a map's solver was created from (the very ``ctypes.CDLL`` object of its `Api`). Nothing here computes anything.
"""
import ctypes as C

import numpy as np

from ._capi import SfError
from ._companion import binder, map_array, one_solver

_H = C.c_void_p
_ip = C.POINTER(C.c_int32)
_fp = C.POINTER(C.c_float)


class SfwFilter(C.Structure):
    """struct sfw_filter of include/sf_map_window.h"""

    _fields_ = [("min_confidence", C.c_float), ("max_age", C.c_int32), ("centre", C.c_float * 3), ("radius", C.c_float),
                ("invert", C.c_int32), ("reserved", C.c_int32)]


_flp = C.POINTER(SfwFilter)

# name -> (restype, argtypes); every function include/sf_map_window.h declares
SIGNATURES = {
    "sfw_version": (C.c_int, []),
    "sfw_filter_bytes": (C.c_size_t, []),
    "sfw_check_filter": (C.c_int, [_flp]),
    "sfw_count_maps": (C.c_int, [_H, C.c_int, C.POINTER(C.c_void_p), _flp, _ip]),
    "sfw_cull_maps": (C.c_int, [_H, C.c_int, C.POINTER(C.c_void_p), _flp, _ip]),
    "sfw_extract": (C.c_int, [C.c_void_p, _flp, _fp, C.c_int, _ip]),
    "sfw_page_out": (C.c_int, [C.c_void_p, _flp, _fp, C.c_int, _ip]),
    "sfw_append": (C.c_int, [C.c_void_p, _fp, C.c_int]),
}

VERSION = 1  # sfw_version() of the header this table restates


def Filter(min_confidence=0.0, max_age=-1, centre=None, radius=0.0, invert=False):
    """a sfw_filter: keep confidence >= min_confidence (> 0 enables), tick - last seen <= max_age (>= 0 enables), within
    `radius` of `centre` (radius > 0 enables); invert: the complement. No test enabled: every surfel."""
    c = (0.0, 0.0, 0.0) if centre is None else tuple(float(x) for x in np.asarray(centre, np.float32).ravel())
    if len(c) != 3:
        raise SfError("Filter: centre has 3 components")
    return SfwFilter(float(min_confidence), int(max_age), (C.c_float * 3)(*c), float(radius), int(bool(invert)), 0)


_bind, _product = binder("sfw_", "map windows are", SIGNATURES, VERSION, [("filter_bytes", "sfw_filter", C.sizeof(SfwFilter))])


def version():
    return _product().version()


def filter_bytes():
    return int(_product().filter_bytes())


def check_filter(f):
    """raises SfError for a filter the library refuses (pure host: no handle, no GPU)"""
    b = _product()
    b.check(b.check_filter(C.byref(f)), "check_filter")


def camera_centre(surfel_map):
    """the camera position of the map's current pose, world frame: a centre for Filter(radius=...)"""
    return surfel_map.info()["pose"][:3, 3].copy()


def _batch(maps, filters):
    maps, filters = list(maps), list(filters)
    if len(maps) != len(filters):
        raise SfError("%d maps and %d filters" % (len(maps), len(filters)))
    n = len(maps)
    one_solver(maps)
    return n, map_array(maps), (SfwFilter * max(n, 1))(*filters), (C.c_int32 * max(n, 1))()


def count(maps, filters):
    """how many surfels of maps[q] filters[q] selects; nothing changes"""
    n, mp, fl, out = _batch(maps, filters)
    if n == 0:
        return []
    b = _bind(maps[0].api)
    b.check(b.count_maps(maps[0].solver.h, n, mp, fl, out), "count_maps")
    return [int(x) for x in out[:n]]


def cull(maps, filters):
    """every map keeps exactly the surfels its filter selects, in order: one set of launches; returns the new counts"""
    n, mp, fl, out = _batch(maps, filters)
    if n == 0:
        return []
    b = _bind(maps[0].api)
    b.check(b.cull_maps(maps[0].solver.h, n, mp, fl, out), "cull_maps")
    return [int(x) for x in out[:n]]


def _copy_out(surfel_map, f, fn_name):
    b = _bind(surfel_map.api)
    fn = getattr(b, fn_name)
    need = C.c_int32(-1)
    code = fn(surfel_map.m, C.byref(f), None, 0, C.byref(need))  # the size first: refused with the count when there is any
    if code != 0 and need.value <= 0:
        b.check(code, fn_name)
    out = np.zeros((max(need.value, 1), 12), np.float32)
    if need.value > 0:
        got = C.c_int32(0)
        b.check(fn(surfel_map.m, C.byref(f), out.ctypes.data_as(_fp), need.value, C.byref(got)), fn_name)
        assert got.value == need.value
    return out[: max(need.value, 0)].copy()


def extract(surfel_map, f):
    """the selected surfels (k x 12), in order; the map is unchanged"""
    return _copy_out(surfel_map, f, "extract")


def page_out(surfel_map, f):
    """the surfels NOT selected (k x 12), in order; they leave the map, the selected ones stay"""
    return _copy_out(surfel_map, f, "page_out")


def append(surfel_map, surfels):
    """page in: the surfels go behind the map's own"""
    b = _bind(surfel_map.api)
    s = np.ascontiguousarray(surfels, dtype=np.float32).reshape(-1, 12)
    b.check(b.append(surfel_map.m, s.ctypes.data_as(_fp), s.shape[0]), "append")
