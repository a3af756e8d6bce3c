"""Surfel maps drawn from any view: depth, colour and index images (include/sf_view.h, symbols ``sfv_*``).

Like the ``sfw_*`` symbols of `map_window.py`, the ``sfv_*`` symbols are not part of the ABI of include/sf.h -- the CPU oracle
does not have them -- so they have a table of their own, bound to the HIP library a map's solver was created from (the very
``ctypes.CDLL`` object of its `Api`). Nothing here computes anything, except `look_at`, which builds a pose on the host.
"""
import ctypes as C

import numpy as np

from ._capi import SfError
from ._companion import binder, map_array, one_solver, ptr_array

_H = C.c_void_p
_fp = C.POINTER(C.c_float)
_pp = C.POINTER(C.c_void_p)

SHADE_COLOUR, SHADE_NORMAL = 0, 1


class SfvView(C.Structure):
    """struct sfv_view of include/sf_view.h"""

    _fields_ = [("pose", C.c_float * 16), ("cx", C.c_float), ("cy", C.c_float), ("fx", C.c_float), ("fy", C.c_float),
                ("rows", C.c_int32), ("cols", C.c_int32), ("min_confidence", C.c_float), ("max_depth", C.c_float),
                ("max_age", C.c_int32), ("shade", C.c_int32), ("reserved", C.c_int32 * 2)]


_vp = C.POINTER(SfvView)

# name -> (restype, argtypes); every function include/sf_view.h declares
SIGNATURES = {
    "sfv_version": (C.c_int, []),
    "sfv_view_bytes": (C.c_size_t, []),
    "sfv_check_view": (C.c_int, [_vp]),
    "sfv_default_view": (C.c_int, [_H, C.c_void_p, _vp]),
    "sfv_render_maps": (C.c_int, [_H, C.c_int, _pp, _vp, _pp, _pp, _pp]),
    "sfv_render_maps_device": (C.c_int, [_H, C.c_int, _pp, _vp, _pp, _pp, _pp]),
    "sfv_render_surfels": (C.c_int, [_H, _fp, C.c_int, C.c_int, _vp, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sfv_last_large_sprites": (C.c_int, [_H, C.c_int, C.POINTER(C.c_int32)]),
}

VERSION = 1  # sfv_version() of the header this table restates


def View(pose, cx, cy, fx, fy, rows, cols, min_confidence=0.25, max_depth=20.0, max_age=-1, shade=SHADE_COLOUR):
    """a sfv_view; pose: 4x4 (row, col) camera-to-world"""
    T = np.asarray(pose, np.float32)
    if T.shape != (4, 4):
        raise SfError("View: pose is 4 x 4")
    return SfvView((C.c_float * 16)(*[float(x) for x in T.T.ravel()]), float(cx), float(cy), float(fx), float(fy), int(rows), int(cols),
                   float(min_confidence), float(max_depth), int(max_age), int(shade))


def view_pose(v):
    """the pose of a view as a 4x4 (row, col) array"""
    return np.array(v.pose[:], np.float32).reshape(4, 4).T.copy()


def look_at(eye, target, up=(0.0, -1.0, 0.0)):
    """camera-to-world pose (4x4, (row, col); View() stores it column-major) of a camera at `eye` whose +z axis points at
    `target`, +y down (the image's row direction) and +x right; `up` is the world's up direction"""
    eye, target, up = (np.asarray(a, np.float64).ravel() for a in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(-up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    T = np.eye(4, dtype=np.float32)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, y, z, eye
    return T


_bind, _product = binder("sfv_", "views are", SIGNATURES, VERSION, [("view_bytes", "sfv_view", C.sizeof(SfvView))])


def version():
    return _product().version()


def view_bytes():
    return int(_product().view_bytes())


def check_view(v):
    """raises SfError for a view the library refuses (pure host: no handle, no GPU)"""
    b = _product()
    b.check(b.check_view(C.byref(v)), "check_view")


def default_view(solver, surfel_map=None):
    """the solver's resolution and default intrinsics, the map's pose (identity without a map)"""
    b = _bind(solver.api)
    v = SfvView()
    b.check(b.default_view(solver.h, None if surfel_map is None else surfel_map.m, C.byref(v)), "default_view")
    return v


def _images(views, depth, rgb, index):
    d = [np.zeros((v.rows, v.cols), np.float32) if depth else None for v in views]
    c = [np.zeros((v.rows, v.cols, 3), np.uint8) if rgb else None for v in views]
    i = [np.zeros((v.rows, v.cols), np.int32) if index else None for v in views]
    return d, c, i


def render(maps, views, depth=True, rgb=True, index=True):
    """views[q] of maps[q] in one call (the same map may appear any number of times; the views may differ in size). Returns a
    list of dicts with the images asked for: depth (rows, cols) float32, rgb (rows, cols, 3) uint8, index (rows, cols) int32."""
    maps, views = list(maps), list(views)
    if len(maps) != len(views):
        raise SfError("%d maps and %d views" % (len(maps), len(views)))
    n = len(maps)
    if n == 0:
        return []
    one_solver(maps)
    b = _bind(maps[0].api)
    d, c, i = _images(views, depth, rgb, index)
    b.check(b.render_maps(maps[0].solver.h, n, map_array(maps), (SfvView * n)(*views), ptr_array(d if depth else None, n),
                          ptr_array(c if rgb else None, n), ptr_array(i if index else None, n)), "render_maps")
    return [{k: a[q] for k, a in (("depth", d), ("rgb", c), ("index", i)) if a[q] is not None} for q in range(n)]


def render_device(maps, views, depth_ptrs=None, rgb_ptrs=None, index_ptrs=None):
    """sfv_render_maps_device: lists of device addresses (ints, or None to skip an image); asynchronous on the solver's stream"""
    maps, views = list(maps), list(views)
    n = len(maps)
    if n == 0:
        return
    b = _bind(maps[0].api)
    b.check(b.render_maps_device(maps[0].solver.h, n, map_array(maps), (SfvView * n)(*views), ptr_array(depth_ptrs, n), ptr_array(rgb_ptrs, n),
                                 ptr_array(index_ptrs, n)), "render_maps_device")


def render_surfels(solver, surfels, view, tick=1, depth=True, rgb=True, index=True):
    """one view of a (count, 12) host surfel buffer without a map (what extract / page_out returned, or a checkpoint)"""
    b = _bind(solver.api)
    s = np.ascontiguousarray(surfels, dtype=np.float32).reshape(-1, 12)
    d, c, i = _images([view], depth, rgb, index)

    def p(a):
        return None if a[0] is None else a[0].ctypes.data

    b.check(b.render_surfels(solver.h, s.ctypes.data_as(_fp), s.shape[0], int(tick), C.byref(view), p(d), p(c), p(i)), "render_surfels")
    return {k: a[0] for k, a in (("depth", d), ("rgb", c), ("index", i)) if a[0] is not None}


def last_large_sprites(solver, n):
    """per view of the solver's last render call: how many surfels were drawn as large sprites (by a whole wave)"""
    b = _bind(solver.api)
    out = (C.c_int32 * max(n, 1))()
    b.check(b.last_large_sprites(solver.h, n, out), "last_large_sprites")
    return [int(x) for x in out[:n]]
