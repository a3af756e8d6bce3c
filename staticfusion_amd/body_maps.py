"""Body maps: every moving region fused into a surfel map of its own (include/sf_body_maps.h, symbols ``sfp_*``).

The functions here take `SurfelMap` objects, as `join.py` does. Like the ``sfb_*`` symbols of `bodies.py`, the ``sfp_*`` symbols
are not part of the ABI of include/sf.h -- the CPU oracle does not have them -- so they have a table of their own, bound to the
HIP library a map's solver was created from (the very ``ctypes.CDLL`` object of its `Api`). Nothing here computes anything.

Images go in as (rows, cols) arrays (colour: (rows, cols, 3) uint8) and motions as 4x4 (row, col) arrays, as everywhere in this
package; the library gets depths, labels and motions column-major. Cameras are those of `tracks.py` (`tracks.Camera`): the two
structs have one layout.
"""
import ctypes as C

import numpy as np

from ._capi import SfError
from ._companion import binder, map_array, one_solver, ptr_array
from .tracks import Camera, SftCamera  # noqa: F401  (Camera: handed on, so that body_maps.Camera makes the cameras of a call)

_H = C.c_void_p
_pp = C.POINTER(C.c_void_p)
_ip = C.POINTER(C.c_int32)
_fp = C.POINTER(C.c_float)
_bp = C.POINTER(C.c_uint8)

SfpCamera = SftCamera  # struct sfp_camera of include/sf_body_maps.h: the camera of include/sf_tracks.h field for field


class SfpParams(C.Structure):
    """struct sfp_params of include/sf_body_maps.h"""

    _fields_ = [("cell", C.c_float), ("z_max", C.c_float), ("normal_dz", C.c_float), ("min_dot", C.c_float), ("conf_new", C.c_float), ("gain", C.c_float),
                ("max_weight", C.c_float), ("reserved", C.c_int32)]


class SfpCounts(C.Structure):
    """struct sfp_counts of include/sf_body_maps.h"""

    _fields_ = [("n_pixels", C.c_int32), ("n_candidates", C.c_int32), ("n_voxels", C.c_int32), ("n_merged", C.c_int32), ("n_added", C.c_int32),
                ("n_conflict", C.c_int32), ("n_out", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in COUNT_FIELDS}


COUNT_FIELDS = ("n_pixels", "n_candidates", "n_voxels", "n_merged", "n_added", "n_conflict", "n_out")

_cp, _sp, _op = C.POINTER(SfpCamera), C.POINTER(SfpParams), C.POINTER(SfpCounts)

# name -> (restype, argtypes); every function include/sf_body_maps.h declares
SIGNATURES = {
    "sfp_version": (C.c_int, []),
    "sfp_params_bytes": (C.c_size_t, []),
    "sfp_counts_bytes": (C.c_size_t, []),
    "sfp_camera_bytes": (C.c_size_t, []),
    "sfp_default_params": (C.c_int, [_sp]),
    "sfp_check_params": (C.c_int, [_sp]),
    "sfp_pixel_surfel": (C.c_int, [_fp, C.c_int, C.c_int, _cp, _bp, _sp, C.c_float, _fp]),
    "sfp_merge_surfel": (C.c_int, [_sp, _fp, _fp, C.c_float, _fp]),
    "sfp_move_maps": (C.c_int, [_H, C.c_int, _pp, _fp]),
    "sfp_fuse_images": (C.c_int, [_H, C.c_int, C.c_int, C.c_int, _pp, _pp, _pp, _cp, _ip, _pp, _fp, _sp, _op]),
    "sfp_fuse_images_device": (C.c_int, [_H, C.c_int, C.c_int, C.c_int, _pp, _pp, _pp, _cp, _ip, _pp, _fp, _sp, _op]),
}

VERSION = 1  # sfp_version() of the header this table restates


def Params(cell=0.01, z_max=8.0, normal_dz=0.05, min_dot=0.8, conf_new=0.1, gain=0.25, max_weight=32.0):
    """a sfp_params; the defaults are those of sfp_default_params: parameter defaults, not tuned values"""
    return SfpParams(float(cell), float(z_max), float(normal_dz), float(min_dot), float(conf_new), float(gain), float(max_weight), 0)


_bind, _product = binder("sfp_", "body maps are", SIGNATURES, VERSION,
                         [("params_bytes", "sfp_params", C.sizeof(SfpParams)), ("counts_bytes", "sfp_counts", C.sizeof(SfpCounts)),
                          ("camera_bytes", "sfp_camera", C.sizeof(SfpCamera))])


def version():
    return _product().version()


def default_params():
    b = _product()
    p = SfpParams()
    b.check(b.default_params(C.byref(p)), "default_params")
    return p


def check_params(p):
    """raises SfError for parameters the library refuses (pure host: no handle, no GPU)"""
    b = _product()
    b.check(b.check_params(C.byref(p)), "check_params")


def pixel_surfel(depths, v, u, cam, colour=None, params=None, time=1.0):
    """sfp_pixel_surfel (pure host): the 12 floats of the pixel surfel of the interior pixel (v, u) from its depth and those of
    (v, u - 1), (v, u + 1), (v - 1, u), (v + 1, u), or None for a pixel without a normal; colour: three bytes or None"""
    b = _product()
    z = np.ascontiguousarray(np.asarray(depths, np.float32).reshape(5))
    p = Params() if params is None else params
    c = None if colour is None else (C.c_uint8 * 3)(*[int(x) for x in colour])
    out = np.zeros(12, np.float32)
    code = b.pixel_surfel(z.ctypes.data_as(_fp), int(v), int(u), C.byref(cam), c, C.byref(p), C.c_float(float(time)), out.ctypes.data_as(_fp))
    if code < 0:
        b.check(code, "pixel_surfel")
    return out if code == 1 else None


def merge_surfel(s, pixel, params=None, time=1.0):
    """sfp_merge_surfel (pure host): the (moved) map surfel s after the pixel surfel `pixel` has been merged into it"""
    b = _product()
    p = Params() if params is None else params
    a = np.ascontiguousarray(np.asarray(s, np.float32).reshape(12))
    q = np.ascontiguousarray(np.asarray(pixel, np.float32).reshape(12))
    out = np.zeros(12, np.float32)
    b.check(b.merge_surfel(C.byref(p), a.ctypes.data_as(_fp), q.ctypes.data_as(_fp), C.c_float(float(time)), out.ctypes.data_as(_fp)), "merge_surfel")
    return out


def _motions(W, n):
    """(the array that keeps the memory alive, the pointer) of n 4x4 (row, col) motions, column-major; (None, None) for None"""
    if W is None:
        return None, None
    w = np.asarray(W, np.float32).reshape(n, 4, 4)
    w = np.ascontiguousarray(np.transpose(w, (0, 2, 1))).reshape(-1)
    return w, w.ctypes.data_as(_fp)


def _list(x, n, kind, what):
    x = [x] * n if isinstance(x, kind) else list(x)
    if len(x) != n:
        raise SfError("%d entries and %d %s" % (n, len(x), what))
    return x


def move(maps, W=None):
    """sfp_move_maps: every surfel of maps[q] moved by W[q] (4x4 (row, col); None: identities) in place"""
    maps = list(maps)
    n = len(maps)
    one_solver(maps)
    if n == 0:
        return
    keep, ptr = _motions(W, n)
    b = _bind(maps[0].api)
    b.check(b.move_maps(maps[0].solver.h, n, map_array(maps), ptr), "move_maps")


def _tables(n, cams, region_labels, params):
    cs = _list(cams, n, SfpCamera, "cameras")
    ps = _list(Params() if params is None else params, n, SfpParams, "parameter sets")
    t = np.ascontiguousarray(region_labels, np.int32).ravel()
    if t.shape[0] != n:
        raise SfError("%d entries and %d region labels" % (n, t.shape[0]))
    return (SfpCamera * max(n, 1))(*cs), (SfpParams * max(n, 1))(*ps), t


def fuse(maps, depth, labels, cams, region_labels, W=None, colour=None, params=None):
    """sfp_fuse_images: entry q fuses the pixels with labels[q] == region_labels[q] of the frame (depth[q] float32, labels[q]
    int32, (rows, cols); colour: None, or a list of (rows, cols, 3) uint8 images that may hold None) seen by cams[q] into
    maps[q], moved by W[q] (4x4 (row, col); None: identities) first. Returns the counts, one dict per entry."""
    maps = list(maps)
    n = len(maps)
    one_solver(maps)
    if n == 0:
        return []
    if len(depth) != n or len(labels) != n or (colour is not None and len(colour) != n):
        raise SfError("one image of each kind per entry")
    rows, cols = np.asarray(depth[0]).shape
    z, lab, rgb = [], [], None if colour is None else []
    for q in range(n):
        a, l = np.asarray(depth[q], np.float32), np.asarray(labels[q], np.int32)
        if a.shape != (rows, cols) or l.shape != (rows, cols):
            raise SfError("an image of shape %r or %r in a call of %d x %d" % (a.shape, l.shape, rows, cols))
        z.append(np.ascontiguousarray(a.T))
        lab.append(np.ascontiguousarray(l.T))
        if colour is not None:
            c = colour[q]
            if c is not None:
                c = np.ascontiguousarray(c, np.uint8)
                if c.shape != (rows, cols, 3):
                    raise SfError("a colour image of shape %r in a call of %d x %d" % (c.shape, rows, cols))
            rgb.append(c)
    cs, ps, t = _tables(n, cams, region_labels, params)
    keep, ptr = _motions(W, n)
    out = (SfpCounts * n)()
    b = _bind(maps[0].api)
    b.check(b.fuse_images(maps[0].solver.h, rows, cols, n, ptr_array(z, n), ptr_array(lab, n), ptr_array(rgb, n), cs, t.ctypes.data_as(_ip), map_array(maps), ptr,
                          ps, out), "fuse_images")
    return [c.as_dict() for c in out]


def fuse_device(maps, rows, cols, depth_ptrs, label_ptrs, cams, region_labels, W=None, colour_ptrs=None, params=None):
    """sfp_fuse_images_device: lists of device addresses (ints; colour_ptrs may be None or hold None) of column-major depth
    and label images and row-major colour images. Returns the counts, one dict per entry, after they have been read back."""
    maps = list(maps)
    n = len(maps)
    one_solver(maps)
    if n == 0:
        return []
    if len(depth_ptrs) != n or len(label_ptrs) != n or (colour_ptrs is not None and len(colour_ptrs) != n):
        raise SfError("one image of each kind per entry")
    cs, ps, t = _tables(n, cams, region_labels, params)
    keep, ptr = _motions(W, n)
    out = (SfpCounts * n)()
    b = _bind(maps[0].api)
    b.check(b.fuse_images_device(maps[0].solver.h, int(rows), int(cols), n, ptr_array(depth_ptrs, n), ptr_array(label_ptrs, n), ptr_array(colour_ptrs, n), cs,
                                 t.ctypes.data_as(_ip), map_array(maps), ptr, ps, out), "fuse_images_device")
    return [c.as_dict() for c in out]
