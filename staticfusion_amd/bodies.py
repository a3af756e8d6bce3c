"""Region motion: the rigid motion of every moving region between two frames (include/sf_bodies.h, symbols ``sfb_*``).

Like the ``sft_*`` symbols of `tracks.py`, the ``sfb_*`` symbols are not part of the ABI of include/sf.h -- the CPU oracle does
not have them -- so they have a table of their own, bound to the HIP library a solver was created from (the very
``ctypes.CDLL`` object of its `Api`). Models, systems, steps and motions are computed on the device; only `apply` and
`pairs_from_tracks` are computed here.

Images go in as (rows, cols) arrays and poses and motions come out as 4x4 (row, col) arrays, as everywhere in this package; the
library gets them column-major. Cameras are those of `tracks.py` (`tracks.Camera`): the two structs have one layout.
"""
import ctypes as C

import numpy as np

from ._capi import SfError
from ._companion import binder, ptr_array
from .align import SYSTEM_DTYPE
from .tracks import Camera, SftCamera  # noqa: F401  (Camera: handed on, so that bodies.Camera makes the cameras of a call)

_H = C.c_void_p
_pp = C.POINTER(C.c_void_p)
_ip = C.POINTER(C.c_int32)
_fp = C.POINTER(C.c_float)
_dp = C.POINTER(C.c_double)
_vp = C.c_void_p

OK, FEW_PAIRS, DEGENERATE = 0, 1, 2
SfbCamera = SftCamera  # struct sfb_camera of include/sf_bodies.h: the camera of include/sf_tracks.h field for field


class SfbParams(C.Structure):
    """struct sfb_params of include/sf_bodies.h"""

    _fields_ = [("dist_max", C.c_float), ("z_max", C.c_float), ("normal_dz", C.c_float), ("damping", C.c_float), ("iterations", C.c_int32),
                ("min_pairs", C.c_int32), ("reserved", C.c_int32 * 2)]


# struct sfb_motion: 192 bytes
MOTION_DTYPE = np.dtype([("d", np.float32, (16,)), ("w", np.float32, (16,)), ("status", np.int32), ("iterations_done", np.int32), ("n_first", np.int64),
                         ("ss_first", np.int64), ("n_last", np.int64), ("ss_last", np.int64), ("reserved", np.int64, (3,))])

_cp, _sp = C.POINTER(SfbCamera), C.POINTER(SfbParams)

# name -> (restype, argtypes); every function include/sf_bodies.h declares
SIGNATURES = {
    "sfb_version": (C.c_int, []),
    "sfb_params_bytes": (C.c_size_t, []),
    "sfb_motion_bytes": (C.c_size_t, []),
    "sfb_camera_bytes": (C.c_size_t, []),
    "sfb_system_bytes": (C.c_size_t, []),
    "sfb_default_params": (C.c_int, [_sp]),
    "sfb_check_params": (C.c_int, [_sp]),
    "sfb_world_motion": (C.c_int, [_fp, _fp, _dp, _fp]),
    "sfb_estimate_images": (C.c_int, [_H, C.c_int, C.c_int, C.c_int, _pp, _pp, _pp, _pp, _cp, _cp, _ip, _ip, _sp, C.c_int, _vp, _vp]),
    "sfb_estimate_images_device": (C.c_int, [_H, C.c_int, C.c_int, C.c_int, _pp, _pp, _pp, _pp, _cp, _cp, _ip, _ip, _sp, C.c_int, _vp, _vp]),
}

VERSION = 1  # sfb_version() of the header this table restates


def Params(dist_max=0.10, z_max=8.0, normal_dz=0.05, damping=0.0, iterations=10, min_pairs=64):
    """a sfb_params; the defaults are those of sfb_default_params: parameter defaults, not tuned values"""
    return SfbParams(float(dist_max), float(z_max), float(normal_dz), float(damping), int(iterations), int(min_pairs), (C.c_int32 * 2)(0, 0))


_bind, _product = binder("sfb_", "region motion is", SIGNATURES, VERSION,
                         [("params_bytes", "sfb_params", C.sizeof(SfbParams)), ("motion_bytes", "sfb_motion", MOTION_DTYPE.itemsize),
                          ("camera_bytes", "sfb_camera", C.sizeof(SfbCamera)), ("system_bytes", "sfb_system", SYSTEM_DTYPE.itemsize)])


def version():
    return _product().version()


def default_params():
    b = _product()
    p = SfbParams()
    b.check(b.default_params(C.byref(p)), "default_params")
    return p


def check_params(p):
    """raises SfError for parameters the library refuses (pure host: no handle, no GPU)"""
    b = _product()
    b.check(b.check_params(C.byref(p)), "check_params")


def world_motion(pose0, pose1, D):
    """sfb_world_motion (pure host): W = (T1 * D) * T0^-1 as a 4x4 (row, col) float32 array, from two 4x4 (row, col)
    camera-to-world poses and D, 12 floats row-major (or the top three rows of a 4x4 (row, col) array)"""
    b = _product()
    p0 = np.ascontiguousarray(np.asarray(pose0, np.float32).reshape(4, 4).T)
    p1 = np.ascontiguousarray(np.asarray(pose1, np.float32).reshape(4, 4).T)
    d = np.ascontiguousarray(np.asarray(D, np.float64).ravel()[:12])
    out = np.zeros(16, np.float32)
    b.check(b.world_motion(p0.ctypes.data_as(_fp), p1.ctypes.data_as(_fp), d.ctypes.data_as(_dp), out.ctypes.data_as(_fp)), "world_motion")
    return np.ascontiguousarray(out.reshape(4, 4).T)


def pairs_from_tracks(tracks, max_regions):
    """the `pairs` row of one entry from the track records of the LATER frame's update (records of tracks.TRACK_DTYPE):
    entry t - 1 is the `region` of the record whose prev_region is t, 0 where region t of the earlier frame went nowhere"""
    row = np.zeros(int(max_regions), np.int32)
    for r in np.asarray(tracks).ravel():
        t = int(r["prev_region"])
        if 1 <= t <= row.shape[0]:
            row[t - 1] = int(r["region"])
    return row


def matrix(record16):
    """a column-major 4 x 4 of a motion record (its `d` or `w`) as a 4x4 (row, col) array"""
    return np.ascontiguousarray(np.asarray(record16, np.float32).reshape(4, 4).T)


def apply(w, points):
    """the points (..., 3) moved by w, a 4x4 (row, col) array or the 16 column-major floats of a record; float64"""
    w = np.asarray(w, np.float64)
    w = w.reshape(4, 4).T if w.ndim == 1 else w
    p = np.asarray(points, np.float64)
    return p @ w[:3, :3].T + w[:3, 3]


def _list(x, n, kind, what):
    x = [x] * n if isinstance(x, kind) else list(x)
    if len(x) != n:
        raise SfError("%d entries and %d %s" % (n, len(x), what))
    return x


def _column_major(images, rows, cols, dtype, what, optional=False):
    out = []
    for a in images:
        if a is None and optional:
            out.append(None)
            continue
        a = np.asarray(a, dtype)
        if a.shape != (rows, cols):
            raise SfError("%s image of shape %r in a call of %d x %d" % (what, a.shape, rows, cols))
        out.append(np.ascontiguousarray(a.T))
    return out


def _tables(n, cams0, cams1, n_regions, pairs, params, max_regions):
    m = int(max_regions)
    c0, c1 = _list(cams0, n, SfbCamera, "cameras of frame 0"), _list(cams1, n, SfbCamera, "cameras of frame 1")
    ps = _list(Params() if params is None else params, n, SfbParams, "parameter sets")
    k = np.ascontiguousarray(n_regions, np.int32).ravel()
    if k.shape[0] != n:
        raise SfError("%d entries and %d region counts" % (n, k.shape[0]))
    pr = None
    if pairs is not None:
        pr = np.ascontiguousarray(pairs, np.int32)
        if pr.size != n * m:
            raise SfError("pairs holds %d entries, the call needs %d x %d" % (pr.size, n, m))
    return (SfbCamera * max(n, 1))(*c0), (SfbCamera * max(n, 1))(*c1), (SfbParams * max(n, 1))(*ps), k, pr


def estimate_images(solver, depth0, labels0, depth1, labels1, cams0, cams1, n_regions, pairs=None, params=None, max_regions=8, systems=False):
    """sfb_estimate_images: entry q aligns the regions 1..n_regions[q] of labels0[q] (int32, with depth0[q]) with frame 1
    (depth1[q]; labels1: None, or a list that may hold None). pairs: None or (n, max_regions) labels of frame 1. Returns a
    (n, max_regions) array of MOTION_DTYPE, and with systems=True also a (n, max_regions, I + 1) array of align.SYSTEM_DTYPE,
    I the largest `iterations`."""
    b = _bind(solver.api)
    n = len(depth0)
    if n == 0:
        raise SfError("no entries")
    rows, cols = np.asarray(depth0[0]).shape
    m = int(max_regions)
    z0, l0 = _column_major(depth0, rows, cols, np.float32, "depth"), _column_major(labels0, rows, cols, np.int32, "label")
    z1 = _column_major(depth1, rows, cols, np.float32, "depth")
    l1 = None if labels1 is None else _column_major(labels1, rows, cols, np.int32, "label", optional=True)
    if len(l0) != n or len(z1) != n or (l1 is not None and len(l1) != n):
        raise SfError("one image of each kind per entry")
    c0, c1, ps, k, pr = _tables(n, cams0, cams1, n_regions, pairs, params, m)
    its = max(int(p.iterations) for p in ps)
    out = np.zeros((n, m), MOTION_DTYPE)
    sysm = np.zeros((n, m, its + 1), SYSTEM_DTYPE) if systems else None
    b.check(b.estimate_images(solver.h, rows, cols, n, ptr_array(z0, n), ptr_array(l0, n), ptr_array(z1, n), ptr_array(l1, n), c0, c1, k.ctypes.data_as(_ip),
                              None if pr is None else pr.ctypes.data_as(_ip), ps, m, out.ctypes.data, None if sysm is None else sysm.ctypes.data), "estimate_images")
    return (out, sysm) if systems else out


def estimate_images_device(solver, rows, cols, depth0_ptrs, labels0_ptrs, depth1_ptrs, labels1_ptrs, cams0, cams1, n_regions, pairs, params, max_regions,
                           motions_ptr, systems_ptr=None):
    """sfb_estimate_images_device: lists of device addresses (ints; labels1_ptrs may be None or hold None) of column-major
    images, motions_ptr the device address of n * max_regions records of MOTION_DTYPE, systems_ptr None or that of
    n * max_regions * (I + 1) records of align.SYSTEM_DTYPE; asynchronous on the solver's stream"""
    b = _bind(solver.api)
    n = len(depth0_ptrs)
    if n == 0:
        return
    c0, c1, ps, k, pr = _tables(n, cams0, cams1, n_regions, pairs, params, max_regions)
    b.check(b.estimate_images_device(solver.h, int(rows), int(cols), n, ptr_array(depth0_ptrs, n), ptr_array(labels0_ptrs, n), ptr_array(depth1_ptrs, n),
                                     ptr_array(labels1_ptrs, n), c0, c1, k.ctypes.data_as(_ip), None if pr is None else pr.ctypes.data_as(_ip), ps, int(max_regions),
                                     C.c_void_p(int(motions_ptr)), None if systems_ptr is None else C.c_void_p(int(systems_ptr))), "estimate_images_device")
