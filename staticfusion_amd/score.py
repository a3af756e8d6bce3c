"""Poses scored against surfel maps: frame-to-map agreement counts (include/sf_score.h, symbols ``sfs_*``).

Like the ``sfv_*`` symbols of `view.py`, the ``sfs_*`` symbols are not part of the ABI of include/sf.h -- the CPU oracle does
not have them -- so they have a table of their own, bound to the HIP library a map's solver was created from (the very
``ctypes.CDLL`` object of its `Api`). The counts and sums are computed on the device; only the four derived ratios of
`derived` are computed here.
"""
import ctypes as C

import numpy as np

from ._capi import SfError
from ._companion import binder, map_array, one_solver, ptr_array
from .view import SfvView

_H = C.c_void_p
_pp = C.POINTER(C.c_void_p)
_vp = C.POINTER(SfvView)


class SfsParams(C.Structure):
    """struct sfs_params of include/sf_score.h"""

    _fields_ = [("tol_abs", C.c_float), ("tol_rel", C.c_float), ("max_residual", C.c_float), ("b_min", C.c_float),
                ("use_grey", C.c_int32), ("use_b", C.c_int32), ("reserved", C.c_int32 * 2)]


FIELDS = ("n_frame", "n_masked", "n_map", "n_both", "n_inlier", "n_front", "n_behind", "sum_abs", "sum_sq", "sum_grey")
# struct sfs_score: the ten fields and two reserved words, all int64
SCORE_DTYPE = np.dtype([(k, np.int64) for k in FIELDS] + [("reserved", np.int64, (2,))])
RESULT_DTYPE = np.dtype([(k, np.int64) for k in FIELDS])
CLASS_NONE, CLASS_FRAME_ONLY, CLASS_MAP_ONLY, CLASS_INLIER, CLASS_FRONT, CLASS_BEHIND, CLASS_MASKED = range(7)

_sp = C.POINTER(SfsParams)

# name -> (restype, argtypes); every function include/sf_score.h declares
SIGNATURES = {
    "sfs_version": (C.c_int, []),
    "sfs_params_bytes": (C.c_size_t, []),
    "sfs_score_bytes": (C.c_size_t, []),
    "sfs_default_params": (C.c_int, [_sp]),
    "sfs_check_params": (C.c_int, [_sp]),
    "sfs_score_streams": (C.c_int, [_H, C.c_int, _pp, _vp, C.POINTER(C.c_int32), _sp, C.c_void_p, _pp]),
    "sfs_score_images": (C.c_int, [_H, C.c_int, _pp, _vp, _pp, _pp, _pp, _sp, C.c_void_p, _pp]),
    "sfs_score_images_device": (C.c_int, [_H, C.c_int, _pp, _vp, _pp, _pp, _pp, _sp, C.c_void_p, _pp]),
}

VERSION = 1  # sfs_version() of the header this table restates


def Params(tol_abs=0.02, tol_rel=0.01, max_residual=8.0, b_min=0.5, use_grey=True, use_b=True):
    """a sfs_params; the defaults are those of sfs_default_params: parameter defaults, not acceptance thresholds"""
    return SfsParams(float(tol_abs), float(tol_rel), float(max_residual), float(b_min), int(use_grey), int(use_b))


_bind, _product = binder("sfs_", "scores are", SIGNATURES, VERSION,
                         [("params_bytes", "sfs_params", C.sizeof(SfsParams)), ("score_bytes", "sfs_score", SCORE_DTYPE.itemsize)])


def version():
    return _product().version()


def default_params():
    b = _product()
    p = SfsParams()
    b.check(b.default_params(C.byref(p)), "default_params")
    return p


def check_params(p):
    """raises SfError for parameters the library refuses (pure host: no handle, no GPU)"""
    b = _product()
    b.check(b.check_params(C.byref(p)), "check_params")


def derived(scores):
    """inlier_ratio = n_inlier / max(n_both, 1), overlap = n_both / max(n_frame, 1), mean_abs and rms in metres, per record"""
    s = np.asarray(scores)
    both = np.maximum(s["n_both"], 1).astype(np.float64)
    return dict(inlier_ratio=s["n_inlier"] / both, overlap=s["n_both"] / np.maximum(s["n_frame"], 1).astype(np.float64),
                mean_abs=s["sum_abs"] / 16384.0 / both, rms=np.sqrt(s["sum_sq"] / both) / 16384.0)


def _entries(maps, views, params):
    maps, views = list(maps), list(views)
    n = len(maps)
    if len(views) != n:
        raise SfError("%d maps and %d views" % (n, len(views)))
    if params is None:
        params = Params()
    params = [params] * n if isinstance(params, SfsParams) else list(params)
    if len(params) != n:
        raise SfError("%d maps and %d parameter sets" % (n, len(params)))
    one_solver(maps)
    return maps, views, params, n


def _results(rec):
    out = np.zeros(rec.shape[0], RESULT_DTYPE)
    for k in FIELDS:
        out[k] = rec[k]
    return out


def _class_images(views, classes):
    if not classes:
        return None, None
    imgs = [np.zeros((v.cols, v.rows), np.uint8) for v in views]  # column-major (v, u) at v + u * rows
    return imgs, (C.c_void_p * len(imgs))(*[a.ctypes.data for a in imgs])


def _finish(rec, imgs):
    res = _results(rec)
    if imgs is None:
        return res
    return res, [np.ascontiguousarray(a.T) for a in imgs]


def score_streams(maps, views, streams, params=None, classes=False):
    """entry q: the current frame of stream streams[q] of the maps' solver (and with use_b the b image of its last solve)
    against maps[q] seen from views[q]. Returns a structured array of the ten fields of sfs_score; with classes=True
    also the list of (rows, cols) uint8 class images."""
    maps, views, params, n = _entries(maps, views, params)
    streams = [int(x) for x in streams]
    if len(streams) != n:
        raise SfError("%d maps and %d streams" % (n, len(streams)))
    rec = np.zeros(n, SCORE_DTYPE)
    if n == 0:
        return _finish(rec, [] if classes else None)
    b = _bind(maps[0].api)
    imgs, cp = _class_images(views, classes)
    b.check(b.score_streams(maps[0].solver.h, n, map_array(maps), (SfvView * n)(*views), (C.c_int32 * n)(*streams), (SfsParams * n)(*params), rec.ctypes.data, cp),
            "score_streams")
    return _finish(rec, imgs)


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


def score_images(maps, views, depth, grey=None, b=None, params=None, classes=False):
    """the same with frames in host memory: depth[q], grey[q], b[q] are (rows, cols) float32 arrays of the size of views[q]
    (grey and b: a list that may hold None, or None)"""
    maps, views, params, n = _entries(maps, views, params)
    rec = np.zeros(n, SCORE_DTYPE)
    if n == 0:
        return _finish(rec, [] if classes else None)
    bd = _bind(maps[0].api)
    d = _column_major(depth, views, "depth")
    g = None if grey is None else _column_major(grey, views, "grey")
    w = None if b is None else _column_major(b, views, "b")
    if len(d) != n or any(a is None for a in d):
        raise SfError("one depth image per entry")
    imgs, cp = _class_images(views, classes)
    bd.check(bd.score_images(maps[0].solver.h, n, map_array(maps), (SfvView * n)(*views), ptr_array(d, n), ptr_array(g, n), ptr_array(w, n),
                             (SfsParams * n)(*params), rec.ctypes.data, cp), "score_images")
    return _finish(rec, imgs)


def score_images_device(maps, views, depth_ptrs, grey_ptrs, b_ptrs, params, scores_ptr, class_ptrs=None):
    """sfs_score_images_device: lists of device addresses (ints; grey_ptrs, b_ptrs and class_ptrs may be None or hold None) of
    column-major images, scores_ptr the device address of n records of SCORE_DTYPE; asynchronous on the solver's stream"""
    maps, views, params, n = _entries(maps, views, params)
    if n == 0:
        return
    b = _bind(maps[0].api)
    b.check(b.score_images_device(maps[0].solver.h, n, map_array(maps), (SfvView * n)(*views), ptr_array(depth_ptrs, n), ptr_array(grey_ptrs, n),
                                  ptr_array(b_ptrs, n), (SfsParams * n)(*params), C.c_void_p(int(scores_ptr)), ptr_array(class_ptrs, n)),
            "score_images_device")
