"""Moving regions: connected components of the dynamic pixels, numbered, with statistics (include/sf_regions.h, symbols ``sfr_*``).

Like the ``sfs_*`` symbols of `score.py`, the ``sfr_*`` symbols are not part of the ABI of include/sf.h -- the CPU oracle does
not have them -- so they have a table of their own, bound to the HIP library a solver was created from (the very
``ctypes.CDLL`` object of its `Api`). Mask, links, components, numbering and the integer records are computed on the device;
only the four ratios of `means` are computed here.

Images go in and come out as (rows, cols) arrays, as everywhere in this package; the library gets them column-major.
"""
import ctypes as C

import numpy as np

from ._capi import SfError
from ._companion import binder, ptr_array

_H = C.c_void_p
_pp = C.POINTER(C.c_void_p)
_ip = C.POINTER(C.c_int32)


class SfrParams(C.Structure):
    """struct sfr_params of include/sf_regions.h"""

    _fields_ = [("z_max", C.c_float), ("b_max", C.c_float), ("dz_abs", C.c_float), ("dz_rel", C.c_float),
                ("connectivity", C.c_int32), ("min_pixels", C.c_int32), ("use_b", C.c_int32), ("reserved", C.c_int32)]


REGION_FIELDS = ("n", "first", "v_min", "v_max", "u_min", "u_max", "z_min", "z_max", "sum_v", "sum_u", "sum_z", "sum_b")
# struct sfr_region: eight int32, then four int64; struct sfr_summary: four int32 and four reserved words
REGION_DTYPE = np.dtype([(k, np.int32) for k in REGION_FIELDS[:8]] + [(k, np.int64) for k in REGION_FIELDS[8:]])
SUMMARY_FIELDS = ("n_mask", "n_components", "n_regions", "n_written")
SUMMARY_DTYPE = np.dtype([(k, np.int32) for k in SUMMARY_FIELDS] + [("reserved", np.int32, (4,))])

_sp = C.POINTER(SfrParams)

# name -> (restype, argtypes); every function include/sf_regions.h declares
SIGNATURES = {
    "sfr_version": (C.c_int, []),
    "sfr_params_bytes": (C.c_size_t, []),
    "sfr_region_bytes": (C.c_size_t, []),
    "sfr_summary_bytes": (C.c_size_t, []),
    "sfr_default_params": (C.c_int, [_sp]),
    "sfr_check_params": (C.c_int, [_sp]),
    "sfr_label_streams": (C.c_int, [_H, C.c_int, _ip, _sp, C.c_int, C.c_void_p, C.c_void_p, _pp]),
    "sfr_label_images": (C.c_int, [_H, C.c_int, C.c_int, C.c_int, _pp, _pp, _sp, C.c_int, C.c_void_p, C.c_void_p, _pp]),
    "sfr_label_images_device": (C.c_int, [_H, C.c_int, C.c_int, C.c_int, _pp, _pp, _sp, C.c_int, C.c_void_p, C.c_void_p, _pp]),
}

VERSION = 1  # sfr_version() of the header this table restates


def Params(z_max=8.0, b_max=0.5, dz_abs=0.05, dz_rel=0.02, connectivity=8, min_pixels=16, use_b=True):
    """a sfr_params; the defaults are those of sfr_default_params: parameter defaults, not tuned thresholds"""
    return SfrParams(float(z_max), float(b_max), float(dz_abs), float(dz_rel), int(connectivity), int(min_pixels), int(use_b), 0)


_bind, _product = binder("sfr_", "moving regions are", SIGNATURES, VERSION,
                         [("params_bytes", "sfr_params", C.sizeof(SfrParams)), ("region_bytes", "sfr_region", REGION_DTYPE.itemsize),
                          ("summary_bytes", "sfr_summary", SUMMARY_DTYPE.itemsize)])


def version():
    return _product().version()


def default_params():
    b = _product()
    p = SfrParams()
    b.check(b.default_params(C.byref(p)), "default_params")
    return p


def check_params(p):
    """raises SfError for parameters the library refuses (pure host: no handle, no GPU)"""
    b = _product()
    b.check(b.check_params(C.byref(p)), "check_params")


def means(regions):
    """(mean v, mean u, mean depth in metres, mean b) per record; records with n == 0 give zeros"""
    r = np.asarray(regions)
    n = np.maximum(r["n"], 1).astype(np.float64)
    return r["sum_v"] / n, r["sum_u"] / n, r["sum_z"] / 1024.0 / n, r["sum_b"] / 4096.0 / n


def _params(params, n):
    if params is None:
        params = Params()
    params = [params] * n if isinstance(params, SfrParams) else list(params)
    if len(params) != n:
        raise SfError("%d entries and %d parameter sets" % (n, len(params)))
    return params


def _wanted(labels, n):
    """labels: False, True or one flag per entry"""
    want = [bool(labels)] * n if isinstance(labels, (bool, np.bool_)) else [bool(x) for x in labels]
    if len(want) != n:
        raise SfError("%d entries and %d label flags" % (n, len(want)))
    return want


def _outputs(n, rows, cols, max_regions, want):
    summ = np.zeros(n, SUMMARY_DTYPE)
    reg = np.zeros((n, max(int(max_regions), 0)), REGION_DTYPE)
    imgs = [np.zeros((cols, rows), np.int32) if w else None for w in want]  # column-major (v, u) at v + u * rows
    lp = ptr_array(imgs, n) if any(want) else None
    return summ, reg, imgs, lp


def _finish(summ, reg, imgs, want):
    """(summaries, list of the n_written records per entry[, list of (rows, cols) label images or None])"""
    per = [reg[q, :int(summ["n_written"][q])].copy() for q in range(summ.shape[0])]
    if not any(want):
        return summ, per
    return summ, per, [None if a is None else np.ascontiguousarray(a.T) for a in imgs]


def label_streams(solver, streams, params=None, max_regions=64, labels=False):
    """entry q: the current level-0 depth of stream streams[q] of `solver` and the b image of its last solve, read on the
    device. Returns (summaries, regions) -- a structured array of SUMMARY_DTYPE and, per entry, the n_written records of
    REGION_DTYPE -- and with labels (True, or one flag per entry) also the list of (rows, cols) int32 label images."""
    streams = [int(x) for x in streams]
    n = len(streams)
    params, want = _params(params, n), _wanted(labels, n)
    summ, reg, imgs, lp = _outputs(n, solver.rows, solver.cols, max_regions, want)
    if n == 0:
        return _finish(summ, reg, imgs, want)
    b = _bind(solver.api)
    b.check(b.label_streams(solver.h, n, (C.c_int32 * n)(*streams), (SfrParams * n)(*params), int(max_regions), summ.ctypes.data,
                            reg.ctypes.data if reg.size else None, lp), "label_streams")
    return _finish(summ, reg, imgs, want)


def _column_major(images, rows, cols, what):
    out = []
    for a in images:
        if a is None:
            out.append(None)
            continue
        a = np.asarray(a, np.float32)
        if a.shape != (rows, cols):
            raise SfError("%s image of shape %r in a call of %d x %d" % (what, a.shape, rows, cols))
        out.append(np.ascontiguousarray(a.T))
    return out


def label_images(solver, depth, b=None, params=None, max_regions=64, labels=False):
    """the same with frames in host memory: depth[q] and b[q] are (rows, cols) float32 arrays, all of one size (b: a list
    that may hold None where use_b is clear, or None)"""
    depth = list(depth)
    n = len(depth)
    params, want = _params(params, n), _wanted(labels, n)
    if n == 0:
        return _finish(*_outputs(0, 1, 1, max_regions, want)[:3], want)
    rows, cols = np.asarray(depth[0]).shape
    d = _column_major(depth, rows, cols, "depth")
    w = None if b is None else _column_major(b, rows, cols, "b")
    if any(a is None for a in d) or (w is not None and len(w) != n):
        raise SfError("one depth image per entry")
    summ, reg, imgs, lp = _outputs(n, rows, cols, max_regions, want)
    bd = _bind(solver.api)
    bd.check(bd.label_images(solver.h, rows, cols, n, ptr_array(d, n), ptr_array(w, n), (SfrParams * n)(*params), int(max_regions), summ.ctypes.data,
                             reg.ctypes.data if reg.size else None, lp), "label_images")
    return _finish(summ, reg, imgs, want)


def label_images_device(solver, rows, cols, depth_ptrs, b_ptrs, params, max_regions, summaries_ptr, regions_ptr, label_ptrs=None):
    """sfr_label_images_device: lists of device addresses (ints; b_ptrs and label_ptrs may be None or hold None) of
    column-major images, summaries_ptr and regions_ptr the device addresses of n records of SUMMARY_DTYPE and n * max_regions
    records of REGION_DTYPE; asynchronous on the solver's stream"""
    n = len(depth_ptrs)
    params = _params(params, n)
    if n == 0:
        return
    b = _bind(solver.api)
    b.check(b.label_images_device(solver.h, int(rows), int(cols), n, ptr_array(depth_ptrs, n), ptr_array(b_ptrs, n), (SfrParams * n)(*params),
                                  int(max_regions), C.c_void_p(int(summaries_ptr)), C.c_void_p(int(regions_ptr)) if regions_ptr else None,
                                  ptr_array(label_ptrs, n)), "label_images_device")
