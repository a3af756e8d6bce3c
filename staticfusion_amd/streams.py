"""Single streams between handles: move, checkpoint, reset (include/sf_migrate.h, symbols ``sfm_*``).

The functions here take `Solver` objects. The ``sfm_*`` symbols are not part of the ABI of include/sf.h -- the CPU oracle
does not have them -- so they have a table of their own, bound to the HIP library a solver was created from (the very
``ctypes.CDLL`` object of its `Api`: one copy of the library, one `sf_last_error`). Nothing here computes anything.
"""
import ctypes as C

import numpy as np

from ._capi import SfError
from ._companion import binder

_H = C.c_void_p
_ip = C.POINTER(C.c_int32)

# name -> (restype, argtypes); every function include/sf_migrate.h declares
SIGNATURES = {
    "sfm_version": (C.c_int, []),
    "sfm_blob_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "sfm_copy_streams": (C.c_int, [_H, _ip, C.c_int, _H, _ip, C.c_int, C.c_int]),
    "sfm_export_stream": (C.c_int, [_H, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    "sfm_import_stream": (C.c_int, [_H, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    "sfm_reset_streams": (C.c_int, [_H, _ip, C.c_int]),
    "sfm_map_rebind": (C.c_int, [C.c_void_p, _H]),
}

VERSION = 1  # sfm_version() of the header this table restates


_bind, _product = binder("sfm_", "stream migration is", SIGNATURES, VERSION)


def _ints(a):
    v = np.ascontiguousarray(a, dtype=np.int32).ravel()
    return v, v.ctypes.data_as(_ip)


def version():
    return _product().version()


def blob_bytes(rows, cols, levels, with_input):
    """bytes of one exported stream of this geometry (pure host arithmetic: no handle, no GPU)"""
    return int(_product().blob_bytes(rows, cols, levels, int(bool(with_input))))


def copy_streams(dst, dst_streams, dst_im_count, src, src_streams, src_im_count):
    """streams src_streams of `src` -> streams dst_streams of `dst` on the device, one launch, asynchronous. The counts are the
    frame numbers the NEXT process_frame of each handle will get."""
    b = _bind(dst.api)
    d, dp = _ints(dst_streams)
    s, sp = _ints(src_streams)
    if len(d) != len(s):
        raise SfError("copy_streams: %d destination and %d source streams" % (len(d), len(s)))
    b.check(b.copy_streams(dst.h, dp, int(dst_im_count), src.h, sp, int(src_im_count), len(d)), "copy_streams")


def export_stream(solver, stream, im_count):
    """one stream as a numpy uint8 array (the blob of include/sf_migrate.h)"""
    b = _bind(solver.api)
    # room for the input-stage images, which the handle may or may not hold: the header says how long the blob really is
    blob = np.zeros(int(b.blob_bytes(solver.rows, solver.cols, solver.levels, 1)), np.uint8)
    b.check(b.export_stream(solver.h, int(stream), int(im_count), blob.ctypes.data_as(C.c_void_p), blob.nbytes), "export_stream")
    total = int(blob[24:32].view(np.uint64)[0])
    return blob[:total].copy()


def import_stream(solver, stream, im_count, blob):
    b = _bind(solver.api)
    a = np.ascontiguousarray(blob, dtype=np.uint8)
    b.check(b.import_stream(solver.h, int(stream), int(im_count), a.ctypes.data_as(C.c_void_p), a.nbytes), "import_stream")


def reset_streams(solver, streams):
    """the named streams back to what the constructor left: slots ready for a new sequence at im_count 0 (asynchronous)"""
    b = _bind(solver.api)
    v, p = _ints(streams)
    b.check(b.reset_streams(solver.h, p, len(v)), "reset_streams")


def rebind_map(surfel_map, solver):
    """the surfel map now belongs to `solver` (same device and resolution); the wrapper follows"""
    b = _bind(solver.api)
    b.check(b.map_rebind(surfel_map.m, solver.h), "map_rebind")
    surfel_map.solver, surfel_map.api = solver, solver.api
