"""Place recognition: fern-coded keyframes that propose poses (include/sf_keyframes.h, symbols ``sfk_*``).

Like the ``sfs_*`` symbols of `score.py`, the ``sfk_*`` symbols are not part of the ABI of include/sf.h -- the CPU oracle does
not have them -- so they have a table of their own, bound to the HIP library a database's solver was created from (the very
``ctypes.CDLL`` object of its `Api`). Codes, distances and the selection of the best slots are computed on the device; nothing
here computes anything but shapes.

Images go in as (rows, cols) arrays and poses as 4x4 (row, col) arrays, as everywhere in this package; the library gets them
column-major. A database never interprets a pose: what `candidates` returns is what `add_*` stored.
"""
import ctypes as C

import numpy as np

from ._capi import SfError
from ._companion import HandleChild, binder, ptr_array

_H = C.c_void_p
_pp = C.POINTER(C.c_void_p)
_ip = C.POINTER(C.c_int32)
_vp = C.c_void_p

# struct sfk_fern, struct sfk_match and struct sfk_info of include/sf_keyframes.h
FERN_DTYPE = np.dtype([("cell", np.int32), ("t_grey", np.int32), ("t_depth", np.int32), ("reserved", np.int32)])
MATCH_DTYPE = np.dtype([("slot", np.int32), ("distance", np.int32)])
INFO_FIELDS = ("rows", "cols", "cell", "grid_rows", "grid_cols", "n_ferns", "words", "capacity", "count")
INFO_DTYPE = np.dtype([(k, np.int32) for k in INFO_FIELDS] + [("reserved", np.int32, (3,))])

# name -> (restype, argtypes); every function include/sf_keyframes.h declares
SIGNATURES = {
    "sfk_version": (C.c_int, []),
    "sfk_fern_bytes": (C.c_size_t, []),
    "sfk_match_bytes": (C.c_size_t, []),
    "sfk_info_bytes": (C.c_size_t, []),
    "sfk_default_ferns": (C.c_int, [C.c_int, C.c_uint64, C.c_int, _vp]),
    "sfk_check_ferns": (C.c_int, [_vp, C.c_int, C.c_int]),
    "sfk_db_create": (C.c_int, [_H, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, _pp]),
    "sfk_db_destroy": (None, [_H]),
    "sfk_db_info": (C.c_int, [_H, _vp]),
    "sfk_db_clear": (C.c_int, [_H]),
    "sfk_db_get": (C.c_int, [_H, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "sfk_db_set": (C.c_int, [_H, C.c_int, _vp, _vp, _vp, _vp]),
    "sfk_encode_streams": (C.c_int, [_H, C.c_int, _ip, _vp]),
    "sfk_encode_images": (C.c_int, [_H, C.c_int, _pp, _pp, _vp]),
    "sfk_encode_images_device": (C.c_int, [_H, C.c_int, _pp, _pp, _vp]),
    "sfk_query_streams": (C.c_int, [_H, C.c_int, _ip, _ip, C.c_int, _vp]),
    "sfk_query_codes": (C.c_int, [_H, C.c_int, _vp, _ip, C.c_int, _vp]),
    "sfk_add_streams": (C.c_int, [_H, C.c_int, _ip, _vp, _ip, _ip, C.c_int, _vp, _vp]),
    "sfk_add_codes": (C.c_int, [_H, C.c_int, _vp, _vp, _ip, _ip, C.c_int, _vp, _vp]),
}

VERSION = 1  # sfk_version() of the header this table restates

_bind, _product = binder("sfk_", "keyframe databases are", SIGNATURES, VERSION,
                         [("fern_bytes", "sfk_fern", FERN_DTYPE.itemsize), ("match_bytes", "sfk_match", MATCH_DTYPE.itemsize),
                          ("info_bytes", "sfk_info", INFO_DTYPE.itemsize)])


def version():
    return _product().version()


def default_ferns(n_ferns, seed, n_cells):
    """sfk_default_ferns: n_ferns records of FERN_DTYPE for a grid of n_cells cells (pure host: no handle, no GPU)"""
    b = _product()
    out = np.zeros(max(int(n_ferns), 1), FERN_DTYPE)
    b.check(b.default_ferns(int(n_ferns), int(seed) & ((1 << 64) - 1), int(n_cells), out.ctypes.data), "default_ferns")
    return out


def check_ferns(ferns, n_cells):
    """raises SfError for ferns the library refuses (pure host: no handle, no GPU)"""
    b = _product()
    f = np.ascontiguousarray(ferns, FERN_DTYPE)
    b.check(b.check_ferns(f.ctypes.data, f.shape[0], int(n_cells)), "check_ferns")


def _ints(x, n, what):
    a = np.ascontiguousarray(x, np.int32).ravel()
    if a.shape[0] != n:
        raise SfError("%d entries and %d %s" % (n, a.shape[0], what))
    return a


def _ip_(a):
    return a.ctypes.data_as(_ip)


class KeyframeDb(HandleChild):
    """numpy wrapper over one sfk_db: the keyframes of a solver's streams (or of images of any one size)"""

    _ptr, _destroy = "db", "db_destroy"

    def __init__(self, solver, cell, ferns=None, n_ferns=128, seed=20261020, capacity=1024, rows=None, cols=None):
        """ferns: records of FERN_DTYPE, or None for default_ferns(n_ferns, seed, cells of the grid); rows, cols: the
        solver's unless given (the stream forms need the solver's)"""
        super().__init__(solver, _bind(solver.api))
        self.rows, self.cols = int(solver.rows if rows is None else rows), int(solver.cols if cols is None else cols)
        if ferns is None:
            ferns = default_ferns(n_ferns, seed, max((self.rows // max(cell, 1)) * (self.cols // max(cell, 1)), 1))
        self.ferns = np.ascontiguousarray(ferns, FERN_DTYPE).copy()
        self.b.check(self.b.db_create(solver.h, self.rows, self.cols, int(cell), self.ferns.ctypes.data, self.ferns.shape[0], int(capacity), C.byref(self.db)),
                     "db_create")
        self.words = (self.ferns.shape[0] + 7) // 8

    def info(self):
        rec = np.zeros(1, INFO_DTYPE)
        self.b.check(self.b.db_info(self.db, rec.ctypes.data), "db_info")
        return {k: int(rec[k][0]) for k in INFO_FIELDS}

    def clear(self):
        self.b.check(self.b.db_clear(self.db), "db_clear")

    def get(self, first=0, n=None):
        """slots first .. first + n - 1 (n = None: to the last): dict of codes (n, words) uint32, poses (n, 4, 4), tags, stamps"""
        n = self.info()["count"] - first if n is None else int(n)
        codes = np.zeros((max(n, 0), self.words), np.uint32)
        poses = np.zeros((max(n, 0), 16), np.float32)
        tags, stamps = np.zeros(max(n, 0), np.int32), np.zeros(max(n, 0), np.int32)
        self.b.check(self.b.db_get(self.db, int(first), n, codes.ctypes.data, poses.ctypes.data, tags.ctypes.data, stamps.ctypes.data), "db_get")
        return dict(codes=codes, poses=np.ascontiguousarray(poses.reshape(-1, 4, 4).transpose(0, 2, 1)), tags=tags, stamps=stamps)

    def set(self, codes, poses, tags, stamps):
        """replaces the content: what `get` returned (of this database or of another of the same size and ferns)"""
        codes = self._codes(codes)
        n = codes.shape[0]
        p, t, st = self._poses(poses, n), _ints(tags, n, "tags"), _ints(stamps, n, "stamps")  # (locals: alive during the call)
        self.b.check(self.b.db_set(self.db, n, codes.ctypes.data, p.ctypes.data, t.ctypes.data, st.ctypes.data), "db_set")

    # -- encode
    def _codes(self, codes):
        c = np.ascontiguousarray(codes, np.uint32)
        if c.ndim != 2 or c.shape[1] != self.words:
            raise SfError("codes of shape %r for %d words per code" % (c.shape, self.words))
        return c

    def _poses(self, poses, n):
        p = np.asarray(poses, np.float32).reshape(-1, 4, 4)
        if p.shape[0] != n:
            raise SfError("%d entries and %d poses" % (n, p.shape[0]))
        return np.ascontiguousarray(p.transpose(0, 2, 1)).reshape(n, 16)  # column-major, like the pose of a view

    def encode_streams(self, streams):
        """the codes (n, words) uint32 of the current frames of the solver's streams `streams`"""
        st = np.ascontiguousarray(streams, np.int32).ravel()
        out = np.zeros((st.shape[0], self.words), np.uint32)
        self.b.check(self.b.encode_streams(self.db, st.shape[0], _ip_(st), out.ctypes.data), "encode_streams")
        return out

    def encode_images(self, depth, grey):
        """the same for (rows, cols) float32 images in host memory"""
        d, g = [self._column_major(x, "depth") for x in depth], [self._column_major(x, "grey") for x in grey]
        if len(d) != len(g):
            raise SfError("%d depth and %d grey images" % (len(d), len(g)))
        out = np.zeros((len(d), self.words), np.uint32)
        self.b.check(self.b.encode_images(self.db, len(d), ptr_array(d, max(len(d), 1)), ptr_array(g, max(len(d), 1)), out.ctypes.data), "encode_images")
        return out

    def _column_major(self, a, what):
        a = np.asarray(a, np.float32)
        if a.shape != (self.rows, self.cols):
            raise SfError("%s image of shape %r for a database of %d x %d" % (what, a.shape, self.rows, self.cols))
        return np.ascontiguousarray(a.T)

    def encode_images_device(self, depth_ptrs, grey_ptrs, codes_ptr):
        """sfk_encode_images_device: lists of device addresses (ints) of column-major images, codes_ptr the device address of
        (n, words) uint32; asynchronous on the solver's stream"""
        n = len(depth_ptrs)
        self.b.check(self.b.encode_images_device(self.db, n, ptr_array(depth_ptrs, max(n, 1)), ptr_array(grey_ptrs, max(n, 1)), C.c_void_p(int(codes_ptr))),
                     "encode_images_device")

    # -- query
    def _tags(self, tags, n):
        return np.full(n, -1, np.int32) if tags is None else _ints(tags, n, "tags")

    def query_streams(self, streams, tags=None, m=4):
        """(n, m) records of MATCH_DTYPE: the m best slots for the current frame of each stream, among every slot (tags None
        or a tag < 0) or the slots of tags[q]; places without a slot are (-1, -1)"""
        st = np.ascontiguousarray(streams, np.int32).ravel()
        n = st.shape[0]
        out = np.zeros((n, max(int(m), 1)), MATCH_DTYPE)
        self.b.check(self.b.query_streams(self.db, n, _ip_(st), _ip_(self._tags(tags, n)), int(m), out.ctypes.data), "query_streams")
        return out

    def query_codes(self, codes, tags=None, m=4):
        c = self._codes(codes)
        n = c.shape[0]
        out = np.zeros((n, max(int(m), 1)), MATCH_DTYPE)
        self.b.check(self.b.query_codes(self.db, n, c.ctypes.data, _ip_(self._tags(tags, n)), int(m), out.ctypes.data), "query_codes")
        return out

    # -- add
    def _add(self, fn, what, first, n, poses, tags, stamps, min_distance, nearest):
        slots = np.full(n, -1, np.int32)
        near = np.full(n, -1, MATCH_DTYPE) if nearest else None
        st = np.zeros(n, np.int32) if stamps is None else _ints(stamps, n, "stamps")
        p, t = self._poses(poses, n), _ints(tags, n, "tags")  # (locals: alive during the call)
        self.b.check(fn(self.db, n, first, p.ctypes.data, _ip_(t), _ip_(st), int(min_distance), slots.ctypes.data, None if near is None else near.ctypes.data), what)
        return (slots, near) if nearest else slots

    def add_streams(self, streams, poses, tags, stamps=None, min_distance=0, nearest=False):
        """appends the current frames of `streams` that are novel under their tags (no slot of the tag nearer than min_distance)
        with poses (n, 4, 4); returns the new slot per entry or -1, with nearest=True also the best same-tag matches before"""
        st = np.ascontiguousarray(streams, np.int32).ravel()
        return self._add(self.b.add_streams, "add_streams", _ip_(st), st.shape[0], poses, tags, stamps, min_distance, nearest)

    def add_codes(self, codes, poses, tags, stamps=None, min_distance=0, nearest=False):
        c = self._codes(codes)
        return self._add(self.b.add_codes, "add_codes", c.ctypes.data, c.shape[0], poses, tags, stamps, min_distance, nearest)

    def candidates(self, matches):
        """the stored poses of the matches of a query, ready to be the view poses of score.score_streams: dict of entry (which
        query), slot, distance and pose (k, 4, 4) over the k places of `matches` that hold a slot, in the order of the matches"""
        mt = np.asarray(matches)
        entry, place = np.nonzero(mt["slot"] >= 0)
        slots = mt["slot"][entry, place]
        poses = np.zeros((slots.shape[0], 4, 4), np.float32)
        if slots.shape[0]:
            lo, hi = int(slots.min()), int(slots.max())
            poses = self.get(lo, hi - lo + 1)["poses"][slots - lo]
        return dict(entry=entry.astype(np.int32), slot=slots.astype(np.int32), distance=mt["distance"][entry, place].astype(np.int32), pose=poses)
