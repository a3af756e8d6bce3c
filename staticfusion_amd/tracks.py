"""Region tracks: the moving regions of `regions.py` followed from frame to frame, with a metric box (include/sf_tracks.h,
symbols ``sft_*``).

Like the ``sfr_*`` symbols of `regions.py`, the ``sft_*`` symbols are not part of the ABI of include/sf.h -- the CPU oracle does
not have them -- so they have a table of their own, bound to the HIP library a tracker's solver was created from (the very
``ctypes.CDLL`` object of its `Api`). Labelling, overlaps, assignment, ids and the integer records are computed on the device;
only the ratios of `centroids` and the differences of `velocities` are computed here.

Images go in and come out as (rows, cols) arrays and poses as 4x4 (row, col) arrays, as everywhere in this package; the library
gets them column-major.
"""
import ctypes as C

import numpy as np

from ._capi import SfError
from ._companion import HandleChild, binder, ptr_array
from .regions import Params as RegionParams
from .regions import SfrParams

_H = C.c_void_p
_pp = C.POINTER(C.c_void_p)
_ip = C.POINTER(C.c_int32)
_vp = C.c_void_p


class SftCamera(C.Structure):
    """struct sft_camera of include/sf_tracks.h"""

    _fields_ = [("pose", C.c_float * 16), ("cx", C.c_float), ("cy", C.c_float), ("fx", C.c_float), ("fy", C.c_float)]


class SftParams(C.Structure):
    """struct sft_params of include/sf_tracks.h"""

    _fields_ = [("min_overlap", C.c_int32), ("min_share", C.c_int32), ("use_depth_gate", C.c_int32), ("dz_abs", C.c_float), ("dz_rel", C.c_float),
                ("reserved", C.c_int32 * 3)]


TRACK_FIELDS = ("id", "region", "prev_region", "birth_frame", "age", "overlap", "n", "first", "v_min", "v_max", "u_min", "u_max", "z_min", "z_max")
# struct sft_track: fourteen int32, the two world corners, then the four sums of the region record and the world sums
TRACK_DTYPE = np.dtype([(k, np.int32) for k in TRACK_FIELDS] + [("qmin", np.int32, (3,)), ("qmax", np.int32, (3,))]
                       + [(k, np.int64) for k in ("sum_v", "sum_u", "sum_z", "sum_b")] + [("sum_q", np.int64, (3,))])
SUMMARY_FIELDS = ("n_regions", "n_tracked", "n_matched", "n_born", "n_ended", "n_untracked", "n_warped", "next_id")
SUMMARY_DTYPE = np.dtype([(k, np.int32) for k in SUMMARY_FIELDS])
INFO_FIELDS = ("rows", "cols", "n_slots", "max_tracks")
INFO_DTYPE = np.dtype([(k, np.int32) for k in INFO_FIELDS] + [("reserved", np.int32, (4,))])
SLOT_FIELDS = ("frames", "next_id", "n_tracks")
SLOT_DTYPE = np.dtype([(k, np.int32) for k in SLOT_FIELDS] + [("reserved", np.int32)])

_cp, _tp, _rp = C.POINTER(SftCamera), C.POINTER(SftParams), C.POINTER(SfrParams)
_fp = C.POINTER(C.c_float)

# name -> (restype, argtypes); every function include/sf_tracks.h declares
SIGNATURES = {
    "sft_version": (C.c_int, []),
    "sft_camera_bytes": (C.c_size_t, []),
    "sft_params_bytes": (C.c_size_t, []),
    "sft_track_bytes": (C.c_size_t, []),
    "sft_summary_bytes": (C.c_size_t, []),
    "sft_info_bytes": (C.c_size_t, []),
    "sft_slot_bytes": (C.c_size_t, []),
    "sft_default_params": (C.c_int, [_tp]),
    "sft_check_params": (C.c_int, [_tp]),
    "sft_relative": (C.c_int, [_fp, _fp, _fp]),
    "sft_assign": (C.c_int, [C.c_int, C.c_int, _ip, _ip, _ip, C.c_int, C.c_int, _ip, _ip, _ip]),
    "sft_tracker_create": (C.c_int, [_H, C.c_int, C.c_int, C.c_int, C.c_int, _pp]),
    "sft_tracker_destroy": (None, [_H]),
    "sft_tracker_info": (C.c_int, [_H, _vp]),
    "sft_slot_info": (C.c_int, [_H, C.c_int, _vp]),
    "sft_reset_slots": (C.c_int, [_H, C.c_int, _ip, C.c_int]),
    "sft_update_streams": (C.c_int, [_H, C.c_int, _ip, _ip, _cp, _rp, _tp, _vp, _vp, _pp]),
    "sft_update_images": (C.c_int, [_H, C.c_int, C.c_int, C.c_int, _ip, _pp, _pp, _cp, _rp, _tp, _vp, _vp, _pp]),
    "sft_update_images_device": (C.c_int, [_H, C.c_int, C.c_int, C.c_int, _ip, _pp, _pp, _cp, _rp, _tp, _vp, _vp, _pp]),
}

VERSION = 1  # sft_version() of the header this table restates


def Params(min_overlap=1, min_share=256, use_depth_gate=True, dz_abs=0.10, dz_rel=0.05):
    """a sft_params; the defaults are those of sft_default_params: parameter defaults, not tuned values"""
    return SftParams(int(min_overlap), int(min_share), int(use_depth_gate), float(dz_abs), float(dz_rel), (C.c_int32 * 3)(0, 0, 0))


def Camera(pose, cx, cy, fx, fy):
    """a sft_camera from a 4x4 (row, col) camera-to-world pose and the intrinsics in pixels"""
    p = np.asarray(pose, np.float32).reshape(4, 4)
    return SftCamera((C.c_float * 16)(*[float(x) for x in p.T.ravel()]), float(cx), float(cy), float(fx), float(fy))


_bind, _product = binder("sft_", "region tracks are", SIGNATURES, VERSION,
                         [("camera_bytes", "sft_camera", C.sizeof(SftCamera)), ("params_bytes", "sft_params", C.sizeof(SftParams)),
                          ("track_bytes", "sft_track", TRACK_DTYPE.itemsize), ("summary_bytes", "sft_summary", SUMMARY_DTYPE.itemsize),
                          ("info_bytes", "sft_info", INFO_DTYPE.itemsize), ("slot_bytes", "sft_slot", SLOT_DTYPE.itemsize)])


def version():
    return _product().version()


def default_params():
    b = _product()
    p = SftParams()
    b.check(b.default_params(C.byref(p)), "default_params")
    return p


def check_params(p):
    """raises SfError for parameters the library refuses (pure host: no handle, no GPU)"""
    b = _product()
    b.check(b.check_params(C.byref(p)), "check_params")


def relative(prev_pose, cur_pose):
    """sft_relative of two 4x4 (row, col) camera-to-world poses: the 4x4 float32 transform that takes previous-camera
    coordinates to current-camera coordinates (pure host)"""
    b = _product()
    p0 = np.ascontiguousarray(np.asarray(prev_pose, np.float32).reshape(4, 4).T)
    p1 = np.ascontiguousarray(np.asarray(cur_pose, np.float32).reshape(4, 4).T)
    out = np.zeros(16, np.float32)
    b.check(b.relative(p0.ctypes.data_as(_fp), p1.ctypes.data_as(_fp), out.ctypes.data_as(_fp)), "relative")
    return np.ascontiguousarray(out.reshape(4, 4).T)


def assign(overlap, n_prev, n_cur, min_overlap=1, min_share=256):
    """sft_assign on a (k_prev, k) table (pure host): (prev_of_cur, cur_of_prev, n_matched), 1-based with 0 for none"""
    b = _product()
    n_prev, n_cur = np.ascontiguousarray(n_prev, np.int32).ravel(), np.ascontiguousarray(n_cur, np.int32).ravel()
    kp, k = n_prev.shape[0], n_cur.shape[0]
    o = np.ascontiguousarray(overlap, np.int32).reshape(kp, k)
    poc, cop, nm = np.zeros(max(k, 1), np.int32), np.zeros(max(kp, 1), np.int32), C.c_int32(-1)
    ip = lambda a: a.ctypes.data_as(_ip)
    b.check(b.assign(kp, k, ip(o), ip(n_prev), ip(n_cur), int(min_overlap), int(min_share), ip(poc), ip(cop), C.byref(nm)), "assign")
    return poc[:k], cop[:kp], int(nm.value)


def centroids(tracks):
    """(n, 3) world centroids in metres of records of TRACK_DTYPE; records with n == 0 give zeros"""
    t = np.asarray(tracks)
    n = np.maximum(t["n"], 1).astype(np.float64)
    return t["sum_q"].astype(np.float64) / n[..., None] / 1024.0


def velocities(prev, cur, dt):
    """{id: (3,) metres per unit of dt} for the ids that `prev` and `cur` (records of two updates of one slot) both hold"""
    pc, cc = centroids(prev), centroids(cur)
    before = {int(i): pc[j] for j, i in enumerate(np.asarray(prev)["id"]) if i > 0}
    return {int(i): (cc[j] - before[int(i)]) / float(dt) for j, i in enumerate(np.asarray(cur)["id"]) if int(i) in before}


def _list(x, n, kind, what):
    x = [x] * n if isinstance(x, kind) else list(x)
    if len(x) != n:
        raise SfError("%d entries and %d %s" % (n, len(x), what))
    return x


class Tracker(HandleChild):
    """numpy wrapper over one sft_tracker: n_slots followed cameras of one image size, at most max_tracks tracks each"""

    _ptr, _destroy = "t", "tracker_destroy"

    def __init__(self, solver, n_slots=1, max_tracks=32, rows=None, cols=None):
        """rows, cols: the solver's unless given (the stream form needs the solver's)"""
        super().__init__(solver, _bind(solver.api))
        self.rows, self.cols = int(solver.rows if rows is None else rows), int(solver.cols if cols is None else cols)
        self.n_slots, self.max_tracks = int(n_slots), int(max_tracks)
        self.b.check(self.b.tracker_create(solver.h, self.rows, self.cols, self.n_slots, self.max_tracks, C.byref(self.t)), "tracker_create")

    def info(self):
        rec = np.zeros(1, INFO_DTYPE)
        self.b.check(self.b.tracker_info(self.t, rec.ctypes.data), "tracker_info")
        return {k: int(rec[k][0]) for k in INFO_FIELDS}

    def slot_info(self, slot):
        rec = np.zeros(1, SLOT_DTYPE)
        self.b.check(self.b.slot_info(self.t, int(slot), rec.ctypes.data), "slot_info")
        return {k: int(rec[k][0]) for k in SLOT_FIELDS}

    def reset(self, slots, restart_ids=False):
        s = np.ascontiguousarray(slots, np.int32).ravel()
        self.b.check(self.b.reset_slots(self.t, s.shape[0], s.ctypes.data_as(_ip), int(bool(restart_ids))), "reset_slots")

    # -- updates
    def _entries(self, slots, cameras, rparams, tparams):
        s = np.ascontiguousarray(slots, np.int32).ravel()
        n = s.shape[0]
        cams = _list(cameras, n, SftCamera, "cameras")
        rp = _list(RegionParams() if rparams is None else rparams, n, SfrParams, "region parameter sets")
        tp = _list(Params() if tparams is None else tparams, n, SftParams, "track parameter sets")
        return s, n, (SftCamera * max(n, 1))(*cams), (SfrParams * max(n, 1))(*rp), (SftParams * max(n, 1))(*tp)

    def _outputs(self, n, ids):
        want = [bool(ids)] * n if isinstance(ids, (bool, np.bool_)) else [bool(x) for x in ids]
        if len(want) != n:
            raise SfError("%d entries and %d id image flags" % (n, len(want)))
        summ = np.zeros(n, SUMMARY_DTYPE)
        trk = np.zeros((n, self.max_tracks), TRACK_DTYPE)
        imgs = [np.zeros((self.cols, self.rows), np.int32) if w else None for w in want]  # column-major
        return want, summ, trk, imgs, (ptr_array(imgs, n) if any(want) else None)

    @staticmethod
    def _finish(want, summ, trk, imgs):
        """(summaries, list of the n_tracked records per entry[, list of (rows, cols) id images or None])"""
        per = [trk[q, :int(summ["n_tracked"][q])].copy() for q in range(summ.shape[0])]
        if not any(want):
            return summ, per
        return summ, per, [None if a is None else np.ascontiguousarray(a.T) for a in imgs]

    def update_streams(self, slots, streams, cameras, rparams=None, tparams=None, ids=False):
        """entry q: slot slots[q] with the current level-0 depth of stream streams[q] of the solver and the b image of its
        last solve, read on the device. Returns (summaries, tracks) -- a structured array of SUMMARY_DTYPE and, per entry,
        the n_tracked records of TRACK_DTYPE -- and with ids (True, or one flag per entry) also the (rows, cols) id images."""
        s, n, cams, rp, tp = self._entries(slots, cameras, rparams, tparams)
        st = np.ascontiguousarray(streams, np.int32).ravel()
        if st.shape[0] != n:
            raise SfError("%d slots and %d streams" % (n, st.shape[0]))
        want, summ, trk, imgs, ip = self._outputs(n, ids)
        if n:
            self.b.check(self.b.update_streams(self.t, n, s.ctypes.data_as(_ip), st.ctypes.data_as(_ip), cams, rp, tp, summ.ctypes.data, trk.ctypes.data, ip),
                         "update_streams")
        return self._finish(want, summ, trk, imgs)

    def _column_major(self, images, what):
        out = []
        for a in images:
            if a is None:
                out.append(None)
                continue
            a = np.asarray(a, np.float32)
            if a.shape != (self.rows, self.cols):
                raise SfError("%s image of shape %r for a tracker of %d x %d" % (what, a.shape, self.rows, self.cols))
            out.append(np.ascontiguousarray(a.T))
        return out

    def update_images(self, slots, depth, b, cameras, rparams=None, tparams=None, ids=False):
        """the same with frames in host memory: depth[q] and b[q] are (rows, cols) float32 arrays (b: a list that may hold
        None where use_b is clear, or None)"""
        s, n, cams, rp, tp = self._entries(slots, cameras, rparams, tparams)
        d = self._column_major(depth, "depth")
        w = None if b is None else self._column_major(b, "b")
        if len(d) != n or any(a is None for a in d) or (w is not None and len(w) != n):
            raise SfError("one depth image per entry")
        want, summ, trk, imgs, ip = self._outputs(n, ids)
        if n:
            self.b.check(self.b.update_images(self.t, self.rows, self.cols, n, s.ctypes.data_as(_ip), ptr_array(d, n), ptr_array(w, n), cams, rp, tp,
                                              summ.ctypes.data, trk.ctypes.data, ip), "update_images")
        return self._finish(want, summ, trk, imgs)

    def update_images_device(self, slots, depth_ptrs, b_ptrs, cameras, rparams, tparams, summaries_ptr, tracks_ptr, id_ptrs=None):
        """sft_update_images_device: lists of device addresses (ints; b_ptrs and id_ptrs may be None or hold None) of
        column-major images, summaries_ptr and tracks_ptr the device addresses of n records of SUMMARY_DTYPE and
        n * max_tracks records of TRACK_DTYPE; asynchronous on the solver's stream"""
        s, n, cams, rp, tp = self._entries(slots, cameras, rparams, tparams)
        if n == 0:
            return
        self.b.check(self.b.update_images_device(self.t, self.rows, self.cols, n, s.ctypes.data_as(_ip), ptr_array(depth_ptrs, n), ptr_array(b_ptrs, n), cams, rp, tp,
                                                 C.c_void_p(int(summaries_ptr)), C.c_void_p(int(tracks_ptr)), ptr_array(id_ptrs, n)), "update_images_device")
