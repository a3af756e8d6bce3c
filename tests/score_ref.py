"""The definition of include/sf_score.h in np.float32, one expression per operation, on top of the NumPy renderer of
tests/view_ref.py: the reference of the score tests. Images are (rows, cols) arrays."""
import copy

import numpy as np

import view_ref

F = np.float32
FIELDS = ("n_frame", "n_masked", "n_map", "n_both", "n_inlier", "n_front", "n_behind", "sum_abs", "sum_sq", "sum_grey")


def score(surfels, view, depth, grey=None, b=None, params=None, tick=1):
    """(dict of the ten integers, (rows, cols) uint8 class image) of one (map, view, frame) entry; params: anything with the
    members of sfs_params"""
    v = copy.copy(view)
    v.shade = 0  # the shade of a view is ignored: gm is the grey of the winner's colour bytes
    img = view_ref.render(surfels, v, tick=tick)
    with np.errstate(all="ignore"):
        drawn = img["index"] >= 0
        zm, gm = img["depth"], view_ref.grey(img["rgb"])
        zf = np.asarray(depth, np.float32)
        fv = zf > F(0)
        w = (np.asarray(b, np.float32) > F(params.b_min)) if params.use_b else np.ones(zf.shape, bool)
        fr = fv & w
        masked = fv & ~w
        both = fr & drawn
        r = zf - zm
        tol = F(params.tol_abs) + F(params.tol_rel) * zm
        inlier = both & (np.abs(r) <= tol)
        front = both & (r < -tol)
        behind = both & (r > tol)
        q = np.rint(np.fmin(np.abs(r), F(params.max_residual)) * F(16384)).astype(np.float64)
        q = np.where(both, q, 0).astype(np.int64)
        out = dict(n_frame=fr.sum(), n_masked=masked.sum(), n_map=drawn.sum(), n_both=both.sum(), n_inlier=inlier.sum(), n_front=front.sum(),
                   n_behind=behind.sum(), sum_abs=q.sum(), sum_sq=(q * q).sum(), sum_grey=0)
        if params.use_grey:
            g = np.rint(np.fmin(np.abs(np.asarray(grey, np.float32) - gm), F(1)) * F(65536)).astype(np.float64)
            out["sum_grey"] = np.where(inlier, g, 0).astype(np.int64).sum()
        cls = np.where(drawn, 2, 0)
        cls = np.where(fr & ~drawn, 1, cls)
        cls = np.where(behind, 5, cls)
        cls = np.where(front, 4, cls)
        cls = np.where(inlier, 3, cls)
        cls = np.where(masked, 6, cls)
    return {k: int(out[k]) for k in FIELDS}, cls.astype(np.uint8)


def as_dict(record):
    """a record of staticfusion_amd.score's structured array as the dict `score` returns"""
    return {k: int(record[k]) for k in FIELDS}
