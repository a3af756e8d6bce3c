"""Frames and maps for the body map tests (include/sf_body_maps.h): scenes that are functions of their size alone, ray-cast or
evaluated in fp64 with depths rounded to millimetres. Imports neither the product nor the oracle."""
import numpy as np

import body_cases as bc
import body_map_ref as pr

F = np.float32
WALL = 3.0
SPHERE_CENTRE = np.array([0.02, -0.01, 1.4])
SPHERE_RADIUS = 0.25


def cam(rows, cols, T=None):
    return bc.cam(rows, cols, T)


def plane(rows, cols, shift=0.0):
    """a slanted plane that fills the frame: every interior pixel has a normal at any size"""
    v, u = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    z = 2.0 + 0.004 * u + 0.007 * v - shift
    return (np.round(z * 1000.0) / 1000.0).astype(F)


def labels_mixed(rows, cols, t=2):
    """label t inside a centred ellipse that reaches the border rows of small frames; outside it 0, 1, t + 1 and -1 in turn, so
    that every wave sees labels <= 0 and > t beside its own"""
    v, u = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    inside = ((v - (rows - 1) / 2.0) / max(rows * 0.45, 1.0)) ** 2 + ((u - (cols - 1) / 2.0) / max(cols * 0.4, 1.0)) ** 2 <= 1.0
    other = np.array([0, 1, t + 1, -1], np.int32)[(v + 2 * u) % 4]
    return np.where(inside, t, other).astype(np.int32)


def colours(rows, cols):
    v, u = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    return np.stack([(v * 7 + u * 13 + k * 29 + 3) % 256 for k in range(3)], -1).astype(np.uint8)


def sphere(rows, cols, camera, centre=SPHERE_CENTRE, radius=SPHERE_RADIUS):
    """(depth (rows, cols) float32 rounded to millimetres, mask of the pixels that see the sphere) of a sphere in front of a wall at
    z = WALL, from `camera`"""
    T = np.asarray(camera["pose"], np.float64)
    v, u = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    d_cam = np.stack([(u - float(camera["cx"])) / float(camera["fx"]), (v - float(camera["cy"])) / float(camera["fy"]), np.ones_like(u)], -1)
    d = d_cam @ T[:3, :3].T
    o = T[:3, 3] - np.asarray(centre, np.float64)
    a, b, c = (d * d).sum(-1), 2.0 * (d @ o), float(o @ o) - radius * radius
    disc = b * b - 4.0 * a * c
    with np.errstate(all="ignore"):
        ts = (-b - np.sqrt(disc)) / (2.0 * a)
        tw = (WALL - T[2, 3]) / d[..., 2]
    hit = (disc > 0) & (ts > 0)
    depth = np.where(hit, ts, tw)  # d_cam has z = 1: the ray parameter is the camera depth
    return (np.round(depth * 1000.0) / 1000.0).astype(F), hit


def first_map(rows, cols, t=2, p=None, tick=1, colour=True):
    """(surfels, counts) of the first sighting of labels_mixed's region on the plane: everything added, in pixel order"""
    return pr.fuse(np.zeros((0, 12), F), tick, plane(rows, cols), labels_mixed(rows, cols, t), cam(rows, cols), t, None, colours(rows, cols) if colour else None, p)


def special_map(surf, seed=3):
    """the surfels with special confidences, weights and colours and out-of-grid positions spread over them (a copy)"""
    s = np.array(surf, F)
    n = s.shape[0]
    special = [(3, np.nan), (3, -0.0), (3, 0.0), (3, -1.0), (3, np.inf), (3, 1.0), (5, np.nan), (5, np.inf), (5, 40.0), (5, 0.0), (4, np.nan), (4, -5.0),
               (4, 16777216.0), (4, 3e9), (0, np.nan), (1, np.inf), (2, 3e38), (11, np.nan), (8, np.nan), (8, 0.0)]
    for j, (col, v) in enumerate(special):
        if n:
            s[(j * 5 + seed) % n, col] = v
    return s
