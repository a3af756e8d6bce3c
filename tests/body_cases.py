"""Frame pairs for the body tests (include/sf_bodies.h): scenes that are functions of their size alone, ray-cast in fp64 with
depths rounded to millimetres. The main one is a four-faced pyramid, apex (0, 0, 1.2) towards the camera, face slope 0.8, cut at
z = 1.5, in front of a wall at z = 3: its four face normals make all six degrees of a rigid motion observable, which a sphere
or a single plane does not. Imports neither the product nor the oracle."""
import numpy as np

import track_ref as tr

F = np.float32
APEX, SLOPE, CUT, WALL = 1.2, 0.8, 1.5, 3.0
CENTRE = np.array([0.0, 0.0, 1.35])
ROTVEC = np.array([0.01, 0.03, -0.02])
SHIFT = np.array([0.02, 0.01, -0.01])


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def motion(rotvec=ROTVEC, shift=SHIFT, centre=CENTRE):
    """the 4x4 that turns by rotvec about centre and then shifts"""
    R = rodrigues(rotvec)
    W = np.eye(4)
    W[:3, :3] = R
    W[:3, 3] = np.asarray(centre) - R @ np.asarray(centre) + np.asarray(shift)
    return W


def pose(rotvec=(0, 0, 0), shift=(0, 0, 0)):
    T = np.eye(4)
    T[:3, :3] = rodrigues(rotvec)
    T[:3, 3] = shift
    return T


def cam(rows, cols, T=None):
    f = 0.875 * cols  # 70 at 60 x 80
    return tr.camera(np.eye(4) if T is None else T, (cols - 1) / 2.0, (rows - 1) / 2.0, f, f)


def render(rows, cols, camera, body=None):
    """(depth (rows, cols) float32 in metres rounded to millimetres, mask of the pixels that see the pyramid) of the pyramid
    under the body-to-world transform `body` and the wall, from `camera`"""
    body = np.eye(4) if body is None else body
    T = np.asarray(camera["pose"], np.float64)
    v, u = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    d_cam = np.stack([(u - float(camera["cx"])) / float(camera["fx"]), (v - float(camera["cy"])) / float(camera["fy"]), np.ones_like(u)], -1)
    d_w = d_cam @ T[:3, :3].T
    o_w = T[:3, 3]
    Rb, tb = body[:3, :3], body[:3, 3]
    o_b = Rb.T @ (o_w - tb)
    d_b = d_w @ Rb  # rows: R_b^T d
    best = np.full((rows, cols), np.inf)
    with np.errstate(all="ignore"):
        for axis in (0, 1):
            for s in (1.0, -1.0):
                nrm = np.zeros(3)
                nrm[axis], nrm[2] = -SLOPE * s, 1.0
                t = (APEX - nrm @ o_b) / (d_b @ nrm)
                p = o_b + t[..., None] * d_b
                ok = (t > 0) & (s * p[..., axis] >= np.abs(p[..., 1 - axis])) & (p[..., 2] <= CUT)
                best = np.where(ok & (t < best), t, best)
        tw = (WALL - o_w[2]) / d_w[..., 2]
    hit = np.isfinite(best)
    depth = np.where(hit, best, tw)
    return (np.round(depth * 1000.0) / 1000.0).astype(F), hit


def pyramid_pair(rows, cols, T0=None, T1=None, moved=True):
    """(z0, l0, z1, l1, cam0, cam1): the pyramid is region 1 of both frames; it moves by motion() between them unless told not to"""
    c0, c1 = cam(rows, cols, T0), cam(rows, cols, T1)
    z0, m0 = render(rows, cols, c0)
    z1, m1 = render(rows, cols, c1, motion() if moved else None)
    return z0, m0.astype(np.int32), z1, m1.astype(np.int32), c0, c1


def with_wall_patch(rows, cols, pair):
    """the same pair with a patch of the wall as region 2 of frame 0 and label 2 of frame 1: a region that did not move"""
    z0, l0, z1, l1, c0, c1 = pair
    l0, l1 = l0.copy(), l1.copy()
    r0, r1, k0, k1 = 0, max(rows // 3, 1), 0, max(cols // 3, 1)
    l0[r0:r1, k0:k1] = np.where(l0[r0:r1, k0:k1] == 0, 2, l0[r0:r1, k0:k1])
    l1[r0:r1, k0:k1] = np.where(l1[r0:r1, k0:k1] == 0, 2, l1[r0:r1, k0:k1])
    return z0, l0, z1, l1, c0, c1


def plane_pair(rows, cols, T0=None, T1=None, step=0.005):
    """(z0, l0, z1, l1, c0, c1): a slanted plane that fills both frames, region 1 everywhere, `step` metres nearer in frame 1: the
    scene whose every interior pixel has a normal at any size (three of the six degrees are observable: a step needs damping)"""
    c0, c1 = cam(rows, cols, T0), cam(rows, cols, T1)
    v, u = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    z = 2.0 + 0.004 * u + 0.007 * v
    ones = np.ones((rows, cols), np.int32)
    return (np.round(z * 1000.0) / 1000.0).astype(F), ones, (np.round((z - step) * 1000.0) / 1000.0).astype(F), ones.copy(), c0, c1


MOVING_CAMERA = (pose((0.004, -0.006, 0.003), (0.01, -0.005, 0.004)), pose((-0.003, 0.005, 0.002), (-0.008, 0.006, -0.003)))


def pose_error(W, truth):
    """(rotation angle in rad, translation in m at the body's centre) between a 4x4 W and the true motion"""
    W, truth = np.asarray(W, np.float64), np.asarray(truth, np.float64)
    dR = W[:3, :3] @ truth[:3, :3].T
    ang = float(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))
    return ang, float(np.linalg.norm(W[:3, :3] @ CENTRE + W[:3, 3] - (truth[:3, :3] @ CENTRE + truth[:3, 3])))
