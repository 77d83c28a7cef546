"""Host-side twin (numpy) of the body collision spheres on the voxel signed-distance field, SGPMP_COST_BODY_SDF (include/sgpmp.h
has the definition; csrc/body_device.h evaluates it on the device), built on voxel_sdf.py's distance, operation for operation:
for tests, examples and host-side checks.  No reference counterpart.  `body` is a robots.body.BodySpheres (or anything with
`links`, `centers`, `radii`)."""
from math import cos, sin

import numpy as np

from . import voxel_sdf


def body_points(frames, body):
    """Link frames [..., L, 4, 4] -> world centres of the body's spheres [..., M, 3]: p_m = P_l + R_l c_m."""
    frames = np.asarray(frames)
    real = frames.dtype.type
    links = np.asarray(body.links, dtype=np.int64)
    if links.max() >= frames.shape[-3]:
        raise ValueError("body_points: the body has a sphere on a link past the given frames")
    c = np.asarray(body.centers, dtype=frames.dtype)
    F = np.take(frames, links, axis=-3)
    R, P = F[..., :3, :3], F[..., :3, 3]
    rot = (R[..., 0] * c[:, 0, None] + R[..., 1] * c[:, 1, None]) + R[..., 2] * c[:, 2, None]
    return P + rot.astype(real)


def clearance(sdf, cell, origin, frames, body):
    """-> s [..., M] = d(p_m) - r_m, in the dtype of `sdf`; a non-finite coordinate gives NaN."""
    sdf = np.asarray(sdf)
    pts = body_points(np.asarray(frames, dtype=sdf.dtype), body)
    return voxel_sdf.distance(sdf, cell, origin, pts) - np.asarray(body.radii, dtype=sdf.dtype)


def field(sdf, cell, origin, margin, frames, body):
    """-> (f [...], h [..., M], s [..., M], g [..., M, 3]): h_m = (margin + r_m) - d(p_m) where positive, else 0, f = sum_m h_m
    in table order, s_m the clearance and g_m = dh_m/dp_m (exactly zero where the hinge is inactive).  In the dtype of `sdf`."""
    sdf = np.asarray(sdf)
    real = sdf.dtype.type
    pts = body_points(np.asarray(frames, dtype=sdf.dtype), body)
    r = np.asarray(body.radii, dtype=sdf.dtype)
    with np.errstate(invalid="ignore"):
        d, dd = voxel_sdf._interp(sdf, cell, origin, pts)
        e = (real(margin) + r) - d
        off = e <= 0
        nan = np.isnan(e)
        h = np.where(off, real(0.), e)
        g = np.where(off[..., None], real(0.), np.where(nan[..., None], e[..., None], -dd))
        f = np.zeros(h.shape[:-1], dtype=sdf.dtype)
        for m in range(h.shape[-1]):
            f = f + h[..., m]
    return f, h, d - r, g


def _rpy(rpy):
    r, p, y = (float(v) for v in rpy)
    cr, sr, cp, sp, cy, sy = cos(r), sin(r), cos(p), sin(p), cos(y), sin(y)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]])


def link_frames(q, chain, dtype=np.float64):
    """q [B, n] -> (frames [B, L, 4, 4], z [B, J, 3], o [B, J, 3]): sgpmp_fk's link frames of the chain [(name, 'revolute' |
    'fixed', rpy, xyz)] -- H_child = H_parent Trans(xyz) RPY(rpy) Rz(q) -- and every joint's axis and origin in the world."""
    q = np.asarray(q, dtype=dtype)
    B, J = q.shape[0], len(chain)
    R = np.broadcast_to(np.eye(3, dtype=dtype), (B, 3, 3)).copy()
    p = np.zeros((B, 3), dtype=dtype)
    frames = np.zeros((B, J + 1, 4, 4), dtype=dtype)
    frames[:, :, 3, 3] = 1.
    frames[:, 0, :3, :3] = R
    z, o = np.zeros((B, J, 3), dtype=dtype), np.zeros((B, J, 3), dtype=dtype)
    k = 0
    for j, (_, kind, rpy, xyz) in enumerate(chain):
        p = p + R @ np.asarray(xyz, dtype=dtype)
        R = R @ _rpy(rpy).astype(dtype)
        z[:, j], o[:, j] = R[:, :, 2], p
        if kind == "revolute":
            with np.errstate(invalid="ignore"):          # (a non-finite joint value: NaN from here on)
                c, s = np.cos(q[:, k]), np.sin(q[:, k])
            a, b = R[:, :, 0].copy(), R[:, :, 1].copy()
            R = R.copy()
            R[:, :, 0] = a * c[:, None] + b * s[:, None]
            R[:, :, 1] = b * c[:, None] - a * s[:, None]
            k += 1
        frames[:, j + 1, :3, :3], frames[:, j + 1, :3, 3] = R, p
    return frames, z, o


def config_field(sdf, cell, origin, margin, q, chain, body):
    """q [B, n] -> (f [B], df/dq [B, n], min_m s_m [B], its gradient through the first arg-min sphere [B, n]), in the dtype of
    `sdf`: df/dq_j = sum over the spheres on links behind revolute joint j of z_j . ((p_m - o_j) x g_m).  A NaN clearance
    anywhere makes the value and every gradient entry NaN."""
    sdf = np.asarray(sdf)
    frames, z, o = link_frames(q, chain, sdf.dtype)
    f, h, s, g = field(sdf, cell, origin, margin, frames, body)
    pts = body_points(frames, body)
    with np.errstate(invalid="ignore"):
        dd = voxel_sdf._interp(sdf, cell, origin, pts)[1]
    links = np.asarray(body.links)
    B, n = frames.shape[0], sum(1 for j in chain if j[1] == "revolute")
    rows = np.arange(B)
    with np.errstate(invalid="ignore"):
        best = np.zeros(B, dtype=np.int64)           # first arg-min, strict comparison (np.argmin would pick a NaN)
        smin = np.full(B, np.inf, dtype=sdf.dtype)
        for m in range(len(links)):
            better = s[:, m] < smin
            smin = np.where(better, s[:, m], smin)
            best = np.where(better, m, best)
    grad, gmin = np.zeros((B, n), dtype=sdf.dtype), np.zeros((B, n), dtype=sdf.dtype)
    k = 0
    for j, (_, kind, _, _) in enumerate(chain):
        if kind != "revolute":
            continue
        for m in np.nonzero(links > j)[0]:
            grad[:, k] += np.einsum("bi,bi->b", z[:, j], np.cross(pts[:, m] - o[:, j], g[:, m]))
        behind = links[best] > j
        t = np.einsum("bi,bi->b", z[:, j], np.cross(pts[rows, best] - o[:, j], dd[rows, best]))
        gmin[:, k] = np.where(behind, t, 0.)
        k += 1
    nan = np.isnan(s).any(-1)
    f = np.where(nan, np.nan, f)
    grad[nan], gmin[nan] = np.nan, np.nan
    smin = np.where(nan, np.nan, smin)
    return f, grad, smin, gmin
