"""Host-side twin (numpy) of the signed-distance grid field, SGPMP_COST_GRID_SDF (include/sgpmp.h has the definition;
csrc/sdf.hip builds the grid on the device, `grid_sdf_field` in csrc/cost_device.h evaluates it) -- what dense.py is for
the dense trajectories: the same arithmetic in the same order, for tests, examples and host-side checks.  No reference
counterpart: the reference's ObstacleMap is occupancy only.
"""
import numpy as np

from .sdf import clamp, signed_distance

MAX_DIM = 4096
_BAD_OCC = "signed_distance_grid: occ must be [ny, nx] with 1 <= ny, nx <= 4096 and cell > 0"


def signed_distance_grid(occ, cell, threshold=0.):
    """occ [ny, nx] -> sdf [ny, nx] (float64): the signed Euclidean distance at cell centres in world units, (D - 0.5) * cell
    for a free cell (D: distance between index pairs to the nearest occupied cell) and -(D - 0.5) * cell for an occupied one
    (D to the nearest free cell); +/- cell * (nx + ny) where there is no such cell.  A cell is occupied when occ > threshold."""
    if np.ndim(occ) != 2:
        raise ValueError(_BAD_OCC)
    return signed_distance(occ, cell, threshold, MAX_DIM, _BAD_OCC)


def field(sdf, xy, cell, offset, margin):
    """The term at points xy [..., 2] of the grid sdf [ny, nx] with offsets (ox, oy): -> (h, d, grad) with d [...] the bilinear,
    clamp-to-edge interpolation between cell centres, h = margin - d where positive, else 0, and grad [..., 2] = dh/d(x, y)
    (exactly zero where the hinge is inactive).  In the dtype of `sdf`; non-finite points give NaN in all three."""
    sdf = np.asarray(sdf)
    real = sdf.dtype.type
    xy = np.asarray(xy, dtype=sdf.dtype)
    ny, nx = sdf.shape
    inv = real(1.) / real(cell)
    with np.errstate(invalid="ignore"):
        u = (xy[..., 0] * inv + real(offset[0])) - real(0.5)
        v = (xy[..., 1] * inv + real(offset[1])) - real(0.5)
        fu, fv = np.floor(u), np.floor(v)
        fx, fy = u - fu, v - fv
        i0, i1 = clamp(fu, nx - 1), clamp(fu + real(1.), nx - 1)
        j0, j1 = clamp(fv, ny - 1), clamp(fv + real(1.), ny - 1)
        s00, s10, s01, s11 = sdf[j0, i0], sdf[j0, i1], sdf[j1, i0], sdf[j1, i1]
        ax, ay = real(1.) - fx, real(1.) - fy
        d = ay * (ax * s00 + fx * s10) + fy * (ax * s01 + fx * s11)
        e = real(margin) - d
        off = e <= 0
        ddx = (ay * (s10 - s00) + fy * (s11 - s01)) * inv
        ddy = (ax * (s01 - s00) + fx * (s11 - s10)) * inv
        nan = np.isnan(e)
        h = np.where(off, real(0.), e)
        gx = np.where(off, real(0.), np.where(nan, e, -ddx))
        gy = np.where(off, real(0.), np.where(nan, e, -ddy))
    return h, d, np.stack((gx, gy), axis=-1)
