"""Host-side twin (numpy) of the voxel signed-distance field, SGPMP_COST_VOXEL_SDF (include/sgpmp.h has the definition;
csrc/sdf.hip builds the volume on the device, `voxel_sdf_field` in csrc/cost_device.h evaluates it) -- what grid_sdf.py is
for the planar field: the same arithmetic in the same order, for tests, examples and host-side checks.  No reference counterpart.
"""
import numpy as np

from .sdf import clamp, signed_distance

MAX_DIM = 512
_BAD_OCC = ("signed_distance_volume: occ must be [nz, ny, nx] with 1 <= nz, ny, nx <= 512, cell > 0 and a threshold "
            "that is not NaN")


def signed_distance_volume(occ, cell, threshold=0.):
    """occ [nz, ny, nx] -> sdf [nz, ny, nx] (float64): the signed Euclidean distance at cell centres in world units,
    (sqrt(D2) - 0.5) * cell for a free cell (D2: squared distance between index triples to the nearest occupied cell) and
    -(sqrt(D2) - 0.5) * cell for an occupied one (D2 to the nearest free cell); +/- cell * (nx + ny + nz) where there is no such
    cell.  A cell is occupied when occ > threshold."""
    if np.ndim(occ) != 3 or threshold != threshold:
        raise ValueError(_BAD_OCC)
    return signed_distance(occ, cell, threshold, MAX_DIM, _BAD_OCC)


def _interp(sdf, cell, origin, pts):
    """-> (d, grad d [..., 3]) in the dtype of sdf: trilinear, clamp-to-edge, x first, then y, then z (cost_device.h:
    voxel_sdf_distance, operation for operation)."""
    sdf = np.asarray(sdf)
    real = sdf.dtype.type
    pts = np.asarray(pts, dtype=sdf.dtype)
    nz, ny, nx = sdf.shape
    inv = real(1.) / real(cell)
    u = (pts[..., 0] * inv + real(origin[0])) - real(0.5)
    v = (pts[..., 1] * inv + real(origin[1])) - real(0.5)
    w = (pts[..., 2] * inv + real(origin[2])) - real(0.5)
    fu, fv, fw = np.floor(u), np.floor(v), np.floor(w)
    fx, fy, fz = u - fu, v - fv, w - fw
    i0, i1 = clamp(fu, nx - 1), clamp(fu + real(1.), nx - 1)
    j0, j1 = clamp(fv, ny - 1), clamp(fv + real(1.), ny - 1)
    k0, k1 = clamp(fw, nz - 1), clamp(fw + real(1.), nz - 1)
    s000, s001, s010, s011 = sdf[k0, j0, i0], sdf[k0, j0, i1], sdf[k0, j1, i0], sdf[k0, j1, i1]      # s[k][j][i]
    s100, s101, s110, s111 = sdf[k1, j0, i0], sdf[k1, j0, i1], sdf[k1, j1, i0], sdf[k1, j1, i1]
    ax, ay, az = real(1.) - fx, real(1.) - fy, real(1.) - fz
    c00, c01 = ax * s000 + fx * s001, ax * s010 + fx * s011
    c10, c11 = ax * s100 + fx * s101, ax * s110 + fx * s111
    e0, e1 = ay * c00 + fy * c01, ay * c10 + fy * c11
    ddx = (az * (ay * (s001 - s000) + fy * (s011 - s010)) + fz * (ay * (s101 - s100) + fy * (s111 - s110))) * inv
    ddy = (az * (c01 - c00) + fz * (c11 - c10)) * inv
    ddz = (e1 - e0) * inv
    return az * e0 + fz * e1, np.stack((ddx, ddy, ddz), axis=-1)


def distance(sdf, cell, origin, pts):
    """The interpolated signed distance d [...] at points pts [..., 3] of the volume sdf [nz, ny, nx] with offsets
    origin = (ox, oy, oz), in the dtype of `sdf`; a non-finite coordinate gives NaN."""
    with np.errstate(invalid="ignore"):
        return _interp(sdf, cell, origin, pts)[0]


def field(sdf, cell, origin, margin, pts):
    """The term's per-point hinge at pts [..., 3]: -> (h, d, grad) with h = margin - d where positive, else 0, and
    grad [..., 3] = dh/dp (exactly zero where the hinge is inactive).  In the dtype of `sdf`; a non-finite coordinate gives
    NaN in all three.  The field of a configuration is the sum of h over its link points."""
    with np.errstate(invalid="ignore"):
        d, dd = _interp(sdf, cell, origin, pts)
        real = d.dtype.type
        e = real(margin) - d
        off = e <= 0
        nan = np.isnan(e)
        h = np.where(off, real(0.), e)
        g = np.where(off[..., None], real(0.), np.where(nan[..., None], e[..., None], -dd))
    return h, d, g
