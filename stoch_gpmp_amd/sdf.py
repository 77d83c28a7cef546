"""The exact Euclidean signed-distance transform of an occupancy grid or volume in numpy: the host-side twin of the device
transform in csrc/sdf.hip, behind grid_sdf.signed_distance_grid and voxel_sdf.signed_distance_volume.  Separable, one pass per
axis, int64 until the one square root -- the same integers the device carries, so the same doubles come out.
"""
import numpy as np

_NONE = 1 << 40                      # "there is no such cell": above any squared distance, and _NONE + (a - a')^2 fits int64


def clamp(a, hi):
    """Float cell indices -> int64 in [0, hi], NaN to 0: the clamp-to-edge of both fields' interpolation."""
    a = np.where(np.isnan(a), 0., a)
    return np.minimum(np.maximum(a, 0.), hi).astype(np.int64)


def _axis_pass(g, axis):
    """g: squared distances (int64, _NONE: none) -> min over a' along `axis` of (a - a')^2 + g[a'], capped at _NONE."""
    g = np.moveaxis(g, axis, -1)
    n = g.shape[-1]
    idx = np.arange(n, dtype=np.int64)
    d2 = (idx[:, None] - idx[None, :]) ** 2                   # [a, a']
    out = np.empty_like(g)
    for a in range(n):                                        # (a loop over the axis keeps the temporary at the input's size)
        out[..., a] = (g + d2[a]).min(axis=-1)
    return np.moveaxis(np.minimum(out, _NONE), -1, axis)


def _squared_distance(mask):
    """Exact squared Euclidean distance (in cells, an integer) from every cell to the nearest True cell; _NONE: none."""
    g = np.where(mask, 0, _NONE).astype(np.int64)
    for axis in range(mask.ndim):                             # slowest axis first: the device's passes
        g = _axis_pass(g, axis)
    return g


def signed_distance(occ, cell, threshold, max_dim, what):
    """occ [ny, nx] or [nz, ny, nx] -> the signed Euclidean distance at cell centres in world units (float64, occ's shape):
    (sqrt(D2) - 0.5) * cell for a free cell (D2: squared distance between index tuples to the nearest occupied cell) and
    -(sqrt(D2) - 0.5) * cell for an occupied one (D2 to the nearest free cell); +/- cap = cell * sum(shape) where there is no
    such cell.  A cell is occupied when occ > threshold.  `what`: the ValueError's text for an occ that is not of that form with
    every extent in [1, max_dim], or a cell that is not > 0."""
    occ = np.asarray(occ)
    if occ.ndim not in (2, 3) or not all(1 <= n <= max_dim for n in occ.shape) or not cell > 0:
        raise ValueError(what)
    o = occ.astype(np.float64) > float(threshold)
    cap = float(cell) * float(sum(o.shape))
    d2 = np.where(o, _squared_distance(~o), _squared_distance(o))
    s = (np.sqrt(d2.astype(np.float64)) - 0.5) * float(cell)
    s = np.where(d2 >= _NONE, cap, s)
    return np.where(o, -s, s)
