"""Test-side oracle of the signed-distance transform behind SGPMP_COST_GRID_SDF and SGPMP_COST_VOXEL_SDF, straight from the
definition in include/sgpmp.h, for an occupancy array of any number of axes: a brute-force numpy distance transform and scipy's
exact transform.  Shares no code with stoch_gpmp_amd/ or the kernels."""
import numpy as np


def brute_sdf(occ, cell, threshold=0.):
    """Every cell against every cell of the other kind: integer squared index distances, one sqrt in double, (D - 0.5) * cell;
    +/- cell * (the sum of the extents) where there is no cell of the other kind."""
    o = np.asarray(occ, dtype=np.float64) > threshold
    cap = cell * sum(o.shape)
    pts = np.stack([g.ravel() for g in np.meshgrid(*(np.arange(n) for n in o.shape), indexing="ij")], 1).astype(np.int64)
    flat = o.ravel()
    out = np.empty(flat.size)
    for kind in (False, True):                                 # cells of this kind look for the nearest cell of the other
        mine, other = pts[flat == kind], pts[flat != kind]
        if len(mine) == 0:
            continue
        if len(other) == 0:
            out[flat == kind] = -cap if kind else cap
            continue
        best = np.empty(len(mine), dtype=np.int64)
        for a in range(0, len(mine), 256):
            d = mine[a:a + 256, None, :] - other[None, :, :]
            best[a:a + 256] = (d * d).sum(-1).min(1)
        s = (np.sqrt(best.astype(np.float64)) - 0.5) * cell
        out[flat == kind] = -s if kind else s
    return out.reshape(o.shape)


def scipy_sdf(occ, cell, threshold=0.):
    """The same from scipy's exact Euclidean transform (for inputs where the brute force is slow)."""
    from scipy.ndimage import distance_transform_edt
    o = np.asarray(occ, dtype=np.float64) > threshold
    cap = cell * sum(o.shape)
    if not o.any():
        return np.full(o.shape, cap)
    if o.all():
        return np.full(o.shape, -cap)
    # (squared integer distances back from the transform's doubles: exact below 2^53, so the one sqrt is the definition's)
    d_out = np.rint(distance_transform_edt(~o) ** 2)
    d_in = np.rint(distance_transform_edt(o) ** 2)
    return np.where(o, -(np.sqrt(d_in) - 0.5) * cell, (np.sqrt(d_out) - 0.5) * cell)
