"""Test-side oracle of the signed-distance grid field (SGPMP_COST_GRID_SDF), straight from the definition in include/sgpmp.h:
the distance transform of tests/sdf_oracle.py (brute force, scipy), and the bilinear hinge in torch fp64 whose gradient comes from
autograd.  Shares no code with stoch_gpmp_amd/grid_sdf.py or the kernels."""
import numpy as np
import torch

from tests.sdf_oracle import brute_sdf, scipy_sdf  # noqa: F401  (the transform: the tests reach it through this module)


def field_torch(sdf, xy, cell, offset, margin):
    """-> (h, d) at xy [..., 2] (fp64 torch, may require grad): bilinear interpolation between cell centres, clamp-to-edge, hinge."""
    sdf = torch.as_tensor(sdf, dtype=torch.float64)
    ny, nx = sdf.shape
    u = xy[..., 0] * (1. / cell) + offset[0] - 0.5
    v = xy[..., 1] * (1. / cell) + offset[1] - 0.5
    fu, fv = torch.floor(u).detach(), torch.floor(v).detach()
    fx, fy = u - fu, v - fv
    i0, i1 = fu.clamp(0, nx - 1).long(), (fu + 1).clamp(0, nx - 1).long()
    j0, j1 = fv.clamp(0, ny - 1).long(), (fv + 1).clamp(0, ny - 1).long()
    d = (1 - fy) * ((1 - fx) * sdf[j0, i0] + fx * sdf[j0, i1]) + fy * ((1 - fx) * sdf[j1, i0] + fx * sdf[j1, i1])
    e = margin - d
    return torch.where(e > 0, e, torch.zeros_like(e)), d


def field_and_grad(sdf, xy, cell, offset, margin):
    """numpy in, numpy out: (h [...], d [...], dh/dxy [..., 2]) with the gradient from autograd."""
    x = torch.tensor(np.asarray(xy, dtype=np.float64), requires_grad=True)
    h, d = field_torch(sdf, x, cell, offset, margin)
    g, = torch.autograd.grad(h.sum(), x)
    return h.detach().numpy(), d.detach().numpy(), g.numpy()


def kink_distance(sdf, xy, cell, offset, margin):
    """How far each point is from where the field is not differentiable, on the oracle: (distance in cells to the nearest
    cell-centre line, |d - margin| / cell)."""
    xy = np.asarray(xy, dtype=np.float64)
    u = xy[..., 0] / cell + offset[0] - 0.5
    v = xy[..., 1] / cell + offset[1] - 0.5
    line = np.minimum(np.abs(u - np.rint(u)), np.abs(v - np.rint(v)))
    _, d = field_torch(sdf, torch.tensor(xy), cell, offset, margin)
    return line, np.abs(d.numpy() - margin) / cell


def draw_points(sdf, cell, offset, margin, count, seed, tol, spread=1.1):
    """`count` points over the map and a band around it, redrawn until none lies within `tol` (in cells) of a kink."""
    rng = np.random.default_rng(seed)
    ny, nx = sdf.shape
    lo = np.array([(0 - offset[0]) * cell, (0 - offset[1]) * cell])
    hi = np.array([(nx - offset[0]) * cell, (ny - offset[1]) * cell])
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * spread
    pts = mid + half * rng.uniform(-1, 1, size=(count, 2))
    for _ in range(1000):
        line, lev = kink_distance(sdf, pts, cell, offset, margin)
        bad = (line < tol) | (lev < tol)
        if not bad.any():
            return pts
        pts[bad] = mid + half * rng.uniform(-1, 1, size=(int(bad.sum()), 2))
    raise AssertionError("could not draw points away from the kinks")


# ------------------------------------------------------------------------------------------------ the maps of the tests
MARGIN = 2.0        # of the tests on the 20 x 24 map: four cells, so that a good third of the drawn points has an active hinge


def box_disc_map():
    """20 x 24 cells of 0.5 with a box in the middle and a disc near a corner; offsets (ox, oy) = (10, 12) -- what ObstacleMap gives
    a grid of this shape (its x offset comes from the row count), so the map is not centred: x in [-5, 7), y in [-6, 4)."""
    ny, nx, cell = 20, 24, 0.5
    occ = np.zeros((ny, nx))
    occ[7:13, 10:15] = 1.
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    occ[(jj - 4) ** 2 + (ii - 4) ** 2 <= 6] = 1.
    return occ, cell, (10., 12.)


def small_maps():
    """name -> (occ, cell): the maps small enough for the brute force."""
    rng = np.random.default_rng(7)
    corner = np.zeros((5, 6)); corner[0, 0] = 1.
    two = np.array([[0., 1.], [1., 0.]])
    row = np.zeros((1, 7)); row[0, 2] = 1.; row[0, 3] = 1.
    col = np.zeros((7, 1)); col[5, 0] = 1.
    # the one transform behind grid and volume: runs past a volume's 512-cell capacity along either axis, and columns whose
    # scan meets the sentinel on one side
    long_row = np.zeros((1, 600)); long_row[0, 0] = 1.
    stripes = np.zeros((2, 600)); stripes[0] = 1.
    return {
        "1x1 free": (np.zeros((1, 1)), 0.5),
        "1x1 occupied": (np.ones((1, 1)), 0.5),
        "1x7": (row, 0.1),
        "7x1": (col, 0.1),
        "2x2": (two, 1.0),
        "20x24 box and disc": (box_disc_map()[0], box_disc_map()[1]),
        "corner cell": (corner, 0.3),
        "70x130 random": ((rng.uniform(size=(70, 130)) < 0.3).astype(np.float64), 0.05),
        "1x600": (long_row, 0.1),
        "600x1": (long_row.T.copy(), 0.1),
        "2x600": (stripes, 0.1),
    }


def large_map():
    """300 x 260, 30 % random occupancy plus a free disc and a solid box (distances of many cells)."""
    rng = np.random.default_rng(11)
    occ = (rng.uniform(size=(300, 260)) < 0.3).astype(np.float64)
    jj, ii = np.meshgrid(np.arange(300), np.arange(260), indexing="ij")
    occ[(jj - 100) ** 2 + (ii - 90) ** 2 <= 40 ** 2] = 0.
    occ[180:260, 120:220] = 1.
    return occ, 0.1


def wide_map():
    """3 x 261: wider than one workgroup of 256 threads and not a multiple of 64."""
    rng = np.random.default_rng(13)
    return (rng.uniform(size=(3, 261)) < 0.1).astype(np.float64), 0.2


# ------------------------------------------------------------------------------------------------ GPMP rows of the term
def support_system(means, sdf, cell, offset, margin, sigma):
    """The term's rows of CostCollision.get_linear_system: one per waypoint 1 .. T-1, error h, A = -dh/d means (autograd),
    precision 1 / sigma^2."""
    B, T, d = means.shape
    x = means.detach().clone().requires_grad_(True)
    h, _ = field_torch(sdf, x[:, 1:, :2], cell, offset, margin)
    A = torch.zeros(B, T - 1, T * d, dtype=means.dtype)
    for i in range(T - 1):
        g, = torch.autograd.grad(h[:, i].sum(), x, retain_graph=True)
        A[:, i] = -g.reshape(B, T * d)
    K = (1. / sigma ** 2) * torch.eye(T - 1, dtype=means.dtype).repeat(B, 1, 1)
    return A, h.detach().unsqueeze(-1), K


def inserted_system(means, n_sub, dt, weight, sdf, cell, offset, margin, sigma):
    """... and its rows on the n_sub inserted states of every interval (tests/gpmp_dense_oracle.py: autograd through the Hermite
    interpolation), precision weight / sigma^2."""
    from tests import gpmp_dense_oracle as DO
    A, err = DO.autograd_rows(means, n_sub, dt, lambda fine: field_torch(sdf, fine[..., :2], cell, offset, margin)[0].unsqueeze(-1))
    ins = [f for f in range(err.shape[1]) if f % (n_sub + 1) != 0]
    return DO._system(A[:, ins, 0], err[:, ins, 0], weight / sigma ** 2)


# the planar problem of the GPMP tests: start and goal on opposite sides of the box of box_disc_map, both inside the hinge's reach
# (so that also the one row of a T = 2 problem is active); dt and sigma_coll picked so that the field rows move the oracle's first
# step by >= 0.05 (relative L2) at every tested shape
GPMP_C = dict(n_dof=2, dt=0.1, start=[-1., -1.2, 0., 0.], goal=[3.3, -0.8, 0., 0.],
              cost_sigma_start=1e-2, cost_sigma_gp=0.5, sigma_goal_prior=1e-1, sigma_coll=1e-2,
              sigma_start_init=1e-3, sigma_goal_init=1e-3, sigma_gp_init=20.,
              sigma_start_sample=1e-3, sigma_goal_sample=1e-3, sigma_gp_sample=3.)


def gpmp_means(T, P, seed=4, noise=0.15):
    """P particles on noisy straight lines from the start to the goal, through the box; velocities of the line plus noise."""
    c = GPMP_C
    gen = torch.Generator().manual_seed(seed)
    start, goal = torch.tensor(c["start"], dtype=torch.float64), torch.tensor(c["goal"], dtype=torch.float64)
    w = torch.linspace(0, 1, T, dtype=torch.float64).reshape(1, T, 1)
    means = torch.zeros(P, T, 4, dtype=torch.float64)
    means[..., :2] = start[:2] + (goal[:2] - start[:2]) * w
    means[..., 2:] = (goal[:2] - start[:2]) / ((T - 1) * c["dt"])
    means[..., :2] += noise * torch.randn(P, T, 2, generator=gen, dtype=torch.float64)
    means[..., 2:] += 2. * torch.randn(P, T, 2, generator=gen, dtype=torch.float64)
    return means


def gpmp_systems_fn(sdf, cell, offset, margin, n_sub=0, weight=1., field=True, limits=None, c=None):
    """systems_fn of oracle.gpmp_equiv.OracleGPMP: GP + goal prior (+ the term's rows at the waypoints, + with n_sub > 0 its rows
    on the inserted states, + limit rows from tests/gpmp_dense_oracle.dense_systems)."""
    from oracle import gpmp_equiv as GP
    from tests import gpmp_dense_oracle as DO
    c = GPMP_C if c is None else c
    start, goals = torch.tensor(c["start"], dtype=torch.float64), torch.tensor([c["goal"]], dtype=torch.float64)

    def fn(m, **obs):
        out = [GP.linear_system_gp(m, start, 2, c["dt"], c["cost_sigma_start"], c["cost_sigma_gp"]),
               GP.linear_system_goal_prior(m, goals, m.shape[0], 2, c["sigma_goal_prior"])]
        if field:
            out.append(support_system(m, sdf, cell, offset, margin, c["sigma_coll"]))
            if n_sub > 0 and weight > 0.:
                out.append(inserted_system(m, n_sub, c["dt"], weight, sdf, cell, offset, margin, c["sigma_coll"]))
        if limits is not None:
            out += DO.dense_systems(m, 2, n_sub, c["dt"], **limits)
        return out
    return fn
