"""Test-side oracle of the voxel signed-distance field (SGPMP_COST_VOXEL_SDF), straight from the definition in include/sgpmp.h:
the distance transform of tests/sdf_oracle.py (brute force, scipy), and the trilinear hinge over the link points in torch fp64 whose
gradient comes from autograd through oracle/fk.py.  Shares no code with stoch_gpmp_amd/voxel_sdf.py or the kernels."""
import numpy as np
import torch

from oracle import ref_equiv as R
from oracle.fk import PANDA_CHAIN, fk_all_links
from tests.sdf_oracle import brute_sdf, scipy_sdf  # noqa: F401  (the transform: the tests reach it through this module)


# ------------------------------------------------------------------------------------------------ the field
def distance_torch(sdf, pts, cell, origin):
    """-> d at pts [..., 3] (fp64 torch, may require grad): trilinear between cell centres (x, then y, then z), clamp-to-edge."""
    sdf = torch.as_tensor(sdf, dtype=torch.float64)
    nz, ny, nx = sdf.shape
    frac, lo, hi = [], [], []
    for a, n in ((0, nx), (1, ny), (2, nz)):
        u = pts[..., a] * (1. / cell) + origin[a] - 0.5
        fu = torch.floor(u).detach()
        frac.append(u - fu)
        lo.append(fu.clamp(0, n - 1).long())
        hi.append((fu + 1).clamp(0, n - 1).long())
    (fx, fy, fz), (i0, j0, k0), (i1, j1, k1) = frac, lo, hi
    e = []
    for k in (k0, k1):
        c = [(1 - fx) * sdf[k, j, i0] + fx * sdf[k, j, i1] for j in (j0, j1)]
        e.append((1 - fy) * c[0] + fy * c[1])
    return (1 - fz) * e[0] + fz * e[1]


def hinge_torch(sdf, pts, cell, origin, margin):
    """-> (h, d) per point."""
    d = distance_torch(sdf, pts, cell, origin)
    e = margin - d
    return torch.where(e > 0, e, torch.zeros_like(e)), d


def point_field_and_grad(sdf, pts, cell, origin, margin):
    """numpy in, numpy out: (h [...], d [...], dh/dp [..., 3]) per point, the gradient from autograd."""
    x = torch.tensor(np.asarray(pts, dtype=np.float64), requires_grad=True)
    h, d = hinge_torch(sdf, x, cell, origin, margin)
    g, = torch.autograd.grad(h.sum(), x)
    return h.detach().numpy(), d.detach().numpy(), g.numpy()


def link_points(q, chain, num_interpolate=0, link_range=(5, 7)):
    """q [B, n] (torch fp64) -> the term's points [B, np, 3]: every link origin, then the interpolated points."""
    return R._link_points(fk_all_links(q, chain), num_interpolate, link_range)


def frames_field(frames, scene, num_interpolate=0, link_range=(5, 7)):
    """Link frames [..., L, 4, 4] -> the field f [...] = sum over the points of the hinge."""
    pts = R._link_points(frames, num_interpolate, link_range)
    return hinge_torch(scene["sdf"], pts, scene["cell"], scene["origin"], scene["margin"])[0].sum(-1)


def config_field_and_grad(q, chain, scene, num_interpolate=0, link_range=(5, 7)):
    """q [B, n] numpy -> (f [B], df/dq [B, n], min_p d [B], its gradient [B, n]) in fp64, gradients from autograd through FK."""
    x = torch.tensor(np.asarray(q, dtype=np.float64), requires_grad=True)
    pts = link_points(x, chain, num_interpolate, link_range)
    h, d = hinge_torch(scene["sdf"], pts, scene["cell"], scene["origin"], scene["margin"])
    f = h.sum(-1)
    g, = torch.autograd.grad(f.sum(), x, retain_graph=True)
    dmin = d.min(-1)[0]
    gd, = torch.autograd.grad(dmin.sum(), x)
    return f.detach().numpy(), g.numpy(), dmin.detach().numpy(), gd.numpy()


def kink_distance(q, chain, scene, num_interpolate=0, link_range=(5, 7)):
    """Per configuration, how far its points stay from where the field is not differentiable: (smallest distance in cells of a
    point to a cell-centre plane, smallest |margin - d| / cell)."""
    pts = link_points(torch.as_tensor(np.asarray(q, dtype=np.float64)), chain, num_interpolate, link_range)
    cell, origin = scene["cell"], scene["origin"]
    u = torch.stack([pts[..., a] / cell + origin[a] - 0.5 for a in range(3)], -1)
    plane = (u - torch.round(u)).abs().amin((-1, -2))
    d = distance_torch(scene["sdf"], pts, cell, origin)
    return plane.numpy(), ((d - scene["margin"]).abs() / cell).amin(-1).numpy()


# ------------------------------------------------------------------------------------------------ the volumes of the tests
def hollow_box():
    occ = np.zeros((6, 7, 8))
    occ[1:5, 1:6, 1:7] = 1.
    occ[2:4, 2:5, 2:6] = 0.
    return occ


def small_volumes():
    """name -> (occ [nz, ny, nx], cell): small enough for the brute force; three different extents catch axis mix-ups."""
    rng = np.random.default_rng(7)
    line = np.zeros((1, 1, 5)); line[0, 0, 1] = 1.
    single = np.zeros((3, 4, 5)); single[1, 2, 3] = 1.
    return {
        "1x1x1 free": (np.zeros((1, 1, 1)), 0.5),
        "1x1x1 occupied": (np.ones((1, 1, 1)), 0.5),
        "1x1x5": (line, 0.1),
        "3x4x5 random": ((rng.uniform(size=(3, 4, 5)) < 0.3).astype(np.float64), 0.2),
        "3x4x5 all free": (np.zeros((3, 4, 5)), 0.25),
        "3x4x5 all occupied": (np.ones((3, 4, 5)), 0.25),
        "3x4x5 single cell": (single, 0.3),
        "6x7x8 hollow box": (hollow_box(), 0.1),
        "9x10x11 random": ((rng.uniform(size=(9, 10, 11)) < 0.2).astype(np.float64), 0.05),
    }


def large_volume():
    """40 x 33 x 70, 2 % random occupancy plus a free ball and a solid box (distances of many cells)."""
    rng = np.random.default_rng(11)
    occ = (rng.uniform(size=(40, 33, 70)) < 0.02).astype(np.float64)
    kk, jj, ii = np.meshgrid(np.arange(40), np.arange(33), np.arange(70), indexing="ij")
    occ[(kk - 20) ** 2 + (jj - 15) ** 2 + (ii - 25) ** 2 <= 12 ** 2] = 0.
    occ[5:30, 8:28, 45:65] = 1.
    return occ, 0.1


def mapping_volumes(tile_y=8):
    """Shapes that cross the kernels' mapping boundaries: nx past one wave / past a 256-thread workgroup / past the y pass's
    32-column tile, ny and nz one above the y pass's row-group count, a line along x and a line along z."""
    rng = np.random.default_rng(13)
    shapes = {"2x3x70": (2, 3, 70), "2x2x300": (2, 2, 300), "3x9x33": (3, tile_y + 1, 33), "9x3x5": (tile_y + 1, 3, 5),
              "1x1x130": (1, 1, 130), "130x1x1": (130, 1, 1), "1x70x1": (1, 70, 1)}
    out = {k: ((rng.uniform(size=s) < 0.08).astype(np.float64), 0.2) for k, s in shapes.items()}
    # the one transform behind grid and volume: a squared distance of 99^2 = 9801, past the grid's sentinel of 8192, along each
    # axis; and a line with no occupied cell at all (the cap)
    for name, shape in (("100x1x1", (100, 1, 1)), ("1x100x1", (1, 100, 1)), ("1x1x100", (1, 1, 100))):
        occ = np.zeros(shape)
        occ.flat[0] = 1.
        out[name] = (occ, 0.2)
    out["1x1x100 all free"] = (np.zeros((1, 1, 100)), 0.2)
    return out


# The arm scene: 10 x 14 x 13 cells of 0.08 over x in [-0.4, 0.64), y in [-0.5, 0.62), z in [0, 0.8) -- the Panda and the toy
# chain reach out of it on every side -- with a box in front of the base and a ball beside it.  The chains' fixed points (the base
# at the origin, the first joint above it) sit away from the cell-centre planes and further than the margin from both obstacles.
TOY_CHAIN = [("j1", "revolute", (0.0, 0.0, 0.0), (0.0, 0.0, 0.21)), ("j2", "revolute", (1.3, 0.0, 0.0), (0.0, 0.0, 0.13)),
             ("j3", "revolute", (0.0, 0.4, 0.0), (0.37, 0.0, 0.0)), ("tip", "fixed", (0.0, 0.0, 0.3), (0.33, 0.05, 0.0))]
CHAINS = {"toy": (TOY_CHAIN, 3, (1, 3)), "panda": (PANDA_CHAIN, 7, (5, 7))}      # chain, n, link_interpolate_range
MARGIN = 0.15


def arm_scene(margin=MARGIN):
    nz, ny, nx, cell, lower = 10, 14, 13, 0.08, (-0.4, -0.5, 0.0)
    occ = np.zeros((nz, ny, nx))
    occ[3:8, 4:10, 8:12] = 1.                                  # box: x [0.24, 0.56), y [-0.18, 0.30), z [0.24, 0.64)
    kk, jj, ii = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    occ[(kk - 7) ** 2 + (jj - 11) ** 2 + (ii - 3) ** 2 <= 4] = 1.   # ball about (-0.12, 0.42, 0.60)
    return dict(occ=occ, cell=cell, lower=lower, origin=tuple(-c / cell for c in lower), margin=margin,
                sdf=brute_sdf_cached(occ, cell))


_CACHE = {}


def brute_sdf_cached(occ, cell):
    key = (occ.tobytes(), occ.shape, cell)
    if key not in _CACHE:
        _CACHE[key] = brute_sdf(occ, cell)
    return _CACHE[key]


def draw_configs(which, B, seed):
    """B seeded joint configurations of chain `which`, uniform in [-2.6, 2.6] (Panda: inside its joint limits' box, roughly)."""
    n = CHAINS[which][1]
    return np.random.default_rng(seed).uniform(-2.6, 2.6, size=(B, n))


def regular(q, chain, scene, delta, num_interpolate=0, link_range=(5, 7)):
    """Mask of the configurations none of whose points lies within `delta` cells of a cell-centre plane or has
    |margin - d| < delta * cell: where the gradient is continuous."""
    plane, level = kink_distance(q, chain, scene, num_interpolate, link_range)
    return (plane >= delta) & (level >= delta)


# ------------------------------------------------------------------------------------------------ GPMP rows of the term
# The Panda problem of the GPMP tests in arm_scene: the hand passes the box's front face within the hinge's reach, so the term's
# rows are active from the first iteration (also the one row of a T = 2 problem); sigma_gp and sigma_coll picked on the oracle so
# that the field rows move its first step by >= 0.05 (relative L2) at every tested shape.
ARM_C = dict(n_dof=7, dt=0.1, start_q=[-0.5, 0.6, 0., -1.6, 0., 2.2, 0.7], goal_q=[0.6, 0.5, 0.1, -1.7, 0., 2.2, 0.7],
             cost_sigma_start=1e-2, cost_sigma_gp=0.5, sigma_goal_prior=1e-1, sigma_coll=2e-2,
             sigma_start_init=1e-3, sigma_goal_init=1e-3, sigma_gp_init=1., sigma_start_sample=1e-3, sigma_goal_sample=1e-3,
             sigma_gp_sample=0.1)


def gpmp_means(T, P, seed=4, noise=0.05):
    """P particles on noisy straight lines in joint space from the start to the goal; velocities of the line plus noise."""
    c = ARM_C
    gen = torch.Generator().manual_seed(seed)
    q0, q1 = torch.tensor(c["start_q"], dtype=torch.float64), torch.tensor(c["goal_q"], dtype=torch.float64)
    w = torch.linspace(0, 1, T, dtype=torch.float64).reshape(1, T, 1)
    means = torch.zeros(P, T, 14, dtype=torch.float64)
    means[..., :7] = q0 + (q1 - q0) * w + noise * torch.randn(P, T, 7, generator=gen, dtype=torch.float64)
    means[..., 7:] = (q1 - q0) / ((T - 1) * c["dt"]) + 0.3 * torch.randn(P, T, 7, generator=gen, dtype=torch.float64)
    return means


def gpmp_systems_fn(scene, n_sub=0, weight=1., field=True, c=None, num_interpolate=0):
    """systems_fn of oracle.gpmp_equiv.OracleGPMP: GP + goal prior (+ the term's rows at the waypoints 1 .. T-1: error f, A = -df/dq
    by autograd through FK, precision 1 / sigma^2; + with n_sub > 0 its rows on the inserted states, precision weight / sigma^2)."""
    from oracle import gpmp_equiv as GP
    from tests import gpmp_dense_oracle as DO
    c = ARM_C if c is None else c
    n = c["n_dof"]
    start = torch.tensor(c["start_q"] + [0.] * n, dtype=torch.float64)
    goals = torch.tensor([c["goal_q"] + [0.] * n], dtype=torch.float64)
    fn_field = lambda fr: frames_field(fr, scene, num_interpolate)                       # noqa: E731

    def fn(m, **obs):
        out = [GP.linear_system_gp(m, start, n, c["dt"], c["cost_sigma_start"], c["cost_sigma_gp"]),
               GP.linear_system_goal_prior(m, goals, m.shape[0], n, c["sigma_goal_prior"])]
        if field:
            out.append(R.collision_linear_system(m, n, fk_all_links, fn_field, c["sigma_coll"]))
            if n_sub > 0 and weight > 0.:
                out.append(DO.collision_system(m, n, n_sub, c["dt"], weight, fn_field, c["sigma_coll"]))
        return out
    return fn
