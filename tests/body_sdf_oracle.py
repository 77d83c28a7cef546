"""Test-side oracle of the body collision spheres on the voxel signed-distance field (SGPMP_COST_BODY_SDF), straight from the
definition in include/sgpmp.h, in torch fp64: body points from oracle/fk.py's link frames, distance and hinge from
tests/voxel_sdf_oracle.py with the per-sphere margin + r, gradients from autograd through the FK.  Shares no code with
stoch_gpmp_amd/body_sdf.py, robots/body.py or the kernels."""
import numpy as np
import torch

from oracle import ref_equiv as R
from oracle.fk import fk_all_links
from tests import voxel_sdf_oracle as VO
from tests.voxel_sdf_oracle import ARM_C, CHAINS, arm_scene, draw_configs, gpmp_means  # noqa: F401  (the tests' scene and problem)


def body_tensors(body):
    """(links [M] long, centres [M, 3], radii [M]) of anything with .links / .centers / .radii, or of a (links, table [M, 4])."""
    if isinstance(body, tuple):
        links, table = body
        table = torch.as_tensor(np.asarray(table, dtype=np.float64))
        return torch.as_tensor(np.asarray(links)).long(), table[:, :3], table[:, 3]
    return (torch.tensor(list(body.links)).long(), torch.tensor([list(c) for c in body.centers], dtype=torch.float64),
            torch.tensor(list(body.radii), dtype=torch.float64))


def frames_points(frames, body):
    """Link frames [..., L, 4, 4] -> sphere centres in the world [..., M, 3]."""
    links, c, _ = body_tensors(body)
    F = frames[..., links, :, :]
    return F[..., :3, 3] + (F[..., :3, :3] @ c.to(frames.dtype).unsqueeze(-1)).squeeze(-1)


def frames_field(frames, body, scene):
    """-> f [...] = sum_m hinge((margin + r_m) - d(p_m))."""
    _, _, r = body_tensors(body)
    pts = frames_points(frames, body)
    return VO.hinge_torch(scene["sdf"], pts, scene["cell"], scene["origin"], scene["margin"] + r)[0].sum(-1)


def frames_clearance(frames, body, scene):
    """-> s [..., M] = d(p_m) - r_m."""
    _, _, r = body_tensors(body)
    return VO.distance_torch(scene["sdf"], frames_points(frames, body), scene["cell"], scene["origin"]) - r


def config_field_and_grad(q, chain, body, scene):
    """q [B, n] numpy -> (f [B], df/dq [B, n], min_m s_m [B], its gradient [B, n], s [B, M]), gradients from autograd."""
    x = torch.tensor(np.asarray(q, dtype=np.float64), requires_grad=True)
    frames = fk_all_links(x, chain)
    f = frames_field(frames, body, scene)
    g, = torch.autograd.grad(f.sum(), x, retain_graph=True)
    s = frames_clearance(frames, body, scene)
    smin = s.min(-1)[0]
    gs, = torch.autograd.grad(smin.sum(), x)
    return f.detach().numpy(), g.numpy(), smin.detach().numpy(), gs.numpy(), s.detach().numpy()


def regular(q, chain, body, scene, delta):
    """Mask of the configurations with no body point within `delta` cells of a cell-centre plane and no
    |margin + r_m - d| < delta * cell: where the field's gradient is continuous."""
    _, _, r = body_tensors(body)
    pts = frames_points(fk_all_links(torch.as_tensor(np.asarray(q, dtype=np.float64)), chain), body)
    cell, origin = scene["cell"], scene["origin"]
    u = torch.stack([pts[..., a] / cell + origin[a] - 0.5 for a in range(3)], -1)
    plane = (u - torch.round(u)).abs().amin((-1, -2))
    d = VO.distance_torch(scene["sdf"], pts, cell, origin)
    level = ((scene["margin"] + r - d).abs() / cell).amin(-1)
    return ((plane >= delta) & (level >= delta)).numpy()


def argmin_gap(s):
    """s [B, M] -> the gap between the smallest and the second smallest clearance [B] (inf for M = 1)."""
    if s.shape[1] < 2:
        return np.full(s.shape[0], np.inf)
    part = np.sort(s, axis=1)
    return part[:, 1] - part[:, 0]


def sweep_term(trajs, n, chain, body, scene, sigma):
    """trajs [B, T, 2n] torch fp64 -> the term of a cost list [B]: 1 / sigma^2 * sum over t = 1 .. T-1 of f(q_t)."""
    B, T = trajs.shape[0], trajs.shape[1]
    if T < 2:
        return torch.zeros(B, dtype=torch.float64)
    q = trajs[:, 1:, :n].reshape(-1, n)
    f = frames_field(fk_all_links(q, chain), body, scene).reshape(B, T - 1)
    return f.sum(-1) / sigma ** 2


def gpmp_systems_fn(scene, body, chain=None, n_sub=0, weight=1., field=True, c=None):
    """systems_fn of oracle.gpmp_equiv.OracleGPMP: GP + goal prior (+ the term's rows at the waypoints 1 .. T-1: error f, A = -df/dq
    by autograd through FK, precision 1 / sigma^2; + with n_sub > 0 its rows on the inserted states, precision weight / sigma^2)."""
    from oracle import gpmp_equiv as GP
    from tests import gpmp_dense_oracle as DO
    c = ARM_C if c is None else c
    chain = CHAINS["panda"][0] if chain is None else chain
    n = c["n_dof"]
    start = torch.tensor(c["start_q"] + [0.] * n, dtype=torch.float64)
    goals = torch.tensor([c["goal_q"] + [0.] * n], dtype=torch.float64)
    fk = lambda q: fk_all_links(q, chain)                                               # noqa: E731
    fn_field = lambda fr: frames_field(fr, body, scene)                                 # noqa: E731

    def fn(m, **obs):
        out = [GP.linear_system_gp(m, start, n, c["dt"], c["cost_sigma_start"], c["cost_sigma_gp"]),
               GP.linear_system_goal_prior(m, goals, m.shape[0], n, c["sigma_goal_prior"])]
        if field:
            out.append(R.collision_linear_system(m, n, fk, fn_field, c["sigma_coll"]))
            if n_sub > 0 and weight > 0.:
                out.append(DO.collision_system(m, n, n_sub, c["dt"], weight, fn_field, c["sigma_coll"], FK=fk))
        return out
    return fn
