"""Generate tests/golden/*.npz by RUNNING THE REFERENCE ITSELF (imported from /root/reference).

Run only in the build container (the reference does not exist on the GPU box):

    python oracle/gen_golden.py

The reference is imported unmodified.  Its one missing third-party import
(`torch_robotics...utils.SE3_distance`, reference costs/fields.py:4, used only by
EESE3DistanceField which is out of scope) is satisfied by an empty stub module so that
`LinkDistanceField` / `LinkSelfDistanceField` can be imported.  Noise is captured by wrapping
`torch.distributions.multivariate_normal._standard_normal`, so the committed eps tensors are
exactly what the reference consumed, in call order.

Fixtures hold data only: inputs, captured noise and the reference's outputs.
"""
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)
sys.path.insert(0, "/root/reference")

import matplotlib  # noqa: E402
matplotlib.use("Agg")
for _name in ("torch_robotics", "torch_robotics.torch_kinematics_tree",
              "torch_robotics.torch_kinematics_tree.geometrics",
              "torch_robotics.torch_kinematics_tree.geometrics.utils"):
    sys.modules[_name] = types.ModuleType(_name)
sys.modules["torch_robotics.torch_kinematics_tree.geometrics.utils"].SE3_distance = None

import torch.distributions.multivariate_normal as _mvn  # noqa: E402
from stoch_gpmp.planner import StochGPMP  # noqa: E402
from stoch_gpmp.costs.cost_functions import (CostCollision, CostComposite, CostGP,  # noqa: E402
                                             CostGoalPrior)
from stoch_gpmp.costs.factors.mp_priors_multi import MultiMPPrior  # noqa: E402
from stoch_gpmp.costs.factors.gp_factor import GPFactor  # noqa: E402
from stoch_gpmp.costs.factors.unary_factor import UnaryFactor  # noqa: E402
from stoch_gpmp.costs.fields import LinkDistanceField, LinkSelfDistanceField  # noqa: E402
from stoch_gpmp.envs.map_generator import generate_obstacle_map  # noqa: E402
from stoch_gpmp.envs.obst_map import ObstacleMap  # noqa: E402

from oracle.fk import fk_all_links  # noqa: E402

F64 = {"device": torch.device("cpu"), "dtype": torch.float64}
F32 = {"device": torch.device("cpu"), "dtype": torch.float32}


class NoiseTap:
    """Records every standard-normal draw torch's MultivariateNormal makes."""

    def __enter__(self):
        self.draws = []
        self._orig = _mvn._standard_normal

        def tapped(shape, dtype, device):
            e = self._orig(shape, dtype=dtype, device=device)
            self.draws.append(e.clone())
            return e
        _mvn._standard_normal = tapped
        return self

    def __exit__(self, *a):
        _mvn._standard_normal = self._orig


def npy(t):
    return t.detach().cpu().numpy().copy()      # copy: the planner updates its means in place


def planar_scene(tensor_args):
    random.seed(0)
    np.random.seed(0)
    return generate_obstacle_map(map_dim=[20, 20], obst_list=[], cell_size=0.1, random_gen=True,
                                 num_obst=15, rand_limits=[[-7.5, 7.5], [-7.5, 7.5]],
                                 rand_rect_shape=[2, 2], tensor_args=tensor_args)[0]


PLANAR = dict(n_dof=2, dt=0.02, start=[-9., -9., 0., 0.],
              cost_sigma_start=1e-3, cost_sigma_gp=0.1, sigma_coll=1e-5, sigma_goal_prior=1e-3,
              sigma_start_init=1e-3, sigma_goal_init=1e-3, sigma_gp_init=20.,
              sigma_start_sample=1e-3, sigma_goal_sample=1e-3, sigma_gp_sample=3.,
              step_size=0.5, temperature=1.)


def build_planar(obst_map, T, goals, nppg, S, seed, ta, initial_particle_means=None,
                 temperature=None, **overrides):
    c = dict(PLANAR, **overrides)
    start = torch.tensor(c["start"], **ta)
    goals_t = torch.tensor(goals, **ta)
    cost = CostComposite(c["n_dof"], T, [
        CostGP(c["n_dof"], T, start, c["dt"],
               dict(sigma_start=c["cost_sigma_start"], sigma_gp=c["cost_sigma_gp"]), ta),
        CostGoalPrior(c["n_dof"], T, multi_goal_states=goals_t, num_particles_per_goal=nppg,
                      num_samples=S, sigma_goal_prior=c["sigma_goal_prior"], tensor_args=ta),
        CostCollision(c["n_dof"], T, field=obst_map, sigma_coll=c["sigma_coll"]),
    ])
    planner = StochGPMP(
        num_particles_per_goal=nppg, num_samples=S, traj_len=T, dt=c["dt"], n_dof=c["n_dof"],
        opt_iters=1, temperature=c["temperature"] if temperature is None else temperature,
        start_state=start, multi_goal_states=goals_t, cost=cost,
        step_size=c["step_size"], sigma_start_init=c["sigma_start_init"],
        sigma_goal_init=c["sigma_goal_init"], sigma_gp_init=c["sigma_gp_init"],
        sigma_start_sample=c["sigma_start_sample"], sigma_goal_sample=c["sigma_goal_sample"],
        sigma_gp_sample=c["sigma_gp_sample"], seed=seed, tensor_args=ta,
        initial_particle_means=initial_particle_means)
    return planner, cost


# ------------------------------------------------------------------------------ G1
def gen_prior():
    """Sigma_inv / means / scale_tril of MultiMPPrior for small and example-size problems."""
    out = {}
    for tag, n, T, dt, ss, sg, sgoal, goals, start in [
        ("planar_T8", 2, 8, 0.02, 1e-3, 3., 1e-3, [[9., 6., 0., 0.], [9., -3., 0., 0.]],
         [-9., -9., 0., 0.]),
        ("planar_T64_init", 2, 64, 0.02, 1e-3, 20., 1e-3, [[9., 6., 0., 0.], [9., -3., 0., 0.]],
         [-9., -9., 0., 0.]),
        ("nogoal_T6", 3, 6, 0.1, 0.05, 0.7, None, None, [0.1, -0.2, 0.3, 0., 0., 0.]),
        ("panda_T16", 7, 16, 0.05, 1e-3, 0.1, 0.07,
         [[0.5, 0.2, 0.3, -1.5, 0.1, 2.0, 0.3] + [0.] * 7],
         [0.012, -0.57, 0., -2.81, 0., 3.037, 0.741] + [0.] * 7),
    ]:
        d = 2 * n
        start_t = torch.tensor(start, **F64)
        goals_t = None if goals is None else torch.tensor(goals, **F64)
        K_s = UnaryFactor(d, ss, start_t, F64).K
        K_g = None if goals is None else UnaryFactor(d, sgoal, goals_t[0], F64).K
        Q = GPFactor(n, sg, dt, T - 1, F64).Q_inv[0]
        prior = MultiMPPrior(T - 1, dt, d, n, K_s, Q, start_t, K_g_inv=K_g, goal_states=goals_t,
                             tensor_args=F64)
        out[tag + "/params"] = np.array([n, T, dt, ss, sg, -1. if sgoal is None else sgoal])
        out[tag + "/start"] = npy(start_t)
        if goals is not None:
            out[tag + "/goals"] = npy(goals_t)
        out[tag + "/means"] = npy(prior.means)
        M = T * d
        if M <= 256:
            out[tag + "/Sigma_inv"] = npy(prior.Sigma_inv)
            out[tag + "/scale_tril"] = npy(prior.dist._unbroadcasted_scale_tril[0])
        else:   # keep the fixture small: first/last block rows + a strided sample of rows
            S_inv, L = prior.Sigma_inv, prior.dist._unbroadcasted_scale_tril[0]
            out[tag + "/Sigma_inv_top"] = npy(S_inv[:2 * d, :3 * d])
            out[tag + "/Sigma_inv_mid"] = npy(S_inv[5 * d:6 * d, 4 * d:7 * d])
            out[tag + "/Sigma_inv_bot"] = npy(S_inv[-2 * d:, -3 * d:])
            out[tag + "/Sigma_inv_offband_absmax"] = np.array(
                float((S_inv - torch.tril(torch.triu(S_inv, -2 * d + 1), 2 * d - 1)).abs().max()))
            rows = list(range(0, M, 37)) + [M - 1]
            out[tag + "/scale_tril_rows_idx"] = np.array(rows)
            out[tag + "/scale_tril_rows"] = npy(L[rows])
    np.savez_compressed(os.path.join(OUT, "g1_prior.npz"), **out)


# ------------------------------------------------------------------------------ G2
def gen_planar_e2e():
    """Config 1 of BASELINE.json: planar, 2 goals x 2 particles, S=16, T=64, fp64, seed 0."""
    obst = planar_scene(F64)
    grid = obst.map
    assert grid.max() <= 255 and np.all(grid == np.round(grid))
    T, goals, nppg, S, seed = 64, [[9., 6., 0., 0.], [9., -3., 0., 0.]], 2, 16, 0
    n_iters, keep_eps = 10, 3
    out = {"grid": grid.astype(np.uint8), "cell_size": np.array(obst.cell_size),
           "c_offset": npy(obst.c_offset), "goals": np.array(goals),
           "dims": np.array([T, nppg, S, seed, n_iters])}
    with NoiseTap() as tap:
        planner, _ = build_planar(obst, T, goals, nppg, S, seed, F64)
        out["means_reset"] = npy(planner.particle_means)
        out["Sigma_inv_sample_diag_blocks"] = npy(planner.Sigma_inv[:8, :12])
        for it in range(1, n_iters + 1):
            sp, cp, st, cs, costs, grad = planner.optimize()
            if it <= keep_eps:
                out[f"costs_{it}"] = npy(costs)
                out[f"grad_{it}"] = npy(grad)
                out[f"weights_{it}"] = npy(planner._weights.reshape(planner.num_particles, S))
            if it in (1, 2, 3, 10):
                out[f"means_{it}"] = npy(planner.particle_means)
            if it == 1:
                out["samples_1_p0_s0"] = npy(planner.state_samples[0, 0])
                out["samples_1_p3_s15"] = npy(planner.state_samples[3, 15])
                out["ret_state_particles_1"] = npy(sp)      # pre-update mean positions
        draws = tap.draws
    assert len(draws) == 2 + n_iters
    out["eps_init"] = npy(draws[0])                  # [nppg, G, M]
    out["eps_discard_checksum"] = np.array(float(draws[1].sum()))
    for it in range(1, keep_eps + 1):
        out[f"eps_{it}"] = npy(draws[1 + it])        # [S, P, M]
    # checksums so a seed replay of the later draws can be validated without storing them
    out["eps_checksums"] = np.array([float(dr.sum()) for dr in draws])
    np.savez_compressed(os.path.join(OUT, "g2_planar_e2e.npz"), **out)

    # a multi-goal 'const_vel' start in a small workspace with soft (not one-hot) weights
    T2, nppg2, S2 = 16, 2, 8
    goals2 = [[2.9, 2.6, 0., 0.], [2.9, -1.3, 0., 0.], [-1.3, 2.9, 0., 0.]]
    soft = dict(start=[-2.9, -2.9, 0., 0.], dt=0.5, cost_sigma_start=0.5, cost_sigma_gp=8.,
                sigma_coll=0.4, sigma_goal_prior=2., sigma_start_sample=2., sigma_goal_sample=2.,
                sigma_gp_sample=6.)
    out2 = {"dims": np.array([T2, nppg2, S2, 1, 3]), "goals": np.array(goals2),
            "temperature": np.array(20.), "start": np.array(soft["start"]),
            "sigmas": np.array([soft["dt"], soft["cost_sigma_start"], soft["cost_sigma_gp"],
                                soft["sigma_coll"], soft["sigma_goal_prior"],
                                soft["sigma_start_sample"], soft["sigma_goal_sample"],
                                soft["sigma_gp_sample"]])}
    with NoiseTap() as tap:
        planner, _ = build_planar(obst, T2, goals2, nppg2, S2, 1, F64,
                                  initial_particle_means='const_vel', temperature=20., **soft)
        out2["means_reset"] = npy(planner.particle_means)
        for it in range(1, 4):
            _, _, _, _, costs, grad = planner.optimize()
            out2[f"costs_{it}"] = npy(costs)
            out2[f"grad_{it}"] = npy(grad)
            out2[f"weights_{it}"] = npy(planner._weights.reshape(planner.num_particles, S2))
            out2[f"means_{it}"] = npy(planner.particle_means)
        draws = tap.draws
    assert len(draws) == 1 + 3
    for it in range(1, 4):
        out2[f"eps_{it}"] = npy(draws[it])
    np.savez_compressed(os.path.join(OUT, "g2b_planar_constvel_soft.npz"), **out2)


# ------------------------------------------------------------------------------ G3
def gen_cost_terms():
    """Per-term costs on random small trajectories, incl. out-of-grid and negative coordinates."""
    g = torch.Generator().manual_seed(123)
    out = {}
    for tag, ta in (("f64", F64), ("f32", F32)):
        n, T, dt = 2, 5, 0.02
        G, nppg, S = 2, 1, 3
        B = G * nppg * S
        obst = planar_scene(ta)
        trajs = (torch.rand(B, T, 2 * n, generator=g, dtype=torch.float64) * 24. - 12.).to(**ta)
        trajs[0, 1, :2] = torch.tensor([-10.0, 9.99], **ta)      # edges / outside
        trajs[1, 2, :2] = torch.tensor([15.0, -15.0], **ta)
        trajs[2, 3, :2] = torch.tensor([-0.05, 0.05], **ta)      # floor on negatives
        trajs[3, 4, :2] = torch.tensor([0.0, 0.0], **ta)
        start = torch.tensor([-9., -9., 0., 0.], **ta)
        goals = torch.tensor([[9., 6., 0., 0.], [9., -3., 0., 0.]], **ta)
        cgp = CostGP(n, T, start, dt, dict(sigma_start=1e-3, sigma_gp=0.1), ta)
        cgl = CostGoalPrior(n, T, multi_goal_states=goals, num_particles_per_goal=nppg,
                            num_samples=S, sigma_goal_prior=1e-3, tensor_args=ta)
        cco = CostCollision(n, T, field=obst, sigma_coll=1e-5)
        out[tag + "/trajs"] = npy(trajs)
        out[tag + "/cost_gp"] = npy(cgp.eval(trajs))
        out[tag + "/cost_goal_prior"] = npy(cgl.eval(trajs))
        out[tag + "/cost_collision"] = npy(cco.eval(trajs))
        out[tag + "/grid_vals"] = npy(obst.compute_cost(trajs[:, :, :2].reshape(-1, 2)))
        out[tag + "/composite"] = npy(CostComposite(n, T, [cgp, cgl, cco]).eval(
            trajs.reshape(G * nppg, S, T, 2 * n)))
    np.savez_compressed(os.path.join(OUT, "g3_cost_terms.npz"), **out)


# ------------------------------------------------------------------------------ G4
def gen_panda_fields():
    """Link fields on random frames, and the reference's CostComposite driven by the oracle FK."""
    g = torch.Generator().manual_seed(7)
    out = {}
    B, T, L = 3, 4, 11
    frames = torch.zeros(B, T, L, 4, 4, dtype=torch.float64)
    frames[..., :3, 3] = torch.rand(B, T, L, 3, generator=g, dtype=torch.float64) * 0.8 - 0.2
    frames[..., 3, 3] = 1.
    frames[0, 0, 3, :3, 3] = frames[0, 0, 2, :3, 3]           # coincident links
    spheres = torch.tensor([[[0.3, 0.1, 0.4, 0.15], [0.1, -0.1, 0.2, 0.1], [0.5, 0.4, 0.1, 0.2]]],
                           dtype=torch.float64)
    out["frames"] = npy(frames)
    out["spheres"] = npy(spheres)
    for tag, ta in (("f64", F64), ("f32", F32)):
        fr, sp = frames.to(**ta), spheres.to(**ta)
        for name, kw in [("rbf", dict(field_type='rbf')), ("sdf", dict(field_type='sdf')),
                         ("sdf_clamp", dict(field_type='sdf', clamp_sdf=True)),
                         ("occ", dict(field_type='occupancy')),
                         ("rbf_interp2", dict(field_type='rbf', num_interpolate=2)),
                         ("sdf_interp3", dict(field_type='sdf', num_interpolate=3,
                                              link_interpolate_range=[2, 6]))]:
            f = LinkDistanceField(tensor_args=ta, **kw)
            out[f"{tag}/{name}"] = npy(f.compute_cost(fr, obstacle_spheres=sp))
            out[f"{tag}/{name}_2dsph"] = npy(f.compute_cost(fr, obstacle_spheres=sp[0]))
        out[f"{tag}/self"] = npy(LinkSelfDistanceField(margin=0.03, tensor_args=ta).compute_cost(fr))
        out[f"{tag}/self_m2_interp2"] = npy(LinkSelfDistanceField(
            margin=0.2, num_interpolate=2, tensor_args=ta).compute_cost(fr))

    # composite Panda cost through the REFERENCE CostComposite with the oracle FK injected
    n, T, dt, nppg, S = 7, 8, 0.05, 2, 4
    start_q = [0.012, -0.57, 0., -2.81, 0., 3.037, 0.741]
    goal_q = [0.5, 0.2, 0.3, -1.5, 0.1, 2.0, 0.3]
    rng = np.random.default_rng(0)
    sph = np.zeros((1, 5, 4))
    sph[0, :, :3] = rng.uniform([0.2, -0.5, 0.2], [1.0, 0.5, 1.0], size=(5, 3))
    sph[0, :, 3] = rng.uniform(0.1, 0.2, size=5)
    out["panda/spheres"] = sph
    out["panda/start_q"] = np.array(start_q)
    out["panda/goal_q"] = np.array(goal_q)
    for tag, ta in (("f64", F64), ("f32", F32)):
        start = torch.tensor(start_q + [0.] * 7, **ta)
        goals = torch.tensor([goal_q + [0.] * 7], **ta)
        # smooth-ish random trajectories between start and goal
        lam = torch.linspace(0, 1, T, dtype=torch.float64).view(1, 1, T, 1)
        base = (1 - lam) * torch.tensor(start_q, dtype=torch.float64) + lam * torch.tensor(goal_q, dtype=torch.float64)
        pos = base + 0.15 * torch.randn(nppg, S, T, n, generator=g, dtype=torch.float64)
        vel = 0.3 * torch.randn(nppg, S, T, n, generator=g, dtype=torch.float64)
        trajs = torch.cat([pos, vel], dim=-1).to(**ta)
        sph_t = torch.from_numpy(sph).to(**ta)
        terms = dict(
            gp=CostGP(n, T, start, dt, dict(sigma_start=1e-4, sigma_gp=7e-4), ta),
            goal_prior=CostGoalPrior(n, T, multi_goal_states=goals, num_particles_per_goal=nppg,
                                     num_samples=S, sigma_goal_prior=20., tensor_args=ta),
            self=CostCollision(n, T, field=LinkSelfDistanceField(margin=0.03, tensor_args=ta),
                               sigma_coll=0.01),
            coll_rbf=CostCollision(n, T, field=LinkDistanceField(tensor_args=ta), sigma_coll=0.01),
            coll_sdf=CostCollision(n, T, field=LinkDistanceField(field_type='sdf', tensor_args=ta),
                                   sigma_coll=0.01),
            coll_occ=CostCollision(n, T, field=LinkDistanceField(field_type='occupancy',
                                                                 tensor_args=ta), sigma_coll=0.01),
        )
        out[f"panda/{tag}/trajs"] = npy(trajs)
        q = trajs.reshape(-1, 2 * n)[:, :n]
        out[f"panda/{tag}/fk_oracle"] = npy(fk_all_links(q))
        for name, term in terms.items():
            cc = CostComposite(n, T, [term], FK=fk_all_links, tensor_args=ta)
            out[f"panda/{tag}/{name}"] = npy(cc.eval(trajs, obstacle_spheres=sph_t))
        cc = CostComposite(n, T, [terms["gp"], terms["goal_prior"], terms["self"],
                                  terms["coll_rbf"]], FK=fk_all_links, tensor_args=ta)
        out[f"panda/{tag}/composite"] = npy(cc.eval(trajs, obstacle_spheres=sph_t))
    np.savez_compressed(os.path.join(OUT, "g4_panda_fields.npz"), **out)


# ------------------------------------------------------------------------------ G5
def gen_update_and_is():
    """_update_distribution and the importance-sampling term on hand-made inputs."""
    obst = planar_scene(F64)
    T, goals, nppg, S = 8, [[9., 6., 0., 0.], [9., -3., 0., 0.]], 2, 5
    g = torch.Generator().manual_seed(99)
    out = {"dims": np.array([T, nppg, S])}
    planner, cost = build_planar(obst, T, goals, nppg, S, 5, F64, temperature=3.0)
    P, d = planner.num_particles, 4
    samples = planner.particle_means.unsqueeze(1) + 0.3 * torch.randn(P, S, T, d, generator=g,
                                                                      dtype=torch.float64)
    planner.state_samples = samples
    out["means_in"] = npy(planner.particle_means)
    out["samples"] = npy(samples)
    out["costs_with_is"] = npy(planner._get_costs())
    out["costs_no_is"] = npy(cost.eval(samples).reshape(P, S))
    for tag, costs in (("spread", torch.tensor([[1., 5., 2., 9., 4.]] * P, dtype=torch.float64)
                        + torch.arange(P, dtype=torch.float64).view(P, 1)),
                       ("neartie", torch.tensor([[7.0, 7.0 + 1e-9, 7.5, 30., 7.0]] * P,
                                                dtype=torch.float64)),
                       ("huge", torch.tensor([[1e11, 3e9, 3e9 + 2., 8e10, 5e9]] * P,
                                             dtype=torch.float64))):
        planner.particle_means = torch.from_numpy(out["means_in"]).clone()
        planner._sample_dist.set_mean(planner.particle_means.view(P, -1))
        grad = planner._update_distribution(costs.clone(), samples)
        out[f"{tag}/costs"] = npy(costs)
        out[f"{tag}/weights"] = npy(planner._weights.reshape(P, S))
        out[f"{tag}/grad"] = npy(grad)
        out[f"{tag}/means_out"] = npy(planner.particle_means)
    np.savez_compressed(os.path.join(OUT, "g5_update_is.npz"), **out)


# ------------------------------------------------------------------------------ G6
def gen_scene_tooling():
    """Setup-side scene generators: the reference's `generate_obstacle_map` with
    fixed + random obstacles on a coarse grid, and `random_init_static_sphere` (envs/panda.py:42-66,
    imported with empty stand-in modules for the PyBullet imports of that file -- the function itself
    is pure numpy) with the example's parameters (examples/panda_environment.py:124-133)."""
    from stoch_gpmp.envs.obst_map import ObstacleCircle, ObstacleRectangle
    for name in ("pybullet", "pybullet_data", "pybullet_utils", "pybullet_utils.bullet_client"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["pybullet_utils"].bullet_client = sys.modules["pybullet_utils.bullet_client"]
    from stoch_gpmp.envs.panda import random_init_static_sphere
    out = {}
    for seed in (0, 7):
        random.seed(seed)
        np.random.seed(seed)
        om, obs = generate_obstacle_map(map_dim=[10, 12], obst_list=[ObstacleRectangle(0, 0, 2, 3),
                                                                     ObstacleCircle(-3, 2, 1.)],
                                        cell_size=0.25, random_gen=True, num_obst=7,
                                        rand_limits=[[-4, 4], [-5, 5]], rand_rect_shape=[1, 2],
                                        rand_circle_radius=0.75, tensor_args=F64)
        out[f"map/{seed}/grid"] = om.map.astype(np.uint8)
        out[f"map/{seed}/n_obst"] = np.array(len(obs))
        np.random.seed(seed)
        sph = np.zeros((5, 4))
        for i in range(5):
            r, pos = random_init_static_sphere(0.1, 0.2, np.array([0.6, -0.2, 0.6]),
                                               np.array([1., 0.2, 1]), 0.01)
            sph[i, :3], sph[i, 3] = pos, r
        out[f"spheres/{seed}"] = sph
    np.savez_compressed(os.path.join(OUT, "g6_scene_tooling.npz"), **out)


# ------------------------------------------------------------------------------ G7
def gen_gpmp():
    """The reference's Gauss-Newton planner GPMP (planner.py:352-661) on a small Panda problem with
    oracle.fk as the FK callable: particle means before / after each of 3 steps, the costs it reports,
    for both damping modes."""
    from stoch_gpmp.planner import GPMP
    from tests import scenarios as SC
    c, n, T, nppg = SC.PANDA, 7, 8, 3
    start = torch.tensor(c["start_q"] + [0.] * n, **F64)
    goals = torch.tensor([c["goal_q"] + [0.] * n, [-0.4, 0.5, -0.3, -2.0, 0.2, 1.5, -0.5] + [0.] * n], **F64)
    sph = torch.as_tensor(SC.panda_spheres()).to(**F64)
    out = {"dims": np.array([T, nppg]), "goals": npy(goals), "spheres": npy(sph)}
    for tag, solver in (("tr", dict(delta=1e-2, trust_region=True, method='cholesky')),
                        ("lm", dict(delta=5.0, trust_region=False, method='inverse'))):
        cost = CostComposite(n, T, [
            CostGP(n, T, start, c["dt"], dict(sigma_start=c["cost_sigma_start"], sigma_gp=c["cost_sigma_gp"]), F64),
            CostGoalPrior(n, T, multi_goal_states=goals, num_particles_per_goal=nppg, num_samples=1,
                          sigma_goal_prior=c["sigma_goal_prior"], tensor_args=F64),
            CostCollision(n, T, field=LinkSelfDistanceField(margin=c["self_margin"], tensor_args=F64),
                          sigma_coll=c["sigma_self"], tensor_args=F64),
            CostCollision(n, T, field=LinkDistanceField(tensor_args=F64), sigma_coll=c["sigma_coll"],
                          tensor_args=F64),
        ], FK=fk_all_links, tensor_args=F64)
        pl = GPMP(num_particles_per_goal=nppg, traj_len=T, opt_iters=1, dt=c["dt"], n_dof=n, step_size=0.5,
                  temperature=1., start_state=start, multi_goal_states=goals, cost=cost,
                  sigma_start_init=c["sigma_start_init"], sigma_start_sample=c["sigma_start_sample"],
                  sigma_goal_init=c["sigma_goal_init"], sigma_goal_sample=c["sigma_goal_sample"],
                  sigma_gp_init=c["sigma_gp_init"], sigma_gp_sample=c["sigma_gp_sample"], seed=0,
                  solver_params=solver, tensor_args=F64)
        out[f"{tag}/means0"] = npy(pl.particle_means)
        for it in range(3):
            vel, pos, costs = pl.optimize(obstacle_spheres=sph)
            out[f"{tag}/means{it + 1}"] = npy(pl.particle_means)
            out[f"{tag}/costs{it + 1}"] = npy(costs)
    np.savez_compressed(os.path.join(OUT, "g7_gpmp.npz"), **out)


def gen_field_surface():
    """The remaining methods of the cited field classes (no caller inside the reference): distances /
    compute_collision / compute_distance of both link fields (fields.py:40-61,100-112) and ObstacleMap.get_xy_grid
    (obst_map.py:158-162), run on the frames and spheres of g4 plus a configuration with links in contact."""
    z = np.load(os.path.join(OUT, "g4_panda_fields.npz"))
    frames = torch.from_numpy(z["frames"]).clone()
    frames[1, 2, 9, :3, 3] = frames[1, 2, 6, :3, 3] + 0.01        # links 9 and 6 nearly coincide (self collision)
    frames[2, 1, 4, :3, 3] = torch.tensor([0.3, 0.1, 0.4]) + 0.05  # link 4 inside sphere 0
    spheres = torch.from_numpy(z["spheres"])[0]                   # [O,4]
    out = {"frames": npy(frames), "spheres": npy(spheres)}
    for tag, ta in (("f64", F64), ("f32", F32)):
        fr, sp = frames.to(**ta), spheres.to(**ta)
        f = LinkDistanceField(tensor_args=ta)
        out[f"{tag}/sph_distances"] = npy(f.distances(fr, sp))
        out[f"{tag}/sph_collision"] = npy(f.compute_collision(fr, sp))
        out[f"{tag}/sph_collision_b01"] = npy(f.compute_collision(fr, sp, buffer=0.1))
        out[f"{tag}/sph_distance"] = npy(f.compute_distance(fr, sp))
        s = LinkSelfDistanceField(tensor_args=ta)
        out[f"{tag}/self_distances"] = npy(s.distances(fr))
        out[f"{tag}/self_collision"] = npy(s.compute_collision(fr))
        out[f"{tag}/self_collision_b02"] = npy(s.compute_collision(fr, buffer=0.2))
        out[f"{tag}/self_distance"] = npy(s.compute_distance(fr))
    om = ObstacleMap([4, 6], 0.5, tensor_args=F64)
    out["xy_grid_4x6_c05"] = npy(om.get_xy_grid(torch.device("cpu")))
    np.savez_compressed(os.path.join(OUT, "g8_field_surface.npz"), **out)


def gen_panda_urdf():
    """The kinematic chain of the reference's OWN robot description, assets/franka_description/robots/
    panda_arm_no_gripper.urdf (a data file of the reference; what examples/panda_environment.py:47 hands to torch_robotics):
    every joint from panda_link0 to ee_link in chain order -- type, origin xyz / rpy, axis, limits -- parsed, not typed.
    The forward-kinematics CODE the reference calls lives in un-vendored torch_robotics; its INPUT data are pinned here."""
    import xml.etree.ElementTree as ET
    root = ET.parse(os.path.join("/root/reference", "assets", "franka_description", "robots", "panda_arm_no_gripper.urdf")).getroot()
    by_parent = {}
    for j in root.findall("joint"):
        by_parent.setdefault(j.find("parent").get("link"), []).append(j)
    names, kinds, xyz, rpy, axis, lower, upper, links = [], [], [], [], [], [], [], ["panda_link0"]
    link = "panda_link0"
    while link != "ee_link":
        cands = by_parent[link]
        j = cands[0] if len(cands) == 1 else [c for c in cands if c.find("child").get("link") in
                                                ("panda_hand", "ee_link") or c.find("child").get("link").startswith("panda_link")][0]
        o = j.find("origin")
        names.append(j.get("name")); kinds.append(j.get("type"))
        xyz.append([float(v) for v in (o.get("xyz") if o is not None and o.get("xyz") else "0 0 0").split()])
        rpy.append([float(v) for v in (o.get("rpy") if o is not None and o.get("rpy") else "0 0 0").split()])
        ax = j.find("axis")
        axis.append([float(v) for v in ax.get("xyz").split()] if ax is not None else [0., 0., 0.])
        lim = j.find("limit")
        lower.append(float(lim.get("lower")) if lim is not None and lim.get("lower") else np.nan)
        upper.append(float(lim.get("upper")) if lim is not None and lim.get("upper") else np.nan)
        link = j.find("child").get("link")
        links.append(link)
    np.savez(os.path.join(OUT, "g9_panda_urdf_chain.npz"), joint_names=np.array(names), joint_types=np.array(kinds),
             xyz=np.array(xyz), rpy=np.array(rpy), axis=np.array(axis), lower=np.array(lower), upper=np.array(upper),
             link_names=np.array(links))


# ------------------------------------------------------------------------------ G10
def gen_per_particle_precisions():
    """Covariance adaptation through the planner's live sampling distribution: a config-1-sized reference
    planner, then `planner._sample_dist.set_Sigma_invs(new)` with one precision matrix PER PARTICLE -- the same prior with its
    GP blocks scaled by 1 + 0.1 p, built by the reference's own get_const_vel_covariance -- then 3 x optimize().  The reference
    samples particle p from precision p while the importance-sampling term keeps `planner.Sigma_inv` captured at reset
    (planner.py:226,233-236; mp_priors_multi.py:125-128)."""
    obst = planar_scene(F64)
    T, goals, nppg, S, seed = 64, [[9., 6., 0., 0.], [9., -3., 0., 0.]], 2, 16, 3
    out = {"grid": obst.map.astype(np.uint8), "cell_size": np.array(obst.cell_size), "goals": np.array(goals),
           "dims": np.array([T, nppg, S, seed, 3])}
    with NoiseTap() as tap:
        planner, _ = build_planar(obst, T, goals, nppg, S, seed, F64)
        out["means_reset"] = npy(planner.particle_means)
        sd = planner._sample_dist
        P = planner.num_particles
        factors = np.array([1. + 0.1 * p for p in range(P)])
        K_s, K_g = planner.start_prior_sample.K, planner.multi_goal_prior_sample[0].K
        Q = planner.gp_prior_sample.Q_inv[0]
        new = torch.stack([sd.get_const_vel_covariance(planner.dt, K_s, Q * float(f), K_g) for f in factors])
        assert new.shape == sd.Sigma_invs.shape
        sd.set_Sigma_invs(new)
        out["gp_scale_per_particle"] = factors
        out["Sigma_invs_p3_rows_0_8"] = npy(new[3, :8, :12])
        out["Sigma_inv_planner_rows_0_8"] = npy(planner.Sigma_inv[:8, :12])      # unchanged: what the IS term uses
        for it in range(1, 4):
            sp, cp, st, cs, costs, grad = planner.optimize()
            out[f"means_{it}"] = npy(planner.particle_means)
            out[f"costs_{it}"] = npy(costs)
            if it == 1:
                out["samples_1_p3_s5"] = npy(planner.state_samples[3, 5])
                out["samples_1_p0_s0"] = npy(planner.state_samples[0, 0])
        draws = tap.draws
    assert len(draws) == 2 + 3
    out["eps_init"] = npy(draws[0])
    for it in range(1, 4):
        out[f"eps_{it}"] = npy(draws[1 + it])
    np.savez_compressed(os.path.join(OUT, "g10_per_particle_precisions.npz"), **out)


# ------------------------------------------------------------------------------ G11
def gen_signatures():
    """Names, parameter names and defaults of every public method of the classes on the path, as the
    reference declares them -- DATA (inspect.signature), so that a CPU test can hold the mirrors in stoch_gpmp_amd to
    "accepts a superset, same defaults" (INTEGRATION.md section 1)."""
    import inspect
    import json
    from stoch_gpmp import planner as ref_planner
    from stoch_gpmp.costs import cost_functions as ref_costs
    from stoch_gpmp.costs import fields as ref_fields
    from stoch_gpmp.costs.factors import field_factor as ref_ff
    from stoch_gpmp.envs import obst_map as ref_om
    classes = {
        "planner.StochGPMP": ref_planner.StochGPMP, "planner.GPMP": ref_planner.GPMP,
        "costs.factors.mp_priors_multi.MultiMPPrior": MultiMPPrior,
        "costs.factors.gp_factor.GPFactor": GPFactor, "costs.factors.unary_factor.UnaryFactor": UnaryFactor,
        "costs.factors.field_factor.FieldFactor": ref_ff.FieldFactor,
        "costs.cost_functions.CostComposite": ref_costs.CostComposite, "costs.cost_functions.CostGP": ref_costs.CostGP,
        "costs.cost_functions.CostGPTrajectory": ref_costs.CostGPTrajectory,
        "costs.cost_functions.CostCollision": ref_costs.CostCollision, "costs.cost_functions.CostGoal": ref_costs.CostGoal,
        "costs.cost_functions.CostGoalPrior": ref_costs.CostGoalPrior,
        "costs.fields.LinkDistanceField": ref_fields.LinkDistanceField,
        "costs.fields.LinkSelfDistanceField": ref_fields.LinkSelfDistanceField,
        "costs.fields.EESE3DistanceField": ref_fields.EESE3DistanceField,
        "envs.obst_map.ObstacleMap": ref_om.ObstacleMap,
    }
    out = {}
    for cname, cls in classes.items():
        methods = {}
        for mname, fn in inspect.getmembers(cls, predicate=inspect.isfunction):
            if mname.startswith("_") and mname != "__init__":
                continue
            params = []
            for pn, prm in inspect.signature(fn).parameters.items():
                if pn == "self":
                    continue
                kind = {prm.VAR_KEYWORD: "**", prm.VAR_POSITIONAL: "*"}.get(prm.kind, "")
                default = None if prm.default is inspect.Parameter.empty else repr(prm.default)
                params.append([kind + pn, default])
            methods[mname] = params
        out[cname] = methods
    # module-level helper of the planner module
    out["planner.<module>"] = {"print_info": [[pn, None] for pn in inspect.signature(ref_planner.print_info).parameters]}
    with open(os.path.join(OUT, "g11_signatures.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


# ------------------------------------------------------------------------------ G12
G12_BRANCHES = {"generic": "COMPATIBLE", "avx2": "AVX2"}       # record name -> MKL_CBWR


def gen_panda_fk_mkl_branches():
    """g4's Panda FK on the other roundings MKL's code branches (MKL_CBWR) give its small GEMMs.  With MKL 2024.2 every branch
    name gives one of three: AVX-512 (AUTO on an AVX-512 host, AVX512, AVX512_E1 .. E5: g4's fk_oracle, the run the reference
    was fed), "avx2" (AVX2, AVX512_MIC) and "generic" (COMPATIBLE, SSE2 .. SSE4_2, AVX).  MKL reads the setting once per
    process, so a child process computes each run.  Data only: the oracle's output on g4's trajectories."""
    part = os.environ.get("G12_PART")
    if part:                                     # (the child: one branch, MKL_CBWR set by the parent)
        z = np.load(os.path.join(OUT, "g4_panda_fields.npz"))
        n = 7
        np.savez(part, **{tag: npy(fk_all_links(torch.as_tensor(z[f"panda/{tag}/trajs"], dtype=dtype).reshape(-1, 2 * n)[:, :n]))
                          for tag, dtype in (("f64", torch.float64), ("f32", torch.float32))})
        return
    import subprocess
    import tempfile
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name, cbwr in G12_BRANCHES.items():
            path = os.path.join(d, name + ".npz")
            subprocess.run([sys.executable, os.path.abspath(__file__), "g12"], env=dict(os.environ, MKL_CBWR=cbwr, G12_PART=path),
                           check=True, stdout=subprocess.DEVNULL)
            with np.load(path) as runs:
                out.update({f"{name}/panda/{tag}/fk_oracle": runs[tag] for tag in runs.files})
    np.savez_compressed(os.path.join(OUT, "g12_panda_fk_mkl_branches.npz"), **out)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(1)
    gens = {"g1": gen_prior, "g2": gen_planar_e2e, "g3": gen_cost_terms, "g4": gen_panda_fields,
            "g5": gen_update_and_is, "g6": gen_scene_tooling, "g7": gen_gpmp, "g8": gen_field_surface,
            "g9": gen_panda_urdf, "g10": gen_per_particle_precisions, "g11": gen_signatures,
            "g12": gen_panda_fk_mkl_branches}
    for key in (sys.argv[1:] or sorted(gens, key=lambda k: int(k[1:]))):          # `python oracle/gen_golden.py g6` regenerates one
        gens[key]()
    for f in sorted(os.listdir(OUT)):
        print(f, os.path.getsize(os.path.join(OUT, f)))
