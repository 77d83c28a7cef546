#!/usr/bin/env python3
"""Gauss-Newton planning (GPMP) of a 2-D point mass in the random map of `examples/planar_environment.py`, headless.  The map's
occupancy grid is piecewise constant and has no linear system; its signed-distance grid under a hinge
(`ObstacleMap.distance_field`, built on the GPU) does, so GPMP plans around the obstacles -- with `dense_cost` also between the
waypoints.  Prints the costs and how many particles end free of collisions at every GP-interpolated state, checked against the
occupancy grid itself.

    python examples/planar_gpmp.py [--iters 60] [--seed 0] [--n-sub 4]
"""
import argparse
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from stoch_gpmp_amd.costs.cost_functions import CostCollision, CostComposite, CostGP, CostGoalPrior  # noqa: E402
from stoch_gpmp_amd.envs.map_generator import generate_obstacle_map  # noqa: E402
from stoch_gpmp_amd.planner import GPMP  # noqa: E402


def main(opt_iters=60, seed=0, num_particles_per_goal=8, traj_len=32, n_sub=4, margin=0.8, sigma_coll=0.01, sigma_gp=2.0, delta=10.,
         dtype=torch.float64, verbose=True):
    tensor_args = {'device': torch.device('cuda:0'), 'dtype': dtype}
    n_dof, dt = 2, 0.04
    start_state = torch.tensor([-9., -9., 0., 0.], **tensor_args)
    multi_goal_states = torch.tensor([[9., 6., 0., 0.], [9., -3., 0., 0.], [-3., 9., 0., 0.]], **tensor_args)

    random.seed(seed)                                   # obstacle positions, as in planar_environment.py
    np.random.seed(seed)                                # (rectangle or circle: the generator's coin)
    obst_map = generate_obstacle_map(map_dim=[20, 20], obst_list=[], cell_size=0.1, random_gen=True,
                                     num_obst=15, rand_limits=[[-7.5, 7.5], [-7.5, 7.5]],
                                     rand_rect_shape=[2, 2], tensor_args=tensor_args)[0]
    field = obst_map.distance_field(margin)             # exact distance transform of the grid, two launches

    cost = CostComposite(n_dof, traj_len, [
        CostGP(n_dof, traj_len, start_state, dt, dict(sigma_start=0.001, sigma_gp=sigma_gp), tensor_args),
        CostGoalPrior(n_dof, traj_len, multi_goal_states=multi_goal_states,
                      num_particles_per_goal=num_particles_per_goal, num_samples=1,
                      sigma_goal_prior=0.001, tensor_args=tensor_args),
        CostCollision(n_dof, traj_len, field=field, sigma_coll=sigma_coll, tensor_args=tensor_args),
    ], tensor_args=tensor_args)
    # Gauss-Newton is a local method: the particles start on start-goal lines bowed sideways by different amounts, and each
    # settles in the passage between obstacles nearest to its bow
    G = multi_goal_states.shape[0]
    gen = torch.Generator().manual_seed(seed)
    w = torch.linspace(0, 1, traj_len, dtype=torch.float64).reshape(1, 1, traj_len, 1)
    line = start_state[:2].cpu().double() + (multi_goal_states[:, None, None, :2].cpu().double() - start_state[:2].cpu().double()) * w
    bow = 3. * torch.sin(w * torch.pi) * torch.randn(G, num_particles_per_goal, 1, 2, generator=gen, dtype=torch.float64)
    vel = ((multi_goal_states[:, None, None, :2].cpu().double() - start_state[:2].cpu().double()) / ((traj_len - 1) * dt))
    init = torch.cat([line + bow, vel.expand(G, num_particles_per_goal, traj_len, 2)], dim=-1).to(**tensor_args)
    planner = GPMP(
        num_particles_per_goal=num_particles_per_goal, traj_len=traj_len, opt_iters=1, dt=dt, n_dof=n_dof,
        step_size=0.5, start_state=start_state, multi_goal_states=multi_goal_states, cost=cost,
        sigma_start_init=1e-3, sigma_goal_init=1e-3, sigma_gp_init=20.,
        sigma_start_sample=1e-3, sigma_goal_sample=1e-3, sigma_gp_sample=3, seed=seed,
        solver_params=dict(delta=delta, trust_region=False, method='cholesky'), tensor_args=tensor_args,
        initial_particle_means=init,
        dense_cost=dict(n_sub=n_sub, weight=1.0) if n_sub > 0 else None)

    def free_particles():
        fine = planner.interpolate_trajectories(n_sub=max(n_sub, 1))
        occ = obst_map.get_collisions(fine[..., :2].contiguous())
        return int((occ.sum(-1) == 0).sum()), fine.shape[0]

    costs = None
    for i in range(opt_iters):
        _, _, costs = planner.optimize()
        if verbose and (i % 10 == 0 or i == opt_iters - 1):
            free, total = free_particles()
            print(f"iteration {i:3d}: cost mean {float(costs.mean()):.4g} min {float(costs.min()):.4g}; "
                  f"{free} of {total} particles free of collisions at all fine states ({planner._engine.last_gpmp_kernel()})")
    return planner, costs, free_particles()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--n-sub", type=int, default=4)
    a = ap.parse_args()
    main(opt_iters=a.iters, seed=a.seed, n_sub=a.n_sub)
