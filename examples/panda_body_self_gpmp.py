#!/usr/bin/env python3
"""The Panda against ITSELF, headless.  The body is `BodySpheres.along_links` (spheres of 5 cm radius every 12 cm along the links);
the world is a floor.  With the elbow folded, the start holds the hand on one side of the upper arm and the goal on the other: the
straight line in joint space swings the hand THROUGH the upper arm.  GPMP plans twice: with the body term alone (the body's
spheres against the world: `VoxelMap.body_field`), which sees nothing wrong, and with the body term plus the body's
self-collision term (`BodySelfDistanceField`: the body's spheres against each other under an allowed-pair mask).  Prints the
minimum self-clearance -- min over the support waypoints and the counted pairs of |p_i - p_j| - r_i - r_j -- of both plans.

    python examples/panda_body_self_gpmp.py [--iters 12]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from stoch_gpmp_amd.costs.cost_functions import CostCollision, CostComposite, CostGP, CostGoalPrior  # noqa: E402
from stoch_gpmp_amd.costs.fields import BodySelfDistanceField  # noqa: E402
from stoch_gpmp_amd.envs.voxel_map import VoxelMap  # noqa: E402
from stoch_gpmp_amd.planner import GPMP  # noqa: E402
from stoch_gpmp_amd.robots.body import BodySpheres  # noqa: E402
from stoch_gpmp_amd.robots.panda import DifferentiableFrankaPanda  # noqa: E402
from stoch_gpmp_amd.robots.panda_chain import PANDA_CHAIN  # noqa: E402

CELL, LOWER, DIMS = 0.05, (-0.8, -0.8, -0.2), (1.6, 1.6, 1.4)             # 32 x 32 x 28 cells
FLOOR = ((0., 0., -0.1), (1.6, 1.6, 0.2))                                 # (centre, size): the top at z = 0
SPACING, RADIUS = 0.12, 0.05
# Link pairs that cannot be told apart by a self-collision check: neighbours two links apart whose spheres touch by construction
# (the Panda has joints with a zero offset, so links 1 and 2 and links 5 and 6 share an origin), and the wrist and hand, links 5
# to 10, which are rigid or turn about a common point.
IGNORE = [(0, 2), (1, 3), (2, 4), (4, 6)] + [(a, b) for a in range(5, 11) for b in range(a + 2, 11)]
# Found on the CPU with the numpy twin (stoch_gpmp_amd/body_self.py): both ends have a self-clearance of +0.058 / +0.064 m, the
# straight line between them -0.063 m at its seventh waypoint (the hand inside the upper arm), and no sphere of a moving link
# comes within 0.2 m of the floor.  The fp64 oracle's GPMP on the self term (tests/body_self_oracle.py) has the plan at -0.035 m
# after one iteration, above 0 from the third on and converged at +0.039 m by the twelfth.
START_Q = [0., -0.3, 0., -2.9, -1.0, 0.85, 0.7]
GOAL_Q = [0., -0.3, 0., -2.9, 1.4, 0.85, 0.7]
SETTINGS = dict(traj_len=16, dt=0.1, margin=0.05, sigma_coll=0.02, sigma_gp=0.5, sigma_start=1e-3, sigma_goal=1e-3,
                delta=1.0, step_size=0.5, opt_iters=12)


def body():
    return BodySpheres.along_links(PANDA_CHAIN, SPACING, RADIUS)


def pair_rows():
    return body().pair_rows(min_link_gap=2, ignore=IGNORE)


def build_scene(tensor_args):
    return VoxelMap(DIMS, CELL, LOWER, tensor_args).add_box(*FLOOR)


def straight_line(traj_len, dt, dtype=torch.float64):
    q0, q1 = torch.tensor(START_Q, dtype=dtype), torch.tensor(GOAL_Q, dtype=dtype)
    w = torch.linspace(0, 1, traj_len, dtype=dtype).reshape(1, traj_len, 1)
    return torch.cat([q0 + (q1 - q0) * w, ((q1 - q0) / ((traj_len - 1) * dt)).expand(1, traj_len, 7)], dim=-1)


def build_planner(fields, tensor_args, s=SETTINGS):
    n, T = 7, s["traj_len"]
    start = torch.tensor(START_Q + [0.] * n, **tensor_args)
    goals = torch.tensor([GOAL_Q + [0.] * n], **tensor_args)
    robot = DifferentiableFrankaPanda(gripper=False, device=tensor_args["device"])
    cost = CostComposite(n, T, [
        CostGP(n, T, start, s["dt"], dict(sigma_start=s["sigma_start"], sigma_gp=s["sigma_gp"]), tensor_args),
        CostGoalPrior(n, T, multi_goal_states=goals, num_particles_per_goal=1, num_samples=1, sigma_goal_prior=s["sigma_goal"],
                      tensor_args=tensor_args),
    ] + [CostCollision(n, T, field=f, sigma_coll=s["sigma_coll"], tensor_args=tensor_args) for f in fields],
        FK=robot.compute_forward_kinematics_all_links, tensor_args=tensor_args)
    planner = GPMP(num_particles_per_goal=1, traj_len=T, opt_iters=1, dt=s["dt"], n_dof=n, step_size=s["step_size"],
                   start_state=start, multi_goal_states=goals, cost=cost, sigma_start_init=1e-3, sigma_goal_init=1e-3,
                   sigma_gp_init=1., sigma_start_sample=1e-3, sigma_goal_sample=1e-3, sigma_gp_sample=0.1, seed=0,
                   solver_params=dict(delta=s["delta"], trust_region=False, method='cholesky'), tensor_args=tensor_args,
                   initial_particle_means=straight_line(T, s["dt"]).to(**tensor_args).reshape(1, 1, T, 2 * n))
    return planner, cost.chain


def main(opt_iters=None, dtype=torch.float64, verbose=True):
    tensor_args = {'device': torch.device('cuda:0'), 'dtype': dtype}
    s = SETTINGS
    opt_iters = s["opt_iters"] if opt_iters is None else opt_iters
    body_field = build_scene(tensor_args).body_field(body(), s["margin"])
    self_field = BodySelfDistanceField(body(), s["margin"], pairs=pair_rows(), tensor_args=tensor_args)

    def self_clearance(planner, chain):
        q = planner.particle_means[..., :7].reshape(-1, 7).contiguous()
        return float(self_field.compute_distance(q, chain).min())

    out = {}
    for name, fields in (("body term alone", [body_field]), ("body and self terms", [body_field, self_field])):
        planner, chain = build_planner(fields, tensor_args)
        first = self_clearance(planner, chain)
        history = []
        for _ in range(opt_iters):
            _, _, costs = planner.optimize()
            history.append(float(costs.mean()))
        out[name] = (planner, history, self_clearance(planner, chain), first)
        if verbose:
            print(f"planned with the {name}: cost {history[0]:.5g} -> {history[-1]:.5g}, minimum self-clearance of the straight line "
                  f"{first:+.4f} m, of the plan {out[name][2]:+.4f} m ({self_field.num_pairs} counted pairs)")
    return out, self_field, chain


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=None)
    main(opt_iters=ap.parse_args().iters)
