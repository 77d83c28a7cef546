#!/usr/bin/env python3
"""The Panda around the box of panda_voxel_gpmp.py, planned twice, headless: once with the voxel field at the arm's link ORIGINS
(`VoxelMap.distance_field`: points without thickness) and once with the same field at a BODY of collision spheres
(`VoxelMap.body_field` on `BodySpheres.along_links`: spheres of 3 cm radius every 12 cm along the links).  Prints, for both plans, the
minimum BODY clearance -- min over waypoints and spheres of d(p_m) - r_m -- which is what a link of finite thickness needs: the
link-origin plan reports itself collision-free while its body still cuts the box's edge.

    python examples/panda_body_gpmp.py [--iters 12]
"""
import argparse
import importlib.util
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from stoch_gpmp_amd.robots.body import BodySpheres  # noqa: E402
from stoch_gpmp_amd.robots.panda_chain import PANDA_CHAIN  # noqa: E402

_spec = importlib.util.spec_from_file_location("panda_voxel_gpmp", os.path.join(HERE, "panda_voxel_gpmp.py"))
scene = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(scene)                                          # the scene, the problem and the planner's settings

# (3 cm: the start and goal states, which the priors pin, hold the hand 6 cm above the table)
SPACING, RADIUS = 0.12, 0.03
# picked on the CPU oracle (tests/body_sdf_oracle.py, OracleGPMP on this problem): its body-field plan has a minimum body clearance
# of -0.013 m after one iteration, +0.0014 m from the second on, and has converged by the twelfth; its link-origin plan ends at
# +0.031 m for the link origins and -0.067 m for the body
OPT_ITERS = 12


def body():
    return BodySpheres.along_links(PANDA_CHAIN, SPACING, RADIUS)


def plan(field, tensor_args, opt_iters):
    planner, chain = scene.build_planner(field, tensor_args)
    history = []
    for _ in range(opt_iters):
        _, _, costs = planner.optimize()
        history.append(float(costs.mean()))
    return planner, chain, history


def main(opt_iters=None, dtype=torch.float64, verbose=True):
    tensor_args = {'device': torch.device('cuda:0'), 'dtype': dtype}
    opt_iters = OPT_ITERS if opt_iters is None else opt_iters
    vm = scene.build_scene(tensor_args)
    margin = scene.SETTINGS["margin"]
    point_field, body_field = vm.distance_field(margin), vm.body_field(body(), margin)

    def body_clearance(planner, chain):
        q = planner.particle_means[..., :7].reshape(-1, 7).contiguous()
        return float(body_field.compute_distance(q, chain).min())

    out = {}
    for name, field in (("link origins", point_field), ("body spheres", body_field)):
        planner, chain, history = plan(field, tensor_args, opt_iters)
        out[name] = (planner, history, body_clearance(planner, chain))
        if verbose:
            print(f"planned with the field at the {name}: cost {history[0]:.5g} -> {history[-1]:.5g}, "
                  f"minimum body clearance of the plan {out[name][2]:+.4f} m")
    return out, body_field, chain


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=None)
    main(opt_iters=ap.parse_args().iters)
