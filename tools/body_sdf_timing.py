"""Timings of the body collision spheres on the voxel field (SGPMP_COST_BODY_SDF) on the MI355X, for the record in
profiles/r15/body_sdf.txt:

  step    the StochGPMP step of the Panda at 1024 particles x 128 samples x 64 waypoints, fp32, with the body term (along_links at
          spacing 0.12 / 0.06 / 0.03: M = 18 / 31 / 55 spheres) against the same step with the voxel point term (11 link origins),
          both on the path without a fused launch: sampler + generic sweep (+ body_cost_kernel) + update.  The question: does the
          body launch grow with the 8 M gathers per state, or is it bound by re-reading the samples?
  gpmp    a Panda GPMP iteration (linearize + solve) at 256 particles x 64 waypoints, fp64: without a collision field and with the
          body term's rows at the waypoints.
  --profile-step N   runs N steps with the body term (M = 18) and nothing else: the run to put under
          `rocprofv3 --kernel-trace --stats -- python tools/body_sdf_timing.py --profile-step 200` for body_cost_kernel's own time.

HIP events around windows of calls, warm-up first, the median and the min .. max of REPEATS windows, variants alternating in one
process.  Rewrites the TIMES part of the output file (default profiles/r15/body_sdf.txt)."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import voxel_sdf_timing as V  # noqa: E402  (the scene, the Panda cost list, the timing helpers)
from stoch_gpmp_amd import workloads as W  # noqa: E402
from stoch_gpmp_amd.planner import GPMP, StochGPMP  # noqa: E402
from stoch_gpmp_amd.robots.body import BodySpheres  # noqa: E402
from stoch_gpmp_amd.robots.panda_chain import PANDA_CHAIN  # noqa: E402

WARMUP, REPEATS, MARK, DEV = V.WARMUP, V.REPEATS, V.MARK, V.DEV
RADIUS = 0.03


def stoch_planner(field, ta, P=1024, S=128, T=64):
    c = W.PANDA
    cost, start, goals = V.panda_cost(T, P, S, ta, field, c["sigma_coll"])
    return StochGPMP(num_particles_per_goal=P, num_samples=S, traj_len=T, opt_iters=1, dt=c["dt"], n_dof=7,
                     step_size=c["step_size"], temperature=c["temperature"], start_state=start, multi_goal_states=goals, cost=cost,
                     sigma_start_init=c["sigma_start_init"], sigma_start_sample=c["sigma_start_sample"],
                     sigma_goal_init=c["sigma_goal_init"], sigma_goal_sample=c["sigma_goal_sample"],
                     sigma_gp_init=c["sigma_gp_init"], sigma_gp_sample=c["sigma_gp_sample"], seed=5, tensor_args=ta)


def step_times():
    ta = {"device": DEV, "dtype": torch.float32}
    P, S, T = 1024, 128, 64
    vm = V.scene(ta)
    variants = [("voxel point term, 11 link origins", stoch_planner(vm.distance_field(0.1), ta))]
    for spacing in (0.12, 0.06, 0.03):
        body = BodySpheres.along_links(PANDA_CHAIN, spacing, RADIUS)
        variants.append((f"body term, M = {len(body)} (spacing {spacing})", stoch_planner(vm.body_field(body, 0.1), ta)))
    names = {}
    for name, pl in variants:
        for _ in range(WARMUP):
            pl.step()
        names[name] = f"{pl._engine.last_cost_kernel()}, {pl._engine.last_step_launches()} launches"
    t = {name: [] for name, _ in variants}
    for _ in range(REPEATS):
        for name, pl in variants:
            t[name].append(V.timed(pl.step, 50))
    base = float(np.median(t[variants[0][0]]))
    out = [f"  step, Panda, P {P}, S {S}, T {T}, float32, 26 x 32 x 24 volume, sampler + generic sweep (+ body launch) + update:"]
    for name, _ in variants:
        out.append(f"    {name:42s} {V.fmt(t[name])}   ratio {np.median(t[name]) / base:.3f}   {names[name]}")
    return out


def gpmp_times():
    ta = {"device": DEV, "dtype": torch.float64}
    c, T, P = W.PANDA, 64, 256
    fld = V.scene(ta).body_field(BodySpheres.along_links(PANDA_CHAIN, 0.12, RADIUS), 0.1)

    def mk(field):
        cost, start, goals = V.panda_cost(T, P, 1, ta, field, 0.02)
        return GPMP(num_particles_per_goal=P, traj_len=T, opt_iters=1, dt=c["dt"], n_dof=7, step_size=0.5, start_state=start,
                    multi_goal_states=goals, cost=cost, sigma_start_init=c["sigma_start_init"],
                    sigma_start_sample=c["sigma_start_sample"], sigma_goal_init=c["sigma_goal_init"],
                    sigma_goal_sample=c["sigma_goal_sample"], sigma_gp_init=c["sigma_gp_init"], sigma_gp_sample=c["sigma_gp_sample"],
                    seed=0, solver_params=dict(delta=1.0, trust_region=False, method="cholesky"), tensor_args=ta)
    variants = [("no collision field", mk(None)), ("the body term's rows at the waypoints (M = 18)", mk(fld))]
    means0 = variants[0][1].particle_means.clone()
    t = {name: [] for name, _ in variants}
    for name, pl in variants:
        pl.particle_means.copy_(means0)
        for _ in range(WARMUP):
            pl.step()
    for _ in range(REPEATS):
        for name, pl in variants:
            pl.particle_means.copy_(means0)
            t[name].append(V.timed(pl.step, 20))
    base = float(np.median(t[variants[0][0]]))
    out = [f"  GPMP iteration (linearize + solve), Panda, P {P}, T {T}, float64:"]
    for name, _ in variants:
        out.append(f"    {name:48s} {V.fmt(t[name])}   ratio {np.median(t[name]) / base:.2f}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "body_sdf.txt"))
    ap.add_argument("--only", default=None, choices=[None, "step", "gpmp"])
    ap.add_argument("--profile-step", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    if args.profile_step > 0:                                  # the run for the kernel trace: nothing timed, nothing written
        ta = {"device": DEV, "dtype": torch.float32}
        pl = stoch_planner(V.scene(ta).body_field(BodySpheres.along_links(PANDA_CHAIN, 0.12, RADIUS), 0.1), ta)
        for _ in range(args.profile_step):
            pl.step()
        torch.cuda.synchronize()
        print(pl._engine.last_cost_kernel())
        return
    if args.only is not None:                                  # one part alone, nothing written
        print("\n".join({"step": step_times, "gpmp": gpmp_times}[args.only]()))
        return
    lines = [f"{MARK}: HIP events, {WARMUP} warm-up calls, median (min .. max) of {REPEATS} windows per variant, variants alternating; "
             f"device {torch.cuda.get_device_name(0)}"]
    for part in (step_times, gpmp_times):
        lines += part()
        print("\n".join(lines), flush=True)
    head = []
    if os.path.exists(args.out):
        for ln in open(args.out).read().splitlines():
            if ln.startswith(MARK):
                break
            head.append(ln)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(head + lines) + "\n")


if __name__ == "__main__":
    main()
