"""Timings of the body's self-collision term (SGPMP_COST_BODY_SELF) on the MI355X, for the record in profiles/r16/body_self.txt:

  step    the StochGPMP step of the Panda at 1024 particles x 128 samples x 64 waypoints, fp32, with the body term
          (SGPMP_COST_BODY_SDF; along_links at spacing 0.12 / 0.06 / 0.03: M = 18 / 31 / 55 spheres) against the same step with
          the body term plus the self term under pair_rows(min_link_gap=2), the pair counts stated, and the time per pair and
          state: (the difference of the two) / (pairs x 1024 x 128 x 63).
  gpmp    a Panda GPMP iteration (linearize + solve) at 256 particles x 64 waypoints, fp64: without a collision field and with the
          self term's rows at the waypoints (M = 18).
  example examples/panda_body_self_gpmp.py: the minimum self-clearance of the plan with the body term alone and with both terms.
  --profile-step N   runs N steps with GP + goal prior + the self term (M = 18) and nothing else: the run to put under
          `rocprofv3 --kernel-trace --stats -- python tools/body_self_timing.py --profile-step 200` for body_self_cost_kernel's
          own time.

HIP events around windows of calls, warm-up first, the median and the min .. max of REPEATS windows, variants alternating in one
process.  Rewrites the TIMES part of the output file (default profiles/r16/body_self.txt)."""
import argparse
import importlib.util
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import voxel_sdf_timing as V  # noqa: E402  (the scene and the timing helpers)
from stoch_gpmp_amd import workloads as W  # noqa: E402
from stoch_gpmp_amd.costs.cost_functions import CostCollision, CostComposite, CostGP, CostGoalPrior  # noqa: E402
from stoch_gpmp_amd.costs.fields import BodySelfDistanceField  # noqa: E402
from stoch_gpmp_amd.planner import GPMP, StochGPMP  # noqa: E402
from stoch_gpmp_amd.robots.body import BodySpheres  # noqa: E402
from stoch_gpmp_amd.robots.panda import DifferentiableFrankaPanda  # noqa: E402
from stoch_gpmp_amd.robots.panda_chain import PANDA_CHAIN  # noqa: E402

WARMUP, REPEATS, MARK, DEV = V.WARMUP, V.REPEATS, V.MARK, V.DEV
RADIUS, MARGIN = 0.03, 0.05


def panda_cost(T, nppg, S, ta, fields, sigma):
    c, n = W.PANDA, 7
    start, goals = torch.tensor(c["start_q"] + [0.] * n, **ta), torch.tensor([c["goal_q"] + [0.] * n], **ta)
    fk = DifferentiableFrankaPanda(gripper=False, device=DEV)
    terms = [CostGP(n, T, start, c["dt"], dict(sigma_start=c["cost_sigma_start"], sigma_gp=c["cost_sigma_gp"]), ta),
             CostGoalPrior(n, T, multi_goal_states=goals, num_particles_per_goal=nppg, num_samples=S,
                           sigma_goal_prior=c["sigma_goal_prior"], tensor_args=ta)]
    terms += [CostCollision(n, T, field=f, sigma_coll=sigma, tensor_args=ta) for f in fields]
    return CostComposite(n, T, terms, FK=fk.compute_forward_kinematics_all_links, tensor_args=ta), start, goals


def stoch_planner(fields, ta, P=1024, S=128, T=64):
    c = W.PANDA
    cost, start, goals = panda_cost(T, P, S, ta, fields, c["sigma_coll"])
    return StochGPMP(num_particles_per_goal=P, num_samples=S, traj_len=T, opt_iters=1, dt=c["dt"], n_dof=7,
                     step_size=c["step_size"], temperature=c["temperature"], start_state=start, multi_goal_states=goals, cost=cost,
                     sigma_start_init=c["sigma_start_init"], sigma_start_sample=c["sigma_start_sample"],
                     sigma_goal_init=c["sigma_goal_init"], sigma_goal_sample=c["sigma_goal_sample"],
                     sigma_gp_init=c["sigma_gp_init"], sigma_gp_sample=c["sigma_gp_sample"], seed=5, tensor_args=ta)


def self_field(body, ta):
    return BodySelfDistanceField(body, MARGIN, min_link_gap=2, tensor_args=ta)


def step_times():
    ta = {"device": DEV, "dtype": torch.float32}
    P, S, T = 1024, 128, 64
    vm = V.scene(ta)
    variants, pairs = [], {}
    for spacing in (0.12, 0.06, 0.03):
        body = BodySpheres.along_links(PANDA_CHAIN, spacing, RADIUS)
        sf = self_field(body, ta)
        pairs[len(body)] = sf.num_pairs
        variants.append((f"body term, M = {len(body)}", len(body), False, stoch_planner([vm.body_field(body, 0.1)], ta)))
        variants.append((f"body + self term, M = {len(body)}, {sf.num_pairs} pairs", len(body), True,
                         stoch_planner([vm.body_field(body, 0.1), sf], ta)))
    names = {}
    for name, _, _, pl in variants:
        for _ in range(WARMUP):
            pl.step()
        names[name] = f"{pl._engine.last_cost_kernel()}, {pl._engine.last_step_launches()} launches"
    t = {v[0]: [] for v in variants}
    for _ in range(REPEATS):
        for name, _, _, pl in variants:
            t[name].append(V.timed(pl.step, 30))
    out = [f"  step, Panda, P {P}, S {S}, T {T}, float32, 26 x 32 x 24 volume, sampler + generic sweep + body launch (+ self launch) + update:"]
    med = {}
    for name, M, with_self, _ in variants:
        med[(M, with_self)] = float(np.median(t[name]))
        out.append(f"    {name:44s} {V.fmt(t[name])}   {names[name]}")
    states = P * S * (T - 1)
    for M, n_pairs in pairs.items():
        d = med[(M, True)] - med[(M, False)]
        out.append(f"    self launch, M = {M}: {d:.4f} ms for {n_pairs} pairs x {states} states = {1e9 * d / (n_pairs * states):.2f} ps per pair "
                   f"and state; ratio to the body-term step {med[(M, True)] / med[(M, False)]:.3f}")
    return out


def gpmp_times():
    ta = {"device": DEV, "dtype": torch.float64}
    c, T, P = W.PANDA, 64, 256
    fld = self_field(BodySpheres.along_links(PANDA_CHAIN, 0.12, RADIUS), ta)

    def mk(fields):
        cost, start, goals = panda_cost(T, P, 1, ta, fields, 0.02)
        return GPMP(num_particles_per_goal=P, traj_len=T, opt_iters=1, dt=c["dt"], n_dof=7, step_size=0.5, start_state=start,
                    multi_goal_states=goals, cost=cost, sigma_start_init=c["sigma_start_init"],
                    sigma_start_sample=c["sigma_start_sample"], sigma_goal_init=c["sigma_goal_init"],
                    sigma_goal_sample=c["sigma_goal_sample"], sigma_gp_init=c["sigma_gp_init"], sigma_gp_sample=c["sigma_gp_sample"],
                    seed=0, solver_params=dict(delta=1.0, trust_region=False, method="cholesky"), tensor_args=ta)
    variants = [("no collision field", mk([])), (f"the self term's rows at the waypoints (M = 18, {fld.num_pairs} pairs)", mk([fld]))]
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
        out.append(f"    {name:62s} {V.fmt(t[name])}   ratio {np.median(t[name]) / base:.2f}")
    return out


def example_figures():
    spec = importlib.util.spec_from_file_location("panda_body_self_gpmp", os.path.join(ROOT, "examples", "panda_body_self_gpmp.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out, fld, _ = ex.main(verbose=False)
    a, b = out["body term alone"], out["body and self terms"]
    return [f"  examples/panda_body_self_gpmp.py, {ex.SETTINGS['opt_iters']} iterations, {fld.num_pairs} counted pairs: minimum self-clearance of the "
            f"straight line {a[3]:+.4f} m, of the plan with the body term alone {a[2]:+.4f} m, of the plan with both terms {b[2]:+.4f} m"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "body_self.txt"))
    ap.add_argument("--only", default=None, choices=[None, "step", "gpmp", "example"])
    ap.add_argument("--profile-step", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    parts = {"step": step_times, "gpmp": gpmp_times, "example": example_figures}
    if args.profile_step > 0:                                  # the run for the kernel trace: nothing timed, nothing written
        ta = {"device": DEV, "dtype": torch.float32}
        pl = stoch_planner([self_field(BodySpheres.along_links(PANDA_CHAIN, 0.12, RADIUS), ta)], ta)
        for _ in range(args.profile_step):
            pl.step()
        torch.cuda.synchronize()
        print(pl._engine.last_cost_kernel())
        return
    if args.only is not None:                                  # one part alone, nothing written
        print("\n".join(parts[args.only]()))
        return
    lines = [f"{MARK}: HIP events, {WARMUP} warm-up calls, median (min .. max) of {REPEATS} windows per variant, variants alternating; "
             f"device {torch.cuda.get_device_name(0)}"]
    for part in (step_times, gpmp_times, example_figures):
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
