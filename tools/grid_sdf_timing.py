"""Timings of the signed-distance grid field (SGPMP_COST_GRID_SDF) on the MI355X, for the record in profiles/r10/grid_sdf.txt:

  build   sgpmp_grid_sdf_build (two launches) at 128^2, 512^2 and 2048^2, fp32, 30 % random occupancy plus a solid block;
  step    the two-launch StochGPMP step (sampler + generic sweep + update) at BASELINE config 2's shape (planar, P = 256, S = 64,
          T = 128, fp32) with the new term, against the occupancy program forced onto the same path (option no_fused_step): four
          gathers and a dozen flops per waypoint against one gather;
  gpmp    a planar GPMP step at 1024 particles x 64 waypoints, fp64: without a field (what planar GPMP could run before), with the
          term's rows at the waypoints, and with n_sub = 4 continuous-time rows as well.

HIP events around windows of calls, warm-up first, the median and the min .. max of REPEATS windows, variants alternating.
`--only build|step|gpmp` runs one part alone and writes nothing (the runs to put under rocprofv3 --kernel-trace --stats for
the kernel times, each in a run of its own).
Rewrites the TIMES part of the output file (default profiles/r10/grid_sdf.txt)."""
import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from stoch_gpmp_amd import workloads as W  # noqa: E402
from stoch_gpmp_amd.costs.cost_functions import CostCollision, CostComposite, CostGP, CostGoalPrior  # noqa: E402
from stoch_gpmp_amd.engine import Engine  # noqa: E402
from stoch_gpmp_amd.envs.obst_map import synthetic_obstacle_map  # noqa: E402
from stoch_gpmp_amd.planner import GPMP  # noqa: E402

WARMUP, REPEATS = 5, 7
MARK = "TIMES"
DEV = torch.device("cuda:0")


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def fmt(ts):
    return f"{float(np.median(ts)):9.4f} ms ({min(ts):.4f} .. {max(ts):.4f})"


def build_times():
    ta = {"device": DEV, "dtype": torch.float32}
    eng = Engine(2, 2, 0, 1, tensor_args=ta)
    out = []
    for N in (128, 512, 2048):
        rng = np.random.default_rng(N)
        occ = (rng.uniform(size=(N, N)) < 0.3).astype(np.float32)
        occ[N // 4:N // 2, N // 4:N // 2] = 1.
        occ[N // 2:, N // 2:] = 0.
        occ_d = torch.from_numpy(occ).to(**ta)
        sdf = torch.empty_like(occ_d)
        call = lambda: eng.grid_sdf_build(occ_d, 0.1, out=sdf)          # noqa: E731
        for _ in range(WARMUP):
            call()
        ts = [timed(call, 10) for _ in range(REPEATS)]
        out.append(f"  build {N:4d} x {N:<4d} float32                      {fmt(ts)}")
    return out


def step_times():
    ta = {"device": DEV, "dtype": torch.float32}
    goals = [[9., 6., 0., 0.], [9., -3., 0., 0.], [-3., 9., 0., 0.], [6., 9., 0., 0.]]
    om = synthetic_obstacle_map(seed=3, tensor_args=ta)
    fld = om.distance_field(0.3)
    mk = lambda field: W.hip_planar_planner(W.PLANAR, 128, goals, 64, 64, field, ta, seed=5)     # noqa: E731
    new, old = mk(fld), mk(om)
    old._engine.set_option("no_fused_step", 1)
    for pl in (new, old):
        for _ in range(WARMUP):
            pl.step()
        assert pl._engine.last_cost_kernel().startswith("cost_sweep_kernel"), pl._engine.last_cost_kernel()
    t = {"new": [], "old": []}
    for _ in range(REPEATS):
        t["new"].append(timed(new.step, 20))
        t["old"].append(timed(old.step, 20))
    return [f"  step, config 2 shape (P 256, S 64, T 128, float32), sampler + generic sweep + update:",
            f"    occupancy lookup (no_fused_step)               {fmt(t['old'])}",
            f"    signed-distance grid term                      {fmt(t['new'])}   ratio {np.median(t['new']) / np.median(t['old']):.3f}"]


def gpmp_times():
    ta = {"device": DEV, "dtype": torch.float64}
    c, T, P = W.PLANAR, 64, 1024
    om = synthetic_obstacle_map(seed=3, tensor_args=ta)
    fld = om.distance_field(0.3)
    start, goals = torch.tensor(c["start"], **ta), torch.tensor([[9., 6., 0., 0.]], **ta)

    def mk(field, dense):
        terms = [CostGP(2, T, start, c["dt"], dict(sigma_start=c["cost_sigma_start"], sigma_gp=c["cost_sigma_gp"]), ta),
                 CostGoalPrior(2, T, multi_goal_states=goals, num_particles_per_goal=P, num_samples=1,
                               sigma_goal_prior=c["sigma_goal_prior"], tensor_args=ta)]
        if field is not None:
            terms.append(CostCollision(2, T, field=field, sigma_coll=0.05, tensor_args=ta))
        return GPMP(num_particles_per_goal=P, traj_len=T, opt_iters=1, dt=c["dt"], n_dof=2, step_size=0.5, start_state=start,
                    multi_goal_states=goals, cost=CostComposite(2, T, terms, tensor_args=ta),
                    sigma_start_init=c["sigma_start_init"], sigma_start_sample=c["sigma_start_sample"],
                    sigma_goal_init=c["sigma_goal_init"], sigma_goal_sample=c["sigma_goal_sample"],
                    sigma_gp_init=c["sigma_gp_init"], sigma_gp_sample=c["sigma_gp_sample"], seed=0,
                    solver_params=dict(delta=1.0, trust_region=False, method="cholesky"), tensor_args=ta, dense_cost=dense)
    variants = [("no field (the planar step before)", mk(None, None)), ("the term's rows at the waypoints", mk(fld, None)),
                ("... and n_sub = 4 inserted rows", mk(fld, dict(n_sub=4, weight=1.0)))]
    means0 = variants[0][1].particle_means.clone()
    t = {name: [] for name, _ in variants}

    def window(pl):
        pl.particle_means.copy_(means0)
        return timed(pl.step, 10)
    kernel = {}
    for name, pl in variants:
        pl.particle_means.copy_(means0)
        for _ in range(WARMUP):
            pl.step()
        kernel[name] = pl._engine.last_gpmp_kernel()              # (the name is the thread's last solve)
    for _ in range(REPEATS):
        for name, pl in variants:
            t[name].append(window(pl))
    base = float(np.median(t[variants[0][0]]))
    out = ["  GPMP step (linearize + solve), planar, P 1024, T 64, float64:"]
    for name, pl in variants:
        out.append(f"    {name:46s} {fmt(t[name])}   ratio {np.median(t[name]) / base:.2f}   {kernel[name]}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "grid_sdf.txt"))
    ap.add_argument("--only", default=None, choices=[None, "build", "step", "gpmp"])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    if args.only is not None:                                  # one part alone, nothing written: the run for the kernel trace
        print("\n".join({"build": build_times, "step": step_times, "gpmp": gpmp_times}[args.only]()))
        return
    lines = [f"{MARK}: HIP events, {WARMUP} warm-up calls, median (min .. max) of {REPEATS} windows per variant, variants alternating; "
             f"device {torch.cuda.get_device_name(0)}"]
    for part in (build_times, step_times, gpmp_times):
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
