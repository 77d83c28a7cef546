"""Timings of the voxel signed-distance field (SGPMP_COST_VOXEL_SDF) on the MI355X, for the record in profiles/r11/voxel_sdf.txt:

  build   sgpmp_voxel_sdf_build (three launches, in place) at 32^3, 128^3 and 256^3, fp32, 5 % random occupancy plus a solid block;
  step    the StochGPMP step without a fused launch (sampler + generic sweep + update) of the Panda at 1024 particles x 128 samples
          x 64 waypoints, fp32, with the voxel term against the same step with the sphere term (rbf, 5 spheres) forced onto the same
          path (options no_fused_step and no_flat_program): eight gathers and ~60 flops per link point against five exponentials;
  gpmp    a Panda GPMP iteration (linearize + solve) at 256 particles x 64 waypoints, fp64: without a collision field, with the
          term's rows at the waypoints, and with n_sub = 2 continuous-time rows as well.

HIP events around windows of calls, warm-up first, the median and the min .. max of REPEATS windows, variants alternating.
`--only build|step|gpmp` runs one part alone and writes nothing.  Rewrites the TIMES part of the output file (default
profiles/r11/voxel_sdf.txt)."""
import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from stoch_gpmp_amd import workloads as W  # noqa: E402
from stoch_gpmp_amd.costs.cost_functions import CostCollision, CostComposite, CostGP, CostGoalPrior  # noqa: E402
from stoch_gpmp_amd.costs.fields import LinkDistanceField  # noqa: E402
from stoch_gpmp_amd.engine import Engine  # noqa: E402
from stoch_gpmp_amd.envs.voxel_map import VoxelMap  # noqa: E402
from stoch_gpmp_amd.planner import GPMP, StochGPMP  # noqa: E402
from stoch_gpmp_amd.robots.panda import DifferentiableFrankaPanda  # noqa: E402

WARMUP, REPEATS = 3, 7
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
    eng = Engine(1, 2, 0, 1, tensor_args=ta)
    out = []
    for N in (32, 128, 256):
        rng = np.random.default_rng(N)
        occ = (rng.uniform(size=(N, N, N)) < 0.05).astype(np.float32)
        occ[N // 4:N // 2, N // 4:N // 2, N // 4:N // 2] = 1.
        occ[N // 2:, N // 2:, N // 2:] = 0.
        occ_d = torch.from_numpy(occ).to(**ta)
        sdf = torch.empty_like(occ_d)
        call = lambda: eng.voxel_sdf_build(occ_d, 0.02, out=sdf)          # noqa: E731
        for _ in range(WARMUP):
            call()
        ts = [timed(call, 100) for _ in range(REPEATS)]
        out.append(f"  build {N:3d}^3 float32                                {fmt(ts)}   {N ** 3 / np.median(ts) * 1e-6:8.2f} Gcell/s")
    return out


def scene(ta):
    """A table and a box in front of the Panda (examples/panda_voxel_gpmp.py's), 26 x 32 x 24 cells of 5 cm."""
    vm = VoxelMap((1.3, 1.6, 1.2), 0.05, (-0.3, -0.8, -0.1), ta)
    vm.add_box((0.6, 0., 0.1), (0.7, 1.4, 0.1)).add_box((0.55, 0., 0.35), (0.2, 0.2, 0.4))
    return vm


def panda_cost(T, nppg, S, ta, field, sigma):
    c, n = W.PANDA, 7
    start, goals = torch.tensor(c["start_q"] + [0.] * n, **ta), torch.tensor([c["goal_q"] + [0.] * n], **ta)
    fk = DifferentiableFrankaPanda(gripper=False, device=DEV)
    terms = [CostGP(n, T, start, c["dt"], dict(sigma_start=c["cost_sigma_start"], sigma_gp=c["cost_sigma_gp"]), ta),
             CostGoalPrior(n, T, multi_goal_states=goals, num_particles_per_goal=nppg, num_samples=S,
                           sigma_goal_prior=c["sigma_goal_prior"], tensor_args=ta)]
    if field is not None:
        terms.append(CostCollision(n, T, field=field, sigma_coll=sigma, tensor_args=ta))
    return CostComposite(n, T, terms, FK=fk.compute_forward_kinematics_all_links, tensor_args=ta), start, goals


def step_times():
    ta = {"device": DEV, "dtype": torch.float32}
    c, P, S, T = W.PANDA, 1024, 128, 64
    sph = torch.as_tensor(W.panda_spheres()).to(**ta)

    def mk(field):
        cost, start, goals = panda_cost(T, P, S, ta, field, c["sigma_coll"])
        return StochGPMP(num_particles_per_goal=P, num_samples=S, traj_len=T, opt_iters=1, dt=c["dt"], n_dof=7,
                         step_size=c["step_size"], temperature=c["temperature"], start_state=start, multi_goal_states=goals, cost=cost,
                         sigma_start_init=c["sigma_start_init"], sigma_start_sample=c["sigma_start_sample"],
                         sigma_goal_init=c["sigma_goal_init"], sigma_goal_sample=c["sigma_goal_sample"],
                         sigma_gp_init=c["sigma_gp_init"], sigma_gp_sample=c["sigma_gp_sample"], seed=5, tensor_args=ta)
    new, old = mk(scene(ta).distance_field(0.1)), mk(LinkDistanceField(field_type="rbf", tensor_args=ta))
    old._engine.set_option("no_fused_step", 1)
    old._engine.set_option("no_flat_program", 1)
    calls = {"new": lambda: new.step(), "old": lambda: old.step(obstacle_spheres=sph)}
    names = {}
    for k, pl in (("new", new), ("old", old)):
        for _ in range(WARMUP):
            calls[k]()
        names[k] = pl._engine.last_cost_kernel()
        assert names[k].startswith("cost_sweep_kernel"), names[k]
    t = {"new": [], "old": []}
    for _ in range(REPEATS):
        t["new"].append(timed(calls["new"], 100))
        t["old"].append(timed(calls["old"], 100))
    return [f"  step, Panda, P {P}, S {S}, T {T}, float32, sampler + generic sweep + update:",
            f"    sphere term, rbf, 5 spheres (no_fused_step, no_flat_program) {fmt(t['old'])}   {names['old']}",
            f"    voxel distance term, 26 x 32 x 24 volume                    {fmt(t['new'])}   {names['new']}   "
            f"ratio {np.median(t['new']) / np.median(t['old']):.3f}"]


def gpmp_times():
    ta = {"device": DEV, "dtype": torch.float64}
    c, T, P = W.PANDA, 64, 256
    fld = scene(ta).distance_field(0.1)

    def mk(field, dense):
        cost, start, goals = panda_cost(T, P, 1, ta, field, 0.02)
        return GPMP(num_particles_per_goal=P, traj_len=T, opt_iters=1, dt=c["dt"], n_dof=7, step_size=0.5, start_state=start,
                    multi_goal_states=goals, cost=cost, sigma_start_init=c["sigma_start_init"],
                    sigma_start_sample=c["sigma_start_sample"], sigma_goal_init=c["sigma_goal_init"],
                    sigma_goal_sample=c["sigma_goal_sample"], sigma_gp_init=c["sigma_gp_init"], sigma_gp_sample=c["sigma_gp_sample"],
                    seed=0, solver_params=dict(delta=1.0, trust_region=False, method="cholesky"), tensor_args=ta, dense_cost=dense)
    variants = [("no collision field", mk(None, None)), ("the voxel term's rows at the waypoints", mk(fld, None)),
                ("... and n_sub = 2 inserted rows", mk(fld, dict(n_sub=2, weight=1.0)))]
    means0 = variants[0][1].particle_means.clone()
    t = {name: [] for name, _ in variants}

    def window(pl):
        pl.particle_means.copy_(means0)
        return timed(pl.step, 20)
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
    out = [f"  GPMP iteration (linearize + solve), Panda, P {P}, T {T}, float64:"]
    for name, pl in variants:
        out.append(f"    {name:46s} {fmt(t[name])}   ratio {np.median(t[name]) / base:.2f}   {kernel[name]}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "voxel_sdf.txt"))
    ap.add_argument("--only", default=None, choices=[None, "build", "step", "gpmp"])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    if args.only is not None:                                  # one part alone, nothing written
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
