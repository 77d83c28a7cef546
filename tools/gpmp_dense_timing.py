"""One Gauss-Newton step of GPMP with the continuous-time factors on (gpmp_dense_solve_kernel + the field launches on the fine
states) against the plain step of the same build (gpmp_thomas_kernel), on the MI355X: at the shape of fixture g7 (P = 6, T = 8,
n_sub = 3) and at P = 1024, T = 64, n_sub = 4, Panda, self + 5 rbf spheres, trust-region damping, fp64 and fp32.

HIP events around windows of STEPS steps, WARMUP untimed steps per planner first, REPEATS windows per variant with the two variants
alternating; every window starts from the same particle means.  Reports the median and the min .. max of the windows and the
ratio of the medians, and rewrites the TIMES part of profiles/r09/gpmp_dense.txt (or --out)."""
import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from stoch_gpmp_amd import workloads as W  # noqa: E402
from stoch_gpmp_amd.planner import GPMP  # noqa: E402

WARMUP, STEPS, REPEATS = 5, 20, 7
MARK = "TIMES"


def planner(ta, P, T, means, goals, dense_cost):
    c, n = W.PANDA, 7
    cost = W.hip_panda_cost(c, T, P // goals.shape[0], 1, ta, goals=goals.to(**ta))
    kw = {} if means is None else {"initial_particle_means": means.to(**ta).reshape(goals.shape[0], -1, T, 2 * n)}
    return GPMP(num_particles_per_goal=P // goals.shape[0], traj_len=T, opt_iters=1, dt=c["dt"], n_dof=n, step_size=0.5,
                start_state=torch.tensor(c["start_q"] + [0.] * n, **ta), multi_goal_states=goals.to(**ta), cost=cost,
                sigma_start_init=c["sigma_start_init"], sigma_start_sample=c["sigma_start_sample"],
                sigma_goal_init=c["sigma_goal_init"], sigma_goal_sample=c["sigma_goal_sample"],
                sigma_gp_init=c["sigma_gp_init"], sigma_gp_sample=c["sigma_gp_sample"], seed=0,
                solver_params=dict(delta=1e-2, trust_region=True, method="cholesky"), tensor_args=ta, dense_cost=dense_cost, **kw)


def setting(means, n_sub):
    """Limits that bind on part of the states: the 10 % / 90 % quantiles of the positions, the 80 % quantile of |velocity|."""
    m = means.double().cpu()
    n = m.shape[-1] // 2
    q, v = m[..., :n].reshape(-1, n), m[..., n:].reshape(-1, n).abs()
    return dict(n_sub=n_sub, weight=1.0, q_limits=(torch.quantile(q, 0.1, dim=0), torch.quantile(q, 0.9, dim=0)),
                v_limits=torch.quantile(v, 0.8, dim=0), sigma_limit=1e-2)


def window(pl, means0, sph):
    pl.particle_means.copy_(means0)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(STEPS):
        pl.step(obstacle_spheres=sph)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / STEPS


def measure(name, ta, P, T, n_sub, means, goals, sph):
    plain = planner(ta, P, T, means, goals, None)
    means0 = plain.particle_means.clone()
    dense = planner(ta, P, T, means0, goals, setting(means0, n_sub))
    sph = sph.to(**ta)
    for pl, kernel in ((plain, "gpmp_thomas_kernel"), (dense, "gpmp_dense_solve_kernel")):
        pl.particle_means.copy_(means0)
        for _ in range(WARMUP):
            pl.step(obstacle_spheres=sph)
        assert pl._engine.last_gpmp_kernel() == kernel, pl._engine.last_gpmp_kernel()     # (the name is the thread's last solve)
    t = {"plain": [], "dense": []}
    for _ in range(REPEATS):
        t["plain"].append(window(plain, means0, sph))
        t["dense"].append(window(dense, means0, sph))
    med = {k: float(np.median(v)) for k, v in t.items()}
    return (f"  {name:34s} {str(ta['dtype'])[6:]:8s} plain {med['plain']:8.3f} ms ({min(t['plain']):.3f} .. {max(t['plain']):.3f})   "
            f"with the rows {med['dense']:8.3f} ms ({min(t['dense']):.3f} .. {max(t['dense']):.3f})   ratio {med['dense'] / med['plain']:6.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "gpmp_dense.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    g = np.load(os.path.join(ROOT, "tests", "golden", "g7_gpmp.npz"))
    lines = [f"{MARK}: ms per GPMP step (linearize + solve), HIP events, {WARMUP} warm-up steps, median (min .. max) of {REPEATS} windows of "
             f"{STEPS} steps,", "  the two variants alternating; plain = the option off (gpmp_thomas_kernel), the same build; "
             f"device {torch.cuda.get_device_name(0)}"]
    for dtype in (torch.float64, torch.float32):
        ta = {"device": torch.device("cuda:0"), "dtype": dtype}
        lines.append(measure("g7: P = 6, T = 8, n_sub = 3", ta, 6, 8, 3, torch.from_numpy(g["tr/means0"]), torch.from_numpy(g["goals"]),
                             torch.from_numpy(g["spheres"])))
        goals = torch.tensor([W.PANDA["goal_q"] + [0.] * 7])
        lines.append(measure("P = 1024, T = 64, n_sub = 4", ta, 1024, 64, 4, None, goals, torch.as_tensor(W.panda_spheres())))
        print("\n".join(lines[-2:]), flush=True)
    head = []
    if os.path.exists(args.out):
        for ln in open(args.out).read().splitlines():
            if ln.startswith(MARK):
                break
            head.append(ln)
    with open(args.out, "w") as f:
        f.write("\n".join(head + lines) + "\n")


if __name__ == "__main__":
    main()
