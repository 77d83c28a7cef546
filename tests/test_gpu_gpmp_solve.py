"""The plain Gauss-Newton solve (csrc/gpmp.hip: gpmp_thomas_kernel for 2, 3, 6 and 7 joints, gpmp_solve_kernel for every other count)
against oracle.gpmp_equiv.OracleGPMP ("inverse"), at the shapes where its launch changes: the particles-per-wave layouts (four per
wave, one per row of 16 lanes, while 4 x 8 T (32 + 9 F) bytes fit 150 KiB; two above), dynamic LDS below and above 64 KiB, every
instantiated joint count, the fallback kernel at the joint counts that really take it, trust-region damping with field rows that
matter, and gpmp_dense_solve_kernel at traj_len = 128.  Every case asserts the kernel and the particles per wave it ran
(Engine.last_gpmp_kernel / last_gpmp_ppw).

fp64 bars: the project's own -- d_theta 1e-7, costs 1e-9, means 1e-8, relative -- over two iterations in both damping modes.
Every case with fields first asserts, on the oracle alone, that removing EACH field's rows moves the first step by >= 0.05
(relative L2).  At the constants of the g7 fixture (tests/scenarios.py PANDA, cost_sigma_gp 7e-4) removing the field rows moves the
oracle's step by 0.002 in Levenberg mode and by 0.000 in trust-region mode: the g7 tests say almost nothing about field rows in
the solve, which is why the Panda problem here is tests/voxel_sdf_oracle.py's ARM_C with self_margin 0.2."""
import numpy as np
import pytest
import torch

from oracle import gpmp_equiv as GP
from oracle.fk import fk_all_links
from tests import gpmp_dense_oracle as DO
from tests import grid_sdf_oracle as GO
from tests import voxel_sdf_oracle as VO
from tests.arm_chains import arm6, arm_config
from tests.hip_builders import hip_panda_cost
from tests.test_gpu_gpmp_dense import hip_gpmp, rel_err
from tests.test_gpu_grid_sdf import CELL, OFF, gpmp_limits
from tests.test_gpu_grid_sdf import gpmp_planner as planar_gpmp
from tests.test_gpu_grid_sdf import make_field as grid_field
from tests.test_gpu_grid_sdf import ref_sdf

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MODES = [("lm", 5.0, False), ("tr", 1e-2, True)]
THOMAS, FALLBACK, DENSE = "gpmp_thomas_kernel", "gpmp_solve_kernel", "gpmp_dense_solve_kernel"
# the project's fp32 bar on costs and means against the fp64 oracle (test_gpmp_fp32_and_errors).  It holds at the long shapes --
# measured on the MI355X: planar T = 128 costs 1.3e-8 means 8.2e-7, Panda T = 97 costs 2.4e-7 means 7.4e-6 -- so no bar had to be
# derived from the oracle's own sensitivity to fp32 inputs
FP32_BAR = 1e-4


def TA(dtype):
    return {"device": DEV, "dtype": dtype}


class Problem:
    """means [P,T,2n]; `systems`: the oracle's systems_fn; `drops`: field name -> systems_fn without that field's rows;
    `obs`: what the oracle's step takes; planner(dtype, delta, trust) -> (the HIP GPMP, what its optimize() takes)."""

    def __init__(self, means, systems, drops, planner, obs=None):
        self.means, self.systems, self.drops, self.planner, self.obs = means, systems, drops, planner, obs or {}


_ORACLE = {}


def oracle_run(key, prob, tag, delta, trust, iters):
    """The oracle's iterations of one problem in one damping mode, computed once per session: [(d_theta, costs, means)], and per
    field how far the first step moves without its rows."""
    k = (key, tag)
    if k not in _ORACLE or len(_ORACLE[k][0]) < iters:
        ora = GP.OracleGPMP(prob.means, prob.systems, 0.5, delta, trust, "inverse")
        steps = []
        for _ in range(iters):
            d_o, c_o = ora.step(**prob.obs)
            steps.append((d_o, c_o, ora.particle_means.clone()))
        moved = {}
        for name, fn in prob.drops.items():
            d0, _ = GP.OracleGPMP(prob.means, fn, 0.5, delta, trust, "inverse").step(**prob.obs)
            moved[name] = DO.rel_l2(d0, steps[0][0])
        _ORACLE[k] = (steps, moved)
    return _ORACLE[k]


def run_case(key, prob, tag, delta, trust, kernel, ppw, iters=2):
    steps, moved = oracle_run(key, prob, tag, delta, trust, iters)
    for name, m in moved.items():                         # the condition: each field's rows matter to the step
        print(f"    {key} {tag}: without the {name} rows d_theta moves by {m:.3f} (relative L2)")
        assert m >= 0.05, (name, m)
    pl, obs = prob.planner(torch.float64, delta, trust)
    worst = [0., 0., 0.]
    for it in range(iters):
        d_o, c_o, m_o = steps[it]
        _, _, costs = pl.optimize(**obs)
        assert pl._engine.last_gpmp_kernel() == kernel, pl._engine.last_gpmp_kernel()
        assert pl._engine.last_gpmp_ppw() == ppw, pl._engine.last_gpmp_ppw()
        e = (rel_err(pl._d_theta, d_o), rel_err(costs, c_o), rel_err(pl.particle_means, m_o))
        print(f"    {key} {tag} iteration {it}: d_theta {e[0]:.2e} costs {e[1]:.2e} means {e[2]:.2e}")
        worst = [max(w, v) for w, v in zip(worst, e)]
        assert e[0] < 1e-7 and e[1] < 1e-9 and e[2] < 1e-8, (it, e)
    return worst


def line_means(q0, q1, T, P, dt, seed=4, noise=0.05, vnoise=0.3):
    """P particles on noisy straight lines in joint space from q0 to q1; velocities of the line plus noise (as the gpmp_means of
    tests/grid_sdf_oracle.py and tests/voxel_sdf_oracle.py)."""
    gen = torch.Generator().manual_seed(seed)
    q0, q1 = torch.tensor(q0, dtype=torch.float64), torch.tensor(q1, dtype=torch.float64)
    n = q0.numel()
    w = torch.linspace(0, 1, T, dtype=torch.float64).reshape(1, T, 1)
    means = torch.zeros(P, T, 2 * n, dtype=torch.float64)
    means[..., :n] = q0 + (q1 - q0) * w + noise * torch.randn(P, T, n, generator=gen, dtype=torch.float64)
    means[..., n:] = (q1 - q0) / ((T - 1) * dt) + vnoise * torch.randn(P, T, n, generator=gen, dtype=torch.float64)
    return means


# ------------------------------------------------------------------------------------------------ planar, N = 2, one grid field
def planar_problem(T, P=5, n_sub=0):
    means = GO.gpmp_means(T, P)
    limits = gpmp_limits(means) if n_sub > 0 else None

    def fn(**kw):
        return GO.gpmp_systems_fn(ref_sdf(), CELL, OFF, GO.MARGIN, n_sub, limits=limits, **kw)

    def planner(dtype, delta, trust):
        return planar_gpmp(means, dtype, delta, trust, n_sub, grid_field(dtype), limits), {}
    return Problem(means, fn(), {"grid field": fn(field=False)}, planner)


# T: request PPW x 8 T (32 + 9) bytes -- 49: 64 288 (the last under 64 KiB), 50: 65 600 (the first over), 117: 153 504 (the last at
# four per wave), 118: 77 408 (the first at two), 128: 83 968 (the cap).  P = 5: a full and a partial wave at four per wave, two full
# waves and a partial one at two.
@pytest.mark.parametrize("tag,delta,trust", MODES)
@pytest.mark.parametrize("T,ppw", [(49, 4), (50, 4), (117, 4), (118, 2), (128, 2)])
def test_planar_solve_at_the_lds_and_layout_boundaries(T, ppw, tag, delta, trust):
    run_case(f"planar T={T}", planar_problem(T), tag, delta, trust, THOMAS, ppw)


# ------------------------------------------------------------------------------------------------ Panda, N = 7, two fields
# ARM_C with both link fields of the Panda cost list; self_margin 0.2 (at tests/scenarios.py's 0.03 the self rows move nothing)
PANDA_C = dict(VO.ARM_C, sigma_coll=0.05, self_margin=0.2, sigma_self=0.05)


def chain_problem(c, means, goals, nppg, sph, chain=None):
    """GP + goal prior + self-distance + rbf spheres on a serial chain (None: the Panda)."""
    T = means.shape[1]
    FK = fk_all_links if chain is None else (lambda q: fk_all_links(q, chain))
    base = GP.panda_systems_fn(c, T, nppg, goals, FK)

    def without(i):
        return lambda m, **obs: [s for j, s in enumerate(base(m, **obs)) if j != i]

    def planner(dtype, delta, trust):
        ta = TA(dtype)
        cost = hip_panda_cost(c, T, nppg, 1, ta, goals=goals.to(**ta), chain=chain)
        return hip_gpmp(means, goals, nppg, ta, delta, trust, cost=cost, c=c), dict(obstacle_spheres=sph.to(**ta))
    return Problem(means, base, {"self-distance": without(2), "sphere": without(3)}, planner, dict(obstacle_spheres=sph))


def panda_problem(golden, T, P=5, goals=1):
    sph = torch.from_numpy(golden("g7_gpmp.npz")["spheres"])
    g = torch.tensor([PANDA_C["goal_q"] + [0.] * 7], dtype=torch.float64).repeat(goals, 1)
    if goals > 1:
        g[1:, :7] += torch.tensor([-0.3, 0.2, 0.1, 0.2, -0.1, -0.2, 0.1], dtype=torch.float64)
    return chain_problem(PANDA_C, VO.gpmp_means(T, P), g, P // goals, sph)


# T: request PPW x 8 T (32 + 18) bytes -- 40: 64 000 (under 64 KiB), 41: 65 600 (the first over), 96: 153 600 (exactly the threshold),
# 97: 77 600 (the first at two per wave)
@pytest.mark.parametrize("tag,delta,trust", MODES)
@pytest.mark.parametrize("T,ppw", [(40, 4), (41, 4), (96, 4), (97, 2)])
def test_panda_solve_at_the_lds_and_layout_boundaries(golden, T, ppw, tag, delta, trust):
    run_case(f"panda T={T}", panda_problem(golden, T), tag, delta, trust, THOMAS, ppw)


def test_panda_trust_region_with_a_row_pack_across_two_goals(golden):
    """T = 16, two goals of three particles: the first wave's four rows of 16 lanes hold particles of both goals (0, 1, 2 | 3), in
    trust-region mode with field rows that matter."""
    run_case("panda T=16 two goals", panda_problem(golden, 16, P=6, goals=2), "tr", 1e-2, True, THOMAS, 4)


# ------------------------------------------------------------------------------------------------ N = 6
def arm6_problem(T, P):
    chain = arm6()
    c, n = arm_config(chain)
    c = dict(VO.ARM_C, n_dof=n, start_q=c["start_q"], goal_q=c["goal_q"], dt=0.1, self_margin=0.2, sigma_self=0.05, sigma_coll=0.05)
    mid = 0.5 * (torch.tensor(c["start_q"], dtype=torch.float64) + torch.tensor(c["goal_q"], dtype=torch.float64))
    tool = fk_all_links(mid.reshape(1, n), chain)[0, -1, :3, 3]
    sph = torch.cat([tool + torch.tensor([0.05, 0.1, 0.], dtype=torch.float64), torch.tensor([0.12], dtype=torch.float64)]).reshape(1, 4)
    goals = torch.tensor([c["goal_q"] + [0.] * n], dtype=torch.float64)
    return chain_problem(c, line_means(c["start_q"], c["goal_q"], T, P, c["dt"]), goals, P, sph, chain=chain)


@pytest.mark.parametrize("tag,delta,trust", MODES)
@pytest.mark.parametrize("T,P", [(3, 5), (16, 6)])
def test_six_joint_arm_solve_matches_the_oracle(T, P, tag, delta, trust):
    run_case(f"arm6 T={T} P={P}", arm6_problem(T, P), tag, delta, trust, THOMAS, 4)


# ------------------------------------------------------------------------------------------------ no chain, no field: N = 3, fallback
BARE_C = dict(dt=0.1, cost_sigma_start=1e-2, cost_sigma_gp=0.5, sigma_goal_prior=1e-1, sigma_start_init=1e-3, sigma_goal_init=1e-3,
              sigma_gp_init=1., sigma_start_sample=1e-3, sigma_goal_sample=1e-3, sigma_gp_sample=0.1)


def bare_problem(n, T, P):
    """CostGP + CostGoalPrior on n degrees of freedom."""
    from stoch_gpmp_amd.costs.cost_functions import CostComposite, CostGP, CostGoalPrior
    c = BARE_C
    q0, q1 = [-0.5 + 0.1 * j for j in range(n)], [0.6 - 0.15 * j for j in range(n)]
    start = torch.tensor(q0 + [0.] * n, dtype=torch.float64)
    goals = torch.tensor([q1 + [0.] * n], dtype=torch.float64)
    means = line_means(q0, q1, T, P, c["dt"])

    def fn(m, **obs):
        return [GP.linear_system_gp(m, start, n, c["dt"], c["cost_sigma_start"], c["cost_sigma_gp"]),
                GP.linear_system_goal_prior(m, goals, P, n, c["sigma_goal_prior"])]

    def planner(dtype, delta, trust):
        ta = TA(dtype)
        cost = CostComposite(n, T, [CostGP(n, T, start.to(**ta), c["dt"], dict(sigma_start=c["cost_sigma_start"], sigma_gp=c["cost_sigma_gp"]), ta),
                                    CostGoalPrior(n, T, multi_goal_states=goals.to(**ta), num_particles_per_goal=P, num_samples=1,
                                                  sigma_goal_prior=c["sigma_goal_prior"], tensor_args=ta)], tensor_args=ta)
        return hip_gpmp(means, goals, P, ta, delta, trust, cost=cost, c=c, start=start.to(**ta)), {}
    return Problem(means, fn, {}, planner)


def diag_sum_is_exactly_zero(prob):
    """No field: the field part of sum_p diag(A^T K A) that gpmp_linearize hands the trust-region damping is zero, exactly."""
    pl, _ = prob.planner(torch.float64, 1e-2, True)
    P, T, d = prob.means.shape
    diag = torch.ones(T * d, device=DEV, dtype=torch.float64)
    pl._engine.gpmp_linearize(pl.particle_means, diag_sum=diag)
    assert bool((diag == 0.).all())


# T = 65: the first request over 64 KiB without fields (4 x 8 x 65 x 32 = 66 560 bytes)
@pytest.mark.parametrize("tag,delta,trust", MODES)
@pytest.mark.parametrize("T,P", [(2, 1), (3, 5), (65, 5)])
def test_three_joint_solve_matches_the_oracle(T, P, tag, delta, trust):
    prob = bare_problem(3, T, P)
    run_case(f"n=3 T={T} P={P}", prob, tag, delta, trust, THOMAS, 4)
    if trust:
        diag_sum_is_exactly_zero(prob)


# n = 8 fills the whole 16 x 16 tile of gpmp_solve_kernel, no padding
@pytest.mark.parametrize("tag,delta,trust", MODES)
@pytest.mark.parametrize("T,P", [(3, 5), (16, 4)])
@pytest.mark.parametrize("n", [1, 4, 5, 8])
def test_fallback_kernel_at_the_joint_counts_that_take_it(n, T, P, tag, delta, trust):
    prob = bare_problem(n, T, P)
    run_case(f"n={n} T={T} P={P}", prob, tag, delta, trust, FALLBACK, 0)
    if trust:
        diag_sum_is_exactly_zero(prob)


# ------------------------------------------------------------------------------------------------ fp32 at the long shapes
@pytest.mark.parametrize("which,T", [("planar", 128), ("panda", 97)])
def test_fp32_at_the_longest_shapes_against_the_fp64_oracle(golden, which, T):
    """One Levenberg iteration of an fp32 context (the kernel computes in double on fp32 inputs) at two particles per wave."""
    prob = planar_problem(T) if which == "planar" else panda_problem(golden, T)
    steps, _ = oracle_run(f"{which} T={T}", prob, "lm", 5.0, False, 1)
    pl, obs = prob.planner(torch.float32, 5.0, False)
    _, _, costs = pl.optimize(**obs)
    assert pl._engine.last_gpmp_kernel() == THOMAS and pl._engine.last_gpmp_ppw() == 2
    e = (rel_err(costs, steps[0][1]), rel_err(pl.particle_means, steps[0][2]))
    print(f"    fp32 {which} T={T}: costs {e[0]:.3e} means {e[1]:.3e} (relative, against the fp64 oracle)")
    assert e[0] < FP32_BAR and e[1] < FP32_BAR, e


# ------------------------------------------------------------------------------------------------ continuous-time solve at the cap
@pytest.mark.parametrize("tag,delta,trust", MODES)
def test_dense_solve_at_the_largest_traj_len(tag, delta, trust):
    """gpmp_dense_solve_kernel at traj_len = 128 (its staging scales with T as well): planar, P = 3, n_sub = 1, limit rows."""
    run_case("planar dense T=128", planar_problem(128, P=3, n_sub=1), tag, delta, trust, DENSE, 0)


@pytest.mark.parametrize("n_sub", [0, 1])
def test_traj_len_129_is_refused_before_any_launch(n_sub):
    from stoch_gpmp_amd import _lib
    prob = planar_problem(129, P=3, n_sub=n_sub)
    pl, obs = prob.planner(torch.float64, 5.0, False)
    before = pl.particle_means.clone()
    with pytest.raises((ValueError, _lib.SgpmpError), match=r"traj_len must be in \[2, 128\]"):
        pl.optimize(**obs)
    assert torch.equal(pl.particle_means, before)
