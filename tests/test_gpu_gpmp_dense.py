"""GPMP with continuous-time factors (GPMP.set_dense_cost -> sgpmp_gpmp_set_dense; csrc/gpmp_dense.hip) against the test-local dense
oracle (tests/gpmp_dense_oracle.py: autograd rows appended to oracle.gpmp_equiv's systems, solved by OracleGPMP "inverse").

fp64 tolerances: the project's own from test_gpmp_matches_reference_run_and_oracle -- d_theta 1e-7, costs 1e-9, means 1e-8, relative.
Every parity test first asserts, on the oracle alone, that the part it covers moves d_theta by at least 0.05 (relative L2)."""
import numpy as np
import pytest
import torch

from oracle import gpmp_equiv as GP
from tests import gpmp_dense_oracle as DO
from tests import scenarios as SC
from tests.hip_builders import hip_panda_cost

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F64 = {"device": DEV, "dtype": torch.float64}
F32 = {"device": DEV, "dtype": torch.float32}
C = SC.PANDA
MODES = [("lm", 5.0, False), ("tr", 1e-2, True)]


def rel_err(a, b):
    a, b = a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / np.abs(b).max())


def hip_gpmp(means, goals, nppg, ta, delta, trust, dense_cost=None, field_type="rbf", clamp=False, cost=None, c=C, start=None):
    """A GPMP planner on `means` [P,T,2n] (P = goals x nppg) with the Panda cost list of tests/scenarios.py (or `cost`)."""
    from stoch_gpmp_amd.planner import GPMP
    P, T, d = means.shape
    n = d // 2
    goals = goals.to(**ta)
    if cost is None:
        cost = hip_panda_cost(c, T, nppg, 1, ta, goals=goals, field_type=field_type, clamp_sdf=clamp)
    if start is None:
        start = torch.tensor(c["start_q"] + [0.] * n, **ta)
    kw = {} if dense_cost is None else {"dense_cost": dense_cost}
    return GPMP(num_particles_per_goal=nppg, traj_len=T, opt_iters=1, dt=c["dt"], n_dof=n, step_size=0.5, temperature=1.,
                start_state=start, multi_goal_states=goals, initial_particle_means=means.to(**ta).reshape(-1, nppg, T, d),
                cost=cost, sigma_start_init=c["sigma_start_init"], sigma_start_sample=c["sigma_start_sample"],
                sigma_goal_init=c["sigma_goal_init"], sigma_goal_sample=c["sigma_goal_sample"],
                sigma_gp_init=c["sigma_gp_init"], sigma_gp_sample=c["sigma_gp_sample"], seed=0,
                solver_params=dict(delta=delta, trust_region=trust, method="cholesky"), tensor_args=ta, **kw)


def setting_dict(n_sub, s, parts):
    """GPMP.set_dense_cost's dict from an oracle setting: `parts` names what is on ('weight', 'q_lo', 'q_hi', 'v_max')."""
    ql = (s["q_lo"] if "q_lo" in parts else None, s["q_hi"] if "q_hi" in parts else None)
    limits = any(k in parts for k in ("q_lo", "q_hi", "v_max"))
    return dict(n_sub=n_sub, weight=s["weight"] if "weight" in parts else 0.,
                q_limits=ql if ("q_lo" in parts or "q_hi" in parts) else None, v_limits=s["v_max"] if "v_max" in parts else None,
                sigma_limit=s["sigma_limit"] if limits else None)


def oracle_pair(means, goals, nppg, n_sub, delta, trust, s, parts, field_type="rbf", clamp=False):
    """(oracle with the parts, oracle without them) on the Panda cost list."""
    T = means.shape[1]
    lim = {k: s[k] for k in ("q_lo", "q_hi", "v_max") if k in parts}
    fn = DO.panda_dense_systems_fn(C, T, nppg, goals, n_sub, weight=s["weight"] if "weight" in parts else 0.,
                                   sigma_limit=s["sigma_limit"], sphere_field=field_type, clamp_sdf=clamp, **lim)
    fn0 = DO.panda_dense_systems_fn(C, T, nppg, goals, n_sub, sphere_field=field_type, clamp_sdf=clamp, collision=False, limits=False)
    return (GP.OracleGPMP(means, fn, 0.5, delta, trust, "inverse"), GP.OracleGPMP(means, fn0, 0.5, delta, trust, "inverse"))


def run_parity(means, goals, nppg, sph, n_sub, delta, trust, s, parts, iters, field_type="rbf", clamp=False):
    ora, ora0 = oracle_pair(means, goals, nppg, n_sub, delta, trust, s, parts, field_type, clamp)
    pl = hip_gpmp(means, goals, nppg, F64, delta, trust, dense_cost=setting_dict(n_sub, s, parts), field_type=field_type, clamp=clamp)
    d0, _ = ora0.step(obstacle_spheres=sph)
    for it in range(iters):
        d_o, c_o = ora.step(obstacle_spheres=sph)
        if it == 0:                                       # the condition: these rows matter to the step
            moved = DO.rel_l2(d0, d_o)
            print(f"parts {parts} n_sub {n_sub}: the rows move d_theta by {moved:.3f} (relative L2)")
            assert moved >= 0.05, moved
        _, _, costs = pl.optimize(obstacle_spheres=sph.to(**F64))
        assert pl._engine.last_gpmp_kernel() == "gpmp_dense_solve_kernel"
        e = (rel_err(pl._d_theta, d_o), rel_err(costs, c_o), rel_err(pl.particle_means, ora.particle_means))
        print(f"  iteration {it}: d_theta {e[0]:.2e} costs {e[1]:.2e} means {e[2]:.2e}")
        assert e[0] < 1e-7 and e[1] < 1e-9 and e[2] < 1e-8, (it, e)


def g7_inputs(golden, tag="lm"):
    g = golden("g7_gpmp.npz")
    T, nppg = [int(v) for v in g["dims"]]
    return g, torch.from_numpy(g[f"{tag}/means0"]), torch.from_numpy(g["goals"]), nppg, torch.from_numpy(g["spheres"])


ALL = ("weight", "q_lo", "q_hi", "v_max")


@pytest.mark.parametrize("n_sub", [1, 3])
@pytest.mark.parametrize("tag,delta,trust", MODES)
def test_full_step_on_g7_matches_oracle(golden, tag, delta, trust, n_sub):
    """Collision rows on the inserted states and all three limit rows, rbf, both damping modes, three iterations."""
    g, means, goals, nppg, sph = g7_inputs(golden, tag)
    run_parity(means, goals, nppg, sph, n_sub, delta, trust, DO.g7_setting(g), ALL, 3)


@pytest.mark.parametrize("n_sub", [0, 3])
def test_trust_region_diag_sum_matches_oracle(golden, n_sub):
    """diag_sum of sgpmp_gpmp_linearize with the option on: the field-and-dense part of sum_p diag(A^T K A), velocity entries and
    waypoint 0 included, to 1e-9."""
    g, means, goals, nppg, sph = g7_inputs(golden, "tr")
    s = DO.g7_setting(g)
    ora, _ = oracle_pair(means, goals, nppg, n_sub, 1e-2, True, s, ALL)
    want = DO.field_dense_diag(ora.systems_fn(means, obstacle_spheres=sph))
    pl = hip_gpmp(means, goals, nppg, F64, 1e-2, True, dense_cost=setting_dict(n_sub, s, ALL))
    diag = torch.zeros(means.shape[1] * means.shape[2], device=DEV, dtype=torch.float64)
    pl._engine.gpmp_linearize(pl.particle_means, spheres=sph.to(**F64), diag_sum=diag)
    T, d = means.shape[1:]
    w = want.reshape(T, d)
    assert float(w[0].abs().max()) > 0. and float(w[:, d // 2:].abs().max()) > 0.     # waypoint 0 and velocity entries carry rows
    assert rel_err(diag, want) < 1e-9


@pytest.mark.parametrize("parts,n_sub", [(("weight",), 3), (("q_lo", "q_hi", "v_max"), 0), (("q_lo", "q_hi", "v_max"), 3),
                                         (("q_lo",), 3), (("v_max",), 3)])
@pytest.mark.parametrize("tag,delta,trust", MODES[:1])
def test_parts_alone_match_oracle(golden, tag, delta, trust, parts, n_sub):
    g, means, goals, nppg, sph = g7_inputs(golden, tag)
    run_parity(means, goals, nppg, sph, n_sub, delta, trust, DO.g7_setting(g), parts, 2)


@pytest.mark.parametrize("clamp", [False, True])
def test_sdf_fields_match_oracle(golden, clamp):
    """The signed-distance sphere field (arg-max rule) on the inserted states, n_sub = 2."""
    g, means, goals, nppg, sph = g7_inputs(golden)
    run_parity(means, goals, nppg, sph, 2, 5.0, False, DO.g7_setting(g), ALL, 2, field_type="sdf", clamp=clamp)


def small_setting(means):
    n = means.shape[-1] // 2
    q, v = means[..., :n].reshape(-1, n), means[..., n:].reshape(-1, n).abs()
    return dict(weight=1e3, sigma_limit=1e-4, q_lo=torch.quantile(q, 0.3, dim=0), q_hi=torch.quantile(q, 0.7, dim=0),
                v_max=torch.quantile(v, 0.6, dim=0))


@pytest.mark.parametrize("T,P,n_sub", [(2, 1, 3), (3, 5, 2), (3, 1, 31)])
def test_smallest_shapes_match_oracle(golden, T, P, n_sub):
    """T = 2 (one interval, no carried block), T = 3, P = 1 and P = 5, the largest n_sub: the first T waypoints of the fixture's
    particles as a problem of their own."""
    g, means, goals, nppg, sph = g7_inputs(golden)
    means = means[:P, :T].contiguous()
    run_parity(means, goals[:1], P, sph, n_sub, 5.0, False, small_setting(means), ALL, 2 if n_sub < 31 else 1)


def test_planar_problem_without_a_chain_matches_oracle():
    """n = 2, no FK chain and no field: GP + goal prior + limit rows only, n_sub = 2, T = 5, P = 3."""
    from stoch_gpmp_amd.costs.cost_functions import CostComposite, CostGP, CostGoalPrior
    c = dict(SC.PLANAR, cost_sigma_start=1e-2, cost_sigma_gp=0.5, sigma_goal_prior=1e-1)
    n, T, P, n_sub = 2, 5, 3, 2
    gen = torch.Generator().manual_seed(4)
    start = torch.tensor([-1., -1., 0., 0.], dtype=torch.float64)
    goals = torch.tensor([[1., 0.5, 0., 0.]], dtype=torch.float64)
    means = torch.zeros(P, T, 4, dtype=torch.float64)
    means[..., :2] = start[:2] + (goals[0, :2] - start[:2]) * torch.linspace(0, 1, T).reshape(1, T, 1)
    means += 0.3 * torch.randn(P, T, 4, generator=gen, dtype=torch.float64)
    means[..., 2:] *= 10.
    s = dict(small_setting(means), sigma_limit=1e-2)
    cost = CostComposite(n, T, [CostGP(n, T, start.to(**F64), c["dt"], dict(sigma_start=c["cost_sigma_start"], sigma_gp=c["cost_sigma_gp"]), F64),
                                CostGoalPrior(n, T, multi_goal_states=goals.to(**F64), num_particles_per_goal=P, num_samples=1,
                                              sigma_goal_prior=c["sigma_goal_prior"], tensor_args=F64)], tensor_args=F64)
    parts = ("q_lo", "q_hi", "v_max")
    pl = hip_gpmp(means, goals, P, F64, 1.0, False, dense_cost=setting_dict(n_sub, s, parts), cost=cost, c=c, start=start.to(**F64))

    def systems(lim):
        def fn(m, **obs):
            return [GP.linear_system_gp(m, start, n, c["dt"], c["cost_sigma_start"], c["cost_sigma_gp"]),
                    GP.linear_system_goal_prior(m, goals, P, n, c["sigma_goal_prior"])] + DO.dense_systems(m, n, n_sub, c["dt"], **lim)
        return fn
    ora = GP.OracleGPMP(means, systems(dict(q_lo=s["q_lo"], q_hi=s["q_hi"], v_max=s["v_max"], sigma_limit=s["sigma_limit"])),
                        0.5, 1.0, False, "inverse")
    ora0 = GP.OracleGPMP(means, systems({}), 0.5, 1.0, False, "inverse")
    d0, _ = ora0.step()
    for it in range(2):
        d_o, c_o = ora.step()
        if it == 0:
            assert DO.rel_l2(d0, d_o) >= 0.05
        _, _, costs = pl.optimize()
        assert pl._engine.last_gpmp_kernel() == "gpmp_dense_solve_kernel"
        assert rel_err(pl._d_theta, d_o) < 1e-7 and rel_err(costs, c_o) < 1e-9
        assert rel_err(pl.particle_means, ora.particle_means) < 1e-8


def test_fp32_against_the_fp64_oracle(golden):
    """Costs and means of an fp32 context within the project's 1e-4 of the fp64 oracle (test_gpmp_fp32_and_errors' bound).
    Measured on the MI355X: costs 3.5e-8, means 3.4e-7 (profiles/r09/gpmp_dense.txt)."""
    g, means, goals, nppg, sph = g7_inputs(golden)
    s = DO.g7_setting(g)
    ora, _ = oracle_pair(means, goals, nppg, 3, 5.0, False, s, ALL)
    d_o, c_o = ora.step(obstacle_spheres=sph)
    pl = hip_gpmp(means, goals, nppg, F32, 5.0, False, dense_cost=setting_dict(3, s, ALL))
    _, _, costs = pl.optimize(obstacle_spheres=sph.to(**F32))
    e = (rel_err(costs, c_o), rel_err(pl.particle_means, ora.particle_means))
    print(f"fp32 with the continuous-time rows: costs {e[0]:.3e} means {e[1]:.3e} (relative, against the fp64 oracle)")
    assert e[0] < 1e-4 and e[1] < 1e-4, e


def test_off_is_off(golden):
    """set_dense_cost(None), n_sub = 0 with weight = 0 and no limits, and a planner that never had the option: the same bits, and
    the kernel of the plain solve; with the option on, gpmp_dense_solve_kernel."""
    g, means, goals, nppg, sph = g7_inputs(golden)
    s = DO.g7_setting(g)
    never = hip_gpmp(means, goals, nppg, F64, 5.0, False)
    was_on = hip_gpmp(means, goals, nppg, F64, 5.0, False, dense_cost=setting_dict(3, s, ALL))
    was_on.optimize(obstacle_spheres=sph.to(**F64))
    assert was_on._engine.last_gpmp_kernel() == "gpmp_dense_solve_kernel" and was_on.state_dict()["dense_cost"]["n_sub"] == 3
    was_on.set_dense_cost(None)
    was_on.particle_means.copy_(never.particle_means)
    zero = hip_gpmp(means, goals, nppg, F64, 5.0, False, dense_cost=dict(n_sub=0, weight=0.))
    outs = []
    for pl in (never, was_on, zero):
        for it in range(2):
            _, _, costs = pl.optimize(obstacle_spheres=sph.to(**F64))
            assert pl._engine.last_gpmp_kernel() == "gpmp_thomas_kernel"
        outs.append((pl._d_theta.clone(), costs.clone(), pl.particle_means.clone()))
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o, outs[0]))
    assert never.state_dict()["dense_cost"] is None


def test_errors_come_before_any_launch(golden):
    from stoch_gpmp_amd import _lib
    g, means, goals, nppg, sph = g7_inputs(golden)
    pl = hip_gpmp(means, goals, nppg, F64, 5.0, False)
    lo = torch.zeros(7)
    for bad in (dict(n_sub=32), dict(n_sub=2, weight=-1.), dict(n_sub=2, q_limits=(lo, None), sigma_limit=0.)):
        with pytest.raises(ValueError):
            pl.set_dense_cost(bad)
    eng = pl._engine
    for args in ((32, 0.05, 1.0), (2, 0.05, -1.0), (2, 0.0, 1.0)):
        with pytest.raises((ValueError, _lib.SgpmpError)):
            eng.gpmp_set_dense(*args)
    with pytest.raises((ValueError, _lib.SgpmpError)):
        eng.gpmp_set_dense(2, 0.05, 1.0, q_limits=(lo, None), sigma_limit=0.)
    # an occupancy field is still refused, with the option on, before anything is launched
    occ = hip_gpmp(means, goals, nppg, F64, 5.0, False, field_type="occupancy", dense_cost=dict(n_sub=2, weight=1.0))
    before = occ.particle_means.clone()
    with pytest.raises((ValueError, _lib.SgpmpError)):
        occ.optimize(obstacle_spheres=sph.to(**F64))
    assert torch.equal(occ.particle_means, before)
