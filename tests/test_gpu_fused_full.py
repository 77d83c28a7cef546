"""fused_step_kernel with the four-term cost program compiled in (csrc/fused_step.inc: FULL; csrc/step_plan.hip:
fused_full_variant) against the generic instantiation, which reads the program at run time: which launch takes which, and
that the two give the same bits.  Needs the MI355X: run with `-m gpu`.

The variant a launch reports (Engine.last_fused_variant): 0 generic, 1 compiled in without softmax partials, 2 compiled in
with the partials buffer armed.  A default context arms the partials for every chain-code step on the launch's 8 x 16 grid
(step_plan.hip: plan.partials), so the default set-up reports 2 and `no_dense_partials` 1; both are held to the generic
kernel here.  (The context keeps the fp64 copy of the costs to itself -- the fp32 row sums widened, what the update reads: the
weights, means and gradient compared below are computed from it.)"""
import pytest
import torch

from tests import scenarios as SC
from tests.hip_builders import hip_panda_planner

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32 = {"device": DEV, "dtype": torch.float32}
GOALS2 = [SC.PANDA["goal_q"] + [0.] * 7, [0.3, 0.1, 0.2, -1.2, 0.0, 1.8, 0.2] + [0.] * 7]

# (particles per goal, S, T, goals): one group and one chunk -- start and goal unary factors in the same chunk; three groups per
# particle (particle index by division) with a chunk carry; two goals x 2 particles, three chunks, goal index by division
# (rows per goal 2 x 16 is a power of two: the shift -- with three particles per goal below, the division)
SHAPES = {"one_chunk": (4, 8, 16, None), "three_groups": (3, 24, 32, None), "two_goals": (2, 16, 48, GOALS2),
          "two_goals_by_division": (3, 16, 48, GOALS2)}


def _spheres():
    return torch.as_tensor(SC.panda_spheres(num=5, seed=23)).to(**F32)


def _planner(nppg, S, T, goals, options=(), **kw):
    if goals is not None:
        kw["goals"] = goals
    pl = hip_panda_planner(SC.PANDA, T, nppg, S, F32, seed=81, **kw)
    pl._engine.set_option("no_small_step", 1)            # fused_step_kernel itself, whatever the number of items
    for name in options:
        pl._engine.set_option(name, 1)
    return pl


def _same_bits(a, b, sph, variant):
    """One storing step, then three iterations in one call (two of them store-free, generic in both planners; the last storing)."""
    for k in (1, 3):
        ra, rb = a.optimize(opt_iters=k, obstacle_spheres=sph), b.optimize(opt_iters=k, obstacle_spheres=sph)
        assert a._engine.last_cost_kernel() == "fused_step_kernel" and b._engine.last_cost_kernel() == "fused_step_kernel"
        assert a._engine.last_fused_variant() == variant and b._engine.last_fused_variant() == 0
        for i, (x, y) in enumerate(zip(ra, rb)):
            assert torch.equal(x, y), (k, i)
        assert torch.equal(a.state_samples, b.state_samples) and torch.equal(a._costs, b._costs), k
        assert torch.equal(a.particle_means, b.particle_means), k
        assert torch.equal(a._weights_buf, b._weights_buf) and torch.equal(a._grad, b._grad), k


@pytest.mark.parametrize("partials", [False, True], ids=["no_partials", "partials_armed"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_compiled_in_program_equals_the_generic_kernel_bitwise(shape, partials):
    nppg, S, T, goals = SHAPES[shape]
    opts = () if partials else ("no_dense_partials",)
    a = _planner(nppg, S, T, goals, opts)
    b = _planner(nppg, S, T, goals, opts + ("fused_generic",))
    _same_bits(a, b, _spheres(), 2 if partials else 1)


@pytest.mark.parametrize("field_type", ["sdf", "occupancy"])
def test_compiled_in_program_for_the_other_field_types(field_type):
    for opts, variant in ((("no_dense_partials",), 1), ((), 2)):
        a = _planner(3, 24, 32, None, opts, field_type=field_type)
        b = _planner(3, 24, 32, None, opts + ("fused_generic",), field_type=field_type)
        _same_bits(a, b, _spheres(), variant)


def test_partials_in_use_equal_the_generic_kernel_bitwise():
    """Spread weights: the launch with the partials armed (variant 2) also WRITES them, and the update adds them."""
    cfg = dict(SC.PANDA, temperature=1e14, sigma_start_sample=1.0, sigma_goal_sample=1.0, sigma_gp_sample=30.0)
    sph = _spheres()
    a = hip_panda_planner(cfg, 32, 6, 64, F32, seed=81)
    b = hip_panda_planner(cfg, 32, 6, 64, F32, seed=81)
    for pl in (a, b):
        pl._engine.set_option("no_small_step", 1)
        pl._engine.set_option("store_free_min_bytes", 0)   # every step stores: every launch is the variant under test
    b._engine.set_option("fused_generic", 1)
    for k in (1, 1, 2):
        a.optimize(opt_iters=k, obstacle_spheres=sph)
        b.optimize(opt_iters=k, obstacle_spheres=sph)
        assert a._engine.last_fused_variant() == 2 and b._engine.last_fused_variant() == 0
        assert torch.equal(a.state_samples, b.state_samples) and torch.equal(a._costs, b._costs), k
        assert torch.equal(a.particle_means, b.particle_means) and torch.equal(a._weights_buf, b._weights_buf), k
        assert torch.equal(a._grad, b._grad), k
    assert a._engine.dense_armed_steps() == 4 and int(a._engine.row_counts().max()) > 16


def _step(pl, sph, iters=1):
    pl.optimize(opt_iters=iters, obstacle_spheres=sph)
    return pl._engine.last_cost_kernel(), pl._engine.last_fused_variant()


def test_everything_else_takes_the_generic_kernel():
    """Dispatch: another program, another mode or another launch reports variant 0 (and the four-term storing step beside it 1 / 2)."""
    from stoch_gpmp_amd.costs.cost_functions import CostGoal, CostGPTrajectory
    from stoch_gpmp_amd.costs.fields import EESE3DistanceField
    from oracle.fk import fk_all_links
    from tests.arm_chains import arm7, arm_config
    sph = _spheres()
    T, nppg, S = 32, 3, 16
    assert _step(_planner(nppg, S, T, None), sph) == ("fused_step_kernel", 2)
    assert _step(_planner(nppg, S, T, None, ("no_dense_partials",)), sph) == ("fused_step_kernel", 1)
    assert _step(_planner(nppg, S, T, None, ("fused_generic",)), sph) == ("fused_step_kernel", 0)
    # an end-effector goal term beside the four
    pl = _planner(nppg, S, T, None)
    H = fk_all_links(torch.tensor([[0.3, -0.5, 0.2, -1.9, 0.1, 1.6, 0.4]], dtype=torch.float64))[0, -1].clone()
    pl.cost.cost_list.append(CostGoal(7, T, field=EESE3DistanceField(H, w_pos=1., w_rot=0.5, tensor_args=F32), sigma_goal=1e-2, tensor_args=F32))
    assert _step(pl, sph) == ("fused_step_kernel", 0)
    # a missing term: no self term, no sphere term
    for drop in (2, 3):
        pl = _planner(nppg, S, T, None)
        del pl.cost.cost_list[drop]
        assert _step(pl, sph) == ("fused_step_kernel", 0), drop
    # a GP term without the start prior
    pl = _planner(nppg, S, T, None)
    gp = pl.cost.cost_list[0]
    pl.cost.cost_list[0] = CostGPTrajectory(7, T, gp.start_state, gp.dt, dict(sigma_gp=gp.sigma_gp), F32)
    pl.cost._version += 1                                # (an edit of the list itself: compile the program again)
    assert _step(pl, sph) == ("fused_step_kernel", 0)
    # store-free steps: the iterations of one call whose samples nobody reads (the call's last iteration stores)
    pl = _planner(nppg, S, T, None)
    assert _step(pl, sph) == ("fused_step_kernel", 2)
    pl.step(_samples_unread=True, obstacle_spheres=sph)
    assert pl._engine.store_free_steps() == 1 and pl._engine.last_fused_variant() == 0
    assert _step(pl, sph, iters=3) == ("fused_step_kernel", 2) and pl._engine.store_free_steps() == 3    # (a call's last iteration stores)
    # shapes off the 8 x 16 grid: S not a multiple of 8, T not a multiple of 16
    assert _step(_planner(nppg, 12, T, None), sph) == ("fused_step_kernel", 0)
    assert _step(_planner(nppg, S, 24, None), sph) == ("fused_step_kernel", 0)
    # the small-step launch
    pl = _planner(nppg, S, T, None)
    pl._engine.set_option("no_small_step", 0)
    assert _step(pl, sph) == ("fused_step_small_kernel", 0)
    # chain code compiled at run time
    chain = arm7()
    c, _ = arm_config(chain)
    pl = hip_panda_planner(c, T, nppg, S, F32, seed=19, chain=chain)
    pl._engine.set_option("no_small_step", 1)
    assert _step(pl, sph) == ("fused_step_kernel (run-time chain code)", 0)
