"""update_kernel_quad (one wave per particle, four particles per workgroup; development switch `update_wide` = -1: wherever it
can run) against update_kernel (one 256-thread workgroup per particle; `update_wide` = 1) bit for bit, and against the fp64
reference of tests/update_oracle.py with the bounds of tests/test_gpu_update.py -- at the shapes where the one-wave form can go
wrong: a short last workgroup (P = 1, 3, 5, 130; 130 also wraps the statistics shards), S across the virtual waves of the
256-thread reduction order (63 / 64 / 65, 128 / 129, 255 / 256, and 257: a virtual thread with two costs) and the ballot groups,
both vector widths and several passes of the element loop, whole and ragged (M = 6, 30, 518, 1024, 1036), the three dtype
pairs, every cost regime.  The default rule (update_wide = 0: halves of a two-chain step of 512 to 1023 particles) is checked on the
names of the kernels launched.  Then single steps with the tail and the row counts at short workgroups, and two chains of a Panda optimize() with the importance-sampling tail, the row counts and the
softmax partials in play.

Engine.update (sgpmp_update) launches the update without the tail and without row counts, so those two outputs are compared
where they exist: through Engine.step and the planners (the row counts directly; the next step's IS weights through the costs,
weights and means of the step that consumes them).  Needs the MI355X: run with `-m gpu`."""
import functools

import pytest
import torch

from tests import scenarios as SC
from tests import update_oracle as U
from tests.hip_builders import hip_panda_planner

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32 = {"device": DEV, "dtype": torch.float32}
EPS32, TINY32 = 2. ** -23, 2. ** -149

QUAD_SHAPES = [  # n, T, P, S
    (1, 3, 1, 1),        # M = 6: two elements per lane; one particle, one sample: three waves of the workgroup have no particle
    (3, 5, 3, 5),        # M = 30; P = 3: one wave without a particle
    (7, 37, 5, 63),      # M = 518: two elements per lane, five passes of the element loop; P = 5: a second, short workgroup
    (8, 64, 4, 64),      # M = 1024: four elements per lane, exactly four passes; P = 4: one full workgroup; one full virtual wave
    (7, 74, 5, 65),      # M = 1036: four elements per lane, a fifth pass with three live lanes; second virtual wave with one cost
    (2, 4, 130, 128),    # P = 130 = 32 workgroups + 2 particles: the statistics shards wrap; two full virtual waves
    (2, 4, 5, 129),      # third virtual wave with one cost
    (2, 4, 3, 255),      # last virtual wave one short
    (2, 4, 5, 256),      # every virtual thread has one cost
    (2, 4, 4, 257),      # virtual thread 0 has two
]
IDS = [f"n{n}-T{T}-P{P}-S{S}" for n, T, P, S in QUAD_SHAPES]


def TA(dtype):
    return {"device": DEV, "dtype": dtype}


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def worst(err, bound):
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max())


def run_update(eng, case):
    real = case["real"]
    P, S, T, d = case["samples"].shape
    means = case["means"].to(DEV).clone()
    w = torch.full((P, S), 12345.0, **TA(real))
    g = torch.full((P, T, d), 12345.0, **TA(real))
    mp = torch.full((P, T, d), 12345.0, **TA(real))
    stats = torch.zeros(64, 4, device=DEV, dtype=torch.float64)
    eng.update(case["costs"].to(DEV), case["samples"].to(DEV), means, case["tau"], case["step"], weights=w, grad=g,
               means_prev=mp, stats=stats)
    torch.cuda.synchronize()
    return dict(weights=w.cpu(), grad=g.cpu(), means_prev=mp.cpu(), means=means.cpu(), stats=stats.cpu())


@functools.lru_cache(maxsize=None)
def both_forms(shape, dtype_name):
    """-> [(regime name, case, outputs of update_kernel_quad, outputs of update_kernel)] -- run once, shared by the tests."""
    from stoch_gpmp_amd.engine import Engine
    n, T, P, S = shape
    eng = Engine(n, T, P, S, tensor_args=TA(U.UPDATE_DTYPES[dtype_name][0]))
    out = []
    try:
        for regime in U.update_regimes(S):
            case = U.update_case(shape, dtype_name, regime)
            eng.set_option("update_wide", -1)
            new = run_update(eng, case)
            eng.set_option("update_wide", 1)
            old = run_update(eng, case)
            out.append((regime[0], case, new, old))
    finally:
        eng.set_option("update_wide", 0)                 # (the switch is process-wide)
        eng.close()
    return out


@pytest.mark.parametrize("dtype_name", list(U.UPDATE_DTYPES))
@pytest.mark.parametrize("shape", QUAD_SHAPES, ids=IDS)
def test_one_wave_update_equals_the_workgroup_update_bitwise(shape, dtype_name):
    P = shape[2]
    for name, case, new, old in both_forms(shape, dtype_name):
        for key in ("weights", "grad", "means", "means_prev"):
            assert same_bits(new[key], old[key]), (name, key)
        assert same_bits(new["means_prev"], case["means"]), name
        assert float(new["weights"].double().sum()) > 0, name
        # statistics: counts exactly; the two sums arrive by atomics in any order in both forms
        sn, so = new["stats"], old["stats"]
        assert sn[:, 2].tolist() == so[:, 2].tolist() and float(sn[:, 2].sum()) == P and bool((sn[:, 3] == 0).all()), name
        for k in (0, 1):
            a, b = float(sn[:, k].sum()), float(so[:, k].sum())
            assert abs(a - b) <= 1e-12 * abs(b), (name, k, a, b)


@pytest.mark.parametrize("dtype_name", list(U.UPDATE_DTYPES))
@pytest.mark.parametrize("shape", QUAD_SHAPES, ids=IDS)
def test_one_wave_update_matches_fp64_softmax_reference(shape, dtype_name):
    """The bounds are those of tests/test_gpu_update.py::test_update_matches_fp64_softmax_reference (lines 73-80 there: weights,
    gradient and means in fp64 and fp32; lines 92-95: the statistics)."""
    n, T, P, S = shape
    real = U.UPDATE_DTYPES[dtype_name][0]
    for name, case, new, _ in both_forms(shape, dtype_name):
        tau, step = case["tau"], case["step"]
        w_ref, g_ref, mu_ref, A = U.update_reference(case["costs"], case["samples"], case["means"], tau, step)
        assert (w_ref != 0).sum(1).tolist() == [case["expect"]] * P, name
        wd, gd, mud = new["weights"].double(), new["grad"].double(), new["means"].double()
        if real == torch.float64:
            bw = 1e-11 * w_ref.abs() + 1e-300
            bg = 1e-10 * A + 1e-14
            bm = 1e-12 * mu_ref.abs() + step * 1e-10 * A
        else:
            bw = EPS32 * w_ref.abs() + TINY32
            bg = 2. ** -22 * A
            bm = EPS32 * mu_ref.abs() + step * 2. ** -22 * A
        rw, rg, rm = worst((wd - w_ref).abs(), bw), worst((gd - g_ref).abs(), bg), worst((mud - mu_ref).abs(), bm)
        print(f"{name}: weights {rw:.3g}, grad {rg:.3g}, means {rm:.3g} of their bounds")
        assert bool(torch.isfinite(gd).all()) and bool(torch.isfinite(mud).all()), name
        assert rw <= 1, (name, "weights", rw)
        assert rg <= 1, (name, "grad", rg)
        assert rm <= 1, (name, "means", rm)
        tot, mins, cnt, per_shard = U.stats_reference(case["costs"])
        st = new["stats"]
        assert bool((st[:, 3] == 0).all())
        assert abs(float(st[:, 0].sum()) - tot) <= 1e-12 * abs(tot), (name, float(st[:, 0].sum()), tot)
        assert abs(float(st[:, 1].sum()) - mins) <= 1e-12 * abs(mins), (name, float(st[:, 1].sum()), mins)
        assert st[:, 2].tolist() == per_shard.tolist() and float(st[:, 2].sum()) == cnt, name


def update_kernels_launched(fn):
    """Names of the update kernels `fn` launches, as the device activity record of torch.profiler has them."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if "update_kernel" in e.name]


def test_a_launch_that_is_not_half_of_a_two_chain_step_keeps_the_workgroup_kernel():
    """The default rule takes update_kernel_quad only for the halves of a two-chain step (tests below): sgpmp_update's launch
    keeps update_kernel even at a shape inside the rule's bounds; the switch overrules the rule both ways at any shape."""
    from stoch_gpmp_amd.engine import Engine
    for P, S in ((512, 128), (4, 257)):
        shape = (1, 2, P, S)
        eng = Engine(1, 2, P, S, tensor_args=TA(torch.float32))
        case = U.update_case(shape, "f32_costs64", ("spread", S, None))
        try:
            for wide, quad_expected in ((0, False), (1, False), (-1, True)):
                eng.set_option("update_wide", wide)
                names = update_kernels_launched(lambda: run_update(eng, case))
                assert len(names) == 1, (P, S, wide, names)
                assert ("update_kernel_quad" in names[0]) == quad_expected, (P, S, wide, names)
        finally:
            eng.set_option("update_wide", 0)             # (the switch is process-wide)
            eng.close()


# ------------------------------------------------------------------- the step's update: tail, row counts, short workgroups
STEP_PRIORS = [U.ISW_CASES[2], U.ISW_CASES[6]]          # n = 7: T = 18 isotropic with a goal, T = 24 full Q_c^-1 with a goal


def step_twice(case, P, dtype, wide):
    """Two sgpmp_step calls of a GP-cost problem with S = 8 from the same start: the first update writes the next step's
    importance-sampling weights (its tail) and -- fp32 -- the row counts; the second step (SGPMP_STEP_MEANS_KEPT) consumes
    those weights in its costs.  -> every tensor of both steps and the row counts after each."""
    from stoch_gpmp_amd import _lib as L
    from stoch_gpmp_amd.engine import Engine
    n, T, dt, ss, sg, sgoal = case
    S, d = 8, 2 * n
    eng = Engine(n, T, P, S, tensor_args=TA(dtype))
    try:
        eng.set_option("update_wide", wide)
        eng.set_prior(L.PRIOR_SAMPLE, dt, ss, sg, sgoal, Q_c_inv=U.isw_prior(case)[0])
        eng.set_costs([dict(kind=L.COST_GP, flags=0, sigma=1.0 if sg is None else sg, dt=dt)])
        means = U.isw_means(case, P, dtype).to(DEV)
        out = []
        for it in range(2):
            samples = torch.zeros(P, S, T, d, **TA(dtype))
            costs, weights = torch.zeros(P, S, **TA(dtype)), torch.zeros(P, S, **TA(dtype))
            grad, prev = torch.zeros(P, T, d, **TA(dtype)), torch.zeros(P, T, d, **TA(dtype))
            eng.step(17, 2 + it, means, samples, 3.0, 0.5, costs=costs, weights=weights, grad=grad, means_prev=prev,
                     flags=L.STEP_MEANS_KEPT if it else 0)
            torch.cuda.synchronize()
            out += [means.clone().cpu(), samples.cpu(), costs.cpu(), weights.cpu(), grad.cpu(), prev.cpu(),
                    torch.from_numpy(eng.row_counts().astype("int64"))]
        return out
    finally:
        eng.set_option("update_wide", 0)                 # (the switch is process-wide)
        eng.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", STEP_PRIORS, ids=[U.isw_case_id(c) for c in STEP_PRIORS])
@pytest.mark.parametrize("P", [1, 3, 4, 5, 130])
def test_step_with_tail_and_row_counts_is_the_same_with_either_update_kernel(P, case, dtype):
    """Short last workgroups (P = 1, 3, 5, 130: waves without a particle go to the tail's barrier, the tail stops at P),
    both tails (isotropic with Q^-1 in registers, full Q_c^-1 from memory) and both dtypes: everything two consecutive steps
    return, and the row counts, bit for bit."""
    new, old = step_twice(case, P, dtype, -1), step_twice(case, P, dtype, 1)
    assert len(new) == 14
    for i, (x, y) in enumerate(zip(new, old)):
        assert torch.equal(x, y), i
    assert bool(torch.isfinite(new[7]).all()) and not torch.equal(new[0], new[7])      # the second step moved the means
    assert float(new[9].abs().max()) > 0                                             # ... on costs that are not all zero


@pytest.mark.parametrize("nppg", [1, 3, 5, 130])
def test_small_panda_planner_is_the_same_run_with_either_update_kernel(nppg):
    """Panda fp32 through the fused launch, nppg particles x 16 samples x 16 waypoints, three optimize() calls of one iteration
    (each consumes the IS weights and the row counts the previous update left; the per-particle offsets into the row counts
    and the softmax partials at a short last workgroup), the kernels named by the device activity record."""
    sph = torch.as_tensor(SC.panda_spheres(num=5, seed=31)).to(**F32)

    def run(wide):
        pl = hip_panda_planner(dict(SC.PANDA), 16, nppg, 16, F32, seed=33, store_free=False)
        pl._engine.set_option("update_wide", wide)
        try:
            out, names = [], []
            for _ in range(3):
                ret = []
                names += update_kernels_launched(lambda: ret.extend(pl.optimize(opt_iters=1, obstacle_spheres=sph)))
                out += [t.clone() for t in ret] + [torch.from_numpy(pl._engine.row_counts().astype("int64"))]
            return out, names
        finally:
            pl._engine.set_option("update_wide", 0)

    (new, names_new), (old, names_old) = run(-1), run(1)
    assert len(names_new) == 3 and all("update_kernel_quad" in k for k in names_new), names_new
    assert len(names_old) == 3 and not any("update_kernel_quad" in k for k in names_old), names_old
    assert len(new) == 21
    for i, (x, y) in enumerate(zip(new, old)):
        assert same_bits(x, y), i
    assert int(new[6].max()) >= 1


# ----------------------------------------------------------------------------------------------- planner level, two chains
def panda_run(c, wide, iters=4, nppg=512):
    """optimize(opt_iters=iters) of Panda 512 x 64 x 16 (each half of the particles brings 16 384 rows: a two-chain step) from
    seed 31 -> (the six returned tensors, row counts, steps that ran as two chains, steps with the partials armed)."""
    sph = torch.as_tensor(SC.panda_spheres(num=5, seed=31)).to(**F32)
    pl = hip_panda_planner(c, 16, nppg, 64, F32, seed=31, store_free=False)
    pl._engine.set_option("update_wide", wide)
    try:
        ret = pl.optimize(opt_iters=iters, obstacle_spheres=sph)
        torch.cuda.synchronize()
        out = [t.clone() for t in ret]
        return out, pl._engine.row_counts().copy(), pl._engine.pipeline_split_steps(), pl._engine.dense_armed_steps()
    finally:
        pl._engine.set_option("update_wide", 0)


def assert_same_run(c, wide=-1, nppg=512):
    new, nnz_new, split_new, armed_new = panda_run(c, wide, nppg=nppg)
    old, nnz_old, split_old, armed_old = panda_run(c, 1, nppg=nppg)
    assert len(new) == 6 and len(old) == 6
    for i, (x, y) in enumerate(zip(new, old)):
        assert same_bits(x, y), i
    assert nnz_new.tolist() == nnz_old.tolist()
    assert split_new == 4 and split_old == 4
    assert armed_new == armed_old
    return nnz_new, armed_new


def test_two_chain_optimize_is_the_same_run_with_one_hot_weights():
    nnz, _ = assert_same_run(dict(SC.PANDA))
    assert int(nnz.max()) >= 1


def test_two_chain_optimize_under_the_default_rule_is_the_same_run():
    """The default rule takes update_kernel_quad for halves of 512 to 1023 particles: 1024 particles run it, 512 (halves of
    256) and 2048 (halves of 1024) keep update_kernel."""
    assert_same_run(dict(SC.PANDA), wide=0, nppg=1024)
    for nppg, quad in ((1024, True), (512, False), (2048, False)):
        names = update_kernels_launched(lambda: panda_run(dict(SC.PANDA), 0, iters=2, nppg=nppg))
        assert len(names) == 4 and all(("update_kernel_quad" in k) == quad for k in names), (nppg, names)


def test_two_chain_optimize_is_the_same_run_with_spread_weights():
    """A temperature (and a weak sampling prior: with the reference's stiff one the softmax is one-hot at any temperature) that
    spreads the weights: iterations 2-4 then add the fused launch's softmax partials (more rows with weight than S / 8)."""
    soft = dict(sigma_start_sample=1.0, sigma_goal_sample=1.0, sigma_gp_sample=30.0)
    sph = torch.as_tensor(SC.panda_spheres(num=5, seed=31)).to(**F32)
    found = None
    for temp in (1e11, 1e14, 1e17):
        c = dict(SC.PANDA, temperature=temp, **soft)
        pl = hip_panda_planner(c, 16, 512, 64, F32, seed=31, store_free=False)
        pl.optimize(opt_iters=1, obstacle_spheres=sph)
        if int((pl._engine.row_counts() > 8).sum()) >= 256:
            found = c
            break
    assert found is not None, "no temperature of the scan spreads the weights: the test needs another scenario"
    nnz, armed = assert_same_run(found)
    assert armed > 0 and int(nnz.max()) > 8, (armed, int(nnz.max()))
