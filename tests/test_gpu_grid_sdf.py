"""The signed-distance grid field (SGPMP_COST_GRID_SDF) on the GPU: the distance transform (csrc/sdf.hip), the term in
sgpmp_field_grad, the sweep, the step, sgpmp_dense_cost / sgpmp_dense_cost_grad and GPMP with and without continuous-time factors,
against the test-side oracle (tests/grid_sdf_oracle.py: brute force / scipy transform, torch fp64 field with autograd) and the
numpy twin (stoch_gpmp_amd/grid_sdf.py).  Needs the MI355X: run with `-m gpu`.

fp64 bounds: the host test's 1e-12 max(1, cap) for the field, 1e-12 relative for the sweep, tests/test_gpu_dense_grad.py's for the
dense cost, tests/test_gpu_gpmp_dense.py's for GPMP (d_theta 1e-7, costs 1e-9, means 1e-8).

fp32 bounds: four times the worst case measured against the fp64 oracle on the MI355X (rounding-order headroom), each below the
project's fp32 bound of 1e-4 relative.  Measured (profiles/r10/grid_sdf.txt): field value 4.8e-7 and gradient 3.6e-7 relative to
max(1, |ref|) at points >= 1e-2 cells off the kinks; sweep costs 4.8e-8 relative."""
import numpy as np
import pytest
import torch

from oracle import gpmp_equiv as GP
from stoch_gpmp_amd import grid_sdf
from tests import gpmp_dense_oracle as DO
from tests import grid_sdf_oracle as O
from tests.test_gpu_dense_cost import check, make_engine
from tests.test_gpu_dense_grad import check_grad, torch_limit_penalty
from tests.test_gpu_gpmp_dense import hip_gpmp, rel_err

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = [torch.float64, torch.float32]
FP32_FIELD_MEASURED = (4.8e-7, 3.6e-7)      # value, gradient: worst |got - oracle| / max(1, |oracle|) on the MI355X
FP32_SWEEP_MEASURED = 4.8e-8                # worst relative error of a cost
OCC, CELL, OFF = O.box_disc_map()


def TA(dtype):
    return {"device": DEV, "dtype": dtype}


_REF = {}


def ref_sdf():
    """The oracle's grid of the 20 x 24 map, computed once."""
    if "sdf" not in _REF:
        _REF["sdf"] = O.brute_sdf(OCC, CELL)
    return _REF["sdf"]


def make_field(dtype, margin=O.MARGIN, occ=OCC, cell=CELL):
    from stoch_gpmp_amd.envs.obst_map import ObstacleMap
    om = ObstacleMap.from_grid(occ, cell, tensor_args=TA(dtype))
    if occ is OCC:
        assert (float(om.origin_xi), float(om.origin_yi)) == OFF
    return om.distance_field(margin)


def build(occ, cell, dtype, threshold=0.):
    from stoch_gpmp_amd.engine import Engine
    eng = Engine(2, 2, 0, 1, tensor_args=TA(dtype))
    return eng.grid_sdf_build(torch.as_tensor(occ).to(**TA(dtype)).contiguous(), cell, threshold).cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. the transform
@pytest.mark.parametrize("dtype", DTYPES)
def test_build_kernel_equals_the_oracle_exactly(dtype):
    cases = [(name, occ, cell, O.brute_sdf) for name, (occ, cell) in O.small_maps().items()]
    cases.append(("3x261", *O.wide_map(), O.brute_sdf))
    cases.append(("300x260", *O.large_map(), O.scipy_sdf))
    np_t = np.float64 if dtype == torch.float64 else np.float32
    for name, occ, cell, oracle in cases:
        got, ref = build(occ, cell, dtype), oracle(occ, cell).astype(np_t)
        assert got.dtype == np_t and got.shape == occ.shape
        assert np.array_equal(got, ref), f"{name} {dtype}: {int((got != ref).sum())} of {got.size} cells differ"
    # the threshold, and a map the kernel must cap
    occ = np.array([[0., 0.5, 1.0, 0.5, 0.]])
    assert np.array_equal(build(occ, 2., dtype, threshold=0.5), O.brute_sdf(occ, 2., 0.5).astype(np_t))
    assert np.array_equal(build(occ, 2., dtype, threshold=1.0), np.full((1, 5), 12., dtype=np_t))


def test_build_refuses_bad_sizes_before_any_launch():
    from stoch_gpmp_amd import _lib
    from stoch_gpmp_amd.engine import Engine
    eng = Engine(2, 2, 0, 1, tensor_args=TA(torch.float64))
    buf = torch.full((8,), 7., **TA(torch.float64))
    out = torch.full((8,), -3., **TA(torch.float64))
    for ny, nx, cell in ((0, 4, 0.1), (4, 0, 0.1), (1, 4097, 0.1), (4097, 1, 0.1), (2, 4, 0.), (2, 4, float("nan"))):
        rc = eng.lib.sgpmp_grid_sdf_build(eng._ctx, _lib.ptr(buf), ny, nx, cell, 0., _lib.ptr(out), _lib.stream_ptr())
        assert rc == _lib.EINVAL and "sgpmp_grid_sdf_build" in _lib.last_error(), (ny, nx, cell)
    assert eng.lib.sgpmp_grid_sdf_build(eng._ctx, _lib.ptr(buf), 2, 4, 0.1, 0., _lib.ptr(buf), _lib.stream_ptr()) == _lib.EINVAL
    torch.cuda.synchronize()
    assert bool((out == -3.).all()) and bool((buf == 7.).all())           # nothing was written
    with pytest.raises(ValueError):
        eng.grid_sdf_build(torch.zeros(4, 4097, **TA(torch.float64)), 0.1)


# ------------------------------------------------------------------------------------------------ 2. sgpmp_field_grad
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_field_grad_matches_oracle_and_autograd(dtype, n):
    f64 = dtype == torch.float64
    sdf = ref_sdf()
    fld = make_field(dtype)
    assert np.array_equal(fld.sdf.cpu().numpy(), sdf.astype(np.float64 if f64 else np.float32))
    pool = O.draw_points(sdf, CELL, OFF, O.MARGIN, 130, seed=3, tol=1e-3 if f64 else 1e-2)
    if not f64:
        pool = pool.astype(np.float32).astype(np.float64)       # the oracle at the points the device is given
    cap = CELL * (sdf.shape[0] + sdf.shape[1])
    worst = [0., 0.]
    for B in (1, 63, 65, 130):
        pts = pool[:B]
        ho, do, go = O.field_and_grad(sdf, pts, CELL, OFF, O.MARGIN)
        if B >= 63:                                            # the conditions, on the oracle alone
            lo, hi = np.array([-OFF[0] * CELL, -OFF[1] * CELL]), np.array([(24 - OFF[0]) * CELL, (20 - OFF[1]) * CELL])
            assert (ho > 0).sum() * 3 >= B and (ho == 0).any() and ((pts < lo) | (pts > hi)).any()
        q = torch.zeros(B, n, dtype=torch.float64)
        q[:, :2] = torch.from_numpy(pts)
        if n == 3:
            q[:, 2] = torch.linspace(-1, 1, B, dtype=torch.float64)
        h, g = fld.compute_cost_and_grad(q.to(**TA(dtype)))
        h, g = h.double().cpu().numpy(), g.double().cpu().numpy()
        assert g.shape == (B, n)
        if n == 3:
            assert np.array_equal(g[:, 2], np.zeros(B))
        assert np.array_equal(g[ho == 0], np.zeros_like(g[ho == 0])) and np.array_equal(h[ho == 0], np.zeros_like(h[ho == 0]))
        if f64:
            tol = 1e-12 * max(1., cap)
            assert np.abs(h - ho).max() <= tol and np.abs(g[:, :2] - go).max() <= tol, (B, np.abs(h - ho).max(), np.abs(g[:, :2] - go).max())
        else:
            worst[0] = max(worst[0], float((np.abs(h - ho) / np.maximum(1., np.abs(ho))).max()))
            worst[1] = max(worst[1], float((np.abs(g[:, :2] - go) / np.maximum(1., np.abs(go))).max()))
    if not f64:
        print(f"    fp32 field against the fp64 oracle: value {worst[0]:.3e}, gradient {worst[1]:.3e} (relative to max(1, |ref|))")
        for w, m in zip(worst, FP32_FIELD_MEASURED):
            assert 4 * m < 1e-4 and w <= 4 * m, (worst, FP32_FIELD_MEASURED)


@pytest.mark.parametrize("dtype", DTYPES)
def test_field_object_methods_and_nan(dtype):
    sdf = ref_sdf()
    fld = make_field(dtype)
    pts = O.draw_points(sdf, CELL, OFF, O.MARGIN, 65, seed=8, tol=1e-2)
    ho, do, go = O.field_and_grad(sdf, pts, CELL, OFF, O.MARGIN)
    X = torch.from_numpy(pts).to(**TA(dtype)).reshape(5, 13, 2)
    # (the wiring of the methods, not the arithmetic: fp32 at 2^-23 x a dozen operations x values up to cap = 22)
    tol = 1e-11 if dtype == torch.float64 else 2e-5
    cost, dist, grad = fld.compute_cost(X), fld.compute_distance(X), fld.gradient(X)
    assert cost.shape == (5, 13) and dist.shape == (5, 13) and grad.shape == (5, 13, 2)
    assert np.abs(cost.double().cpu().numpy().ravel() - ho).max() <= tol
    assert np.abs(dist.double().cpu().numpy().ravel() - do).max() <= tol
    assert np.abs(grad.double().cpu().numpy().reshape(-1, 2) - go).max() <= tol
    assert torch.equal(fld(X), cost)
    # a non-finite point: NaN in the value and in both derivatives, its neighbours untouched
    bad = X.reshape(-1, 2).clone()
    bad[3, 0], bad[7, 1], bad[11, 0] = float("nan"), float("inf"), float("-inf")
    h, g = fld.compute_cost_and_grad(bad)
    rows = torch.tensor([3, 7, 11], device=DEV)
    keep = torch.ones(65, dtype=torch.bool, device=DEV)
    keep[rows] = False
    assert bool(torch.isnan(h[rows]).all()) and bool(torch.isnan(g[rows]).all())
    assert torch.equal(h[keep], cost.reshape(-1)[keep]) and torch.equal(g[keep], grad.reshape(-1, 2)[keep])
    assert bool(torch.isnan(fld.compute_distance(bad)[rows]).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_x_is_clamped_by_the_x_extent_on_a_non_square_map(dtype):
    """3 x 5 cells: far out in x the field reads column 4 (the occupancy lookup's clamp of x by the row count is not copied)."""
    from stoch_gpmp_amd.engine import Engine
    from stoch_gpmp_amd import _lib
    sdf = (np.arange(15.).reshape(3, 5) * 0.1 - 0.4)
    eng = Engine(2, 2, 0, 1, tensor_args=TA(dtype))
    t = torch.from_numpy(sdf).to(**TA(dtype)).contiguous()
    eng.set_costs([dict(kind=_lib.COST_GRID_SDF, flags=_lib.FLAG_GRID_DISTANCE, sigma=1., sigma2=0.7, device_tensor=t, dim0=3, dim1=5,
                        p0=0.5, p1=1., p2=2.)])
    pts = np.array([[100., 0.2], [-100., 0.2], [0.3, 100.], [0.3, -100.], [0.33, 0.21]])
    d, _ = eng.field_grad(0, torch.from_numpy(pts).to(**TA(dtype)).contiguous())
    _, want, _ = grid_sdf.field(sdf, pts, 0.5, (1., 2.), 0.7)
    assert np.abs(d.double().cpu().numpy() - want).max() <= (1e-12 if dtype == torch.float64 else 1e-6)
    assert float(d[0]) > float(d[1]) + 0.39


def test_get_linear_system_through_the_field_factor():
    from stoch_gpmp_amd.costs.cost_functions import CostCollision
    T, P = 5, 3
    ta = TA(torch.float64)
    c = O.GPMP_C
    fld = make_field(torch.float64)
    means = O.gpmp_means(T, P)
    A, b, K = CostCollision(2, T, field=fld, sigma_coll=c["sigma_coll"], tensor_args=ta).get_linear_system(means.to(**ta))
    Ao, bo, Ko = O.support_system(means, ref_sdf(), CELL, OFF, O.MARGIN, c["sigma_coll"])
    assert float(bo.abs().max()) > 0 and float(Ao.abs().max()) > 0
    assert rel_err(A, Ao) < 1e-12 and rel_err(b, bo) < 1e-12 and rel_err(K, Ko) < 1e-12


# ------------------------------------------------------------------------------------------------ 3. the sweep and the step
def planar_descs(T, rows, ta, field=None, S=1):
    from stoch_gpmp_amd.costs.cost_functions import CostGP, CostGoalPrior
    c = O.GPMP_C
    start, goals = torch.tensor(c["start"], **ta), torch.tensor([c["goal"]], **ta)
    d = CostGP(2, T, start, c["dt"], dict(sigma_start=c["cost_sigma_start"], sigma_gp=c["cost_sigma_gp"]), ta).descriptors()
    d += CostGoalPrior(2, T, multi_goal_states=goals, num_particles_per_goal=rows, num_samples=S,
                       sigma_goal_prior=c["sigma_goal_prior"], tensor_args=ta).descriptors()
    return d + ([field.descriptor(c["sigma_coll"])] if field is not None else [])


@pytest.mark.parametrize("dtype", DTYPES)
def test_sweep_adds_k_times_the_sum_of_the_hinge(dtype):
    f64 = dtype == torch.float64
    ta = TA(dtype)
    fld = make_field(dtype)
    K = 1. / O.GPMP_C["sigma_coll"] ** 2
    sdf = ref_sdf()
    worst = 0.
    for T in (2, 3, 17):
        for B in (1, 9, 130):
            x = O.gpmp_means(T, B, seed=T * 1000 + B, noise=0.4).to(dtype)
            xd = x.to(DEV).contiguous()
            with_f = make_engine(2, T, dtype, costs=planar_descs(T, B, ta, fld))
            without = make_engine(2, T, dtype, costs=planar_descs(T, B, ta))
            c1 = with_f.cost_eval(xd, out64=torch.empty(B, device=DEV, dtype=torch.float64)).cpu().numpy()
            c0 = without.cost_eval(xd, out64=torch.empty(B, device=DEV, dtype=torch.float64)).cpu().numpy()
            assert "cost_sweep_kernel" in with_f.last_cost_kernel()
            h, _, _ = grid_sdf.field(sdf, x.double().numpy()[:, 1:, :2], CELL, OFF, O.MARGIN)
            ref = c0 + K * h.sum(1)
            assert float((K * h.sum(1)).min()) > 0                     # the term is there, in every trajectory
            err = float((np.abs(c1 - ref) / np.abs(ref)).max())
            worst = max(worst, err)
            if f64:
                assert err <= 1e-12, (T, B, err)
    if not f64:
        print(f"    fp32 sweep with the term against fp64 twin: worst relative error {worst:.3e}")
        assert 4 * FP32_SWEEP_MEASURED < 1e-4 and worst <= 4 * FP32_SWEEP_MEASURED, worst


def planar_planner(dtype, field, T=16, nppg=2, S=8, seed=31, **kw):
    from stoch_gpmp_amd.workloads import hip_planar_planner
    c = dict(O.GPMP_C, step_size=0.5, temperature=1.)
    return hip_planar_planner(c, T, [c["goal"]], nppg, S, field, TA(dtype), seed=seed, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
def test_step_with_the_term_is_sampler_sweep_update_bit_for_bit(dtype):
    from stoch_gpmp_amd import _lib as L
    from stoch_gpmp_amd.envs.obst_map import ObstacleMap
    fld = make_field(dtype)
    p, q = planar_planner(dtype, fld), planar_planner(dtype, fld)
    assert torch.equal(p.particle_means, q.particle_means)
    costs, grad = p.step()
    assert "fused" not in p._engine.last_cost_kernel() and p._engine.last_cost_kernel().startswith("cost_sweep_kernel")
    eng, S, P = q._engine, q.num_samples, q.num_particles_local
    means = q.particle_means
    smp = eng.sample(L.PRIOR_SAMPLE, q.seed, q._draw, means, S, mode_offset=q.p0)
    isw = eng.is_weights(means, q.temperature)
    c, c64 = torch.empty(P, S, **TA(dtype)), torch.empty(P, S, device=DEV, dtype=torch.float64)
    eng.cost_eval(smp, is_weights=isw, rows_per_particle=S, out=c, out64=c64)
    w, g, mp = torch.empty(P, S, **TA(dtype)), torch.empty_like(means), torch.empty_like(means)
    eng.update(c64, smp, means, q.temperature, q.step_size, weights=w, grad=g, means_prev=mp)
    assert torch.equal(p.state_samples, smp) and torch.equal(costs, c)
    assert torch.equal(p._weights_buf, w) and torch.equal(grad, g) and torch.equal(p.particle_means, means)
    # the term is in those costs: the same samples through a program without it (no importance-sampling term in either) give less
    bare = make_engine(2, 16, dtype, costs=planar_descs(16, P, TA(dtype), S=S))
    c1 = eng.cost_eval(smp, out64=torch.empty(P * S, device=DEV, dtype=torch.float64))
    c0 = bare.cost_eval(smp, out64=torch.empty(P * S, device=DEV, dtype=torch.float64))
    assert float((c1 - c0).min()) > 0
    # the same planner on the occupancy map keeps the fused planar launch it has today
    occ_pl = planar_planner(dtype, ObstacleMap.from_grid(OCC, CELL, tensor_args=TA(dtype)))
    ref_pl = planar_planner(dtype, ObstacleMap.from_grid(OCC, CELL, tensor_args=TA(dtype)))
    ref_pl._engine.set_option("no_fused_step", 1)
    occ_pl.step()
    ref_pl.step()
    assert occ_pl._engine.last_cost_kernel().startswith("fused_step_f64" if dtype == torch.float64 else "fused_planar")
    assert ref_pl._engine.last_cost_kernel().startswith("cost_sweep_kernel")


def test_update_rebuilds_on_the_device_and_planners_recompile():
    from stoch_gpmp_amd.envs.obst_map import ObstacleMap
    dtype = torch.float64
    om = ObstacleMap.from_grid(OCC, CELL, tensor_args=TA(dtype))
    fld = om.distance_field(O.MARGIN)
    a = planar_planner(dtype, fld, seed=7)
    a.step()
    v0, ptr0 = fld._version, fld.sdf.data_ptr()
    occ2 = OCC.copy()
    occ2[7:13, 10:15] = 0.                                    # the box goes, a wall appears
    occ2[2:18, 16:18] = 1.
    om.map = occ2
    om.convert_map()
    assert fld.update() is fld.sdf and fld._version == v0 + 1 and fld.sdf.data_ptr() == ptr0
    assert np.array_equal(fld.sdf.cpu().numpy(), O.brute_sdf(occ2, CELL))
    fresh = ObstacleMap.from_grid(occ2, CELL, tensor_args=TA(dtype)).distance_field(O.MARGIN)
    assert torch.equal(fresh.sdf, fld.sdf)
    # a's next step sees the new map: its costs are those of a planner built on the new map at the same means and draw ...
    prev, draw = a.particle_means.clone(), a._draw
    ca = a.step()[0].clone()
    d = planar_planner(dtype, fresh, seed=7)
    d.particle_means.copy_(prev)
    d._draw = draw
    assert torch.equal(ca, d.step()[0])
    # ... and not those of the old map
    e = planar_planner(dtype, make_field(dtype), seed=7)
    e.particle_means.copy_(prev)
    e._draw = draw
    assert not torch.equal(ca, e.step()[0])
    # a map of ANOTHER SHAPE (six more rows, the box back): update() has to hand out a new tensor, so only a planner that
    # re-compiled its cost program (the version moved) can see it -- a stale program would go on reading the old 20 x 24 grid
    occ3 = np.zeros((26, 24))
    occ3[:20] = occ2
    occ3[7:13, 10:15] = 1.
    occ3[21:25, 3:9] = 1.
    om.map = occ3
    om.convert_map()
    old_sdf, v1 = fld.sdf, fld._version
    assert fld.update() is fld.sdf and fld.sdf is not old_sdf and tuple(fld.sdf.shape) == (26, 24) and fld._version == v1 + 1
    assert np.array_equal(fld.sdf.cpu().numpy(), O.brute_sdf(occ3, CELL))
    assert np.array_equal(old_sdf.cpu().numpy(), O.brute_sdf(occ2, CELL))              # (the old grid is what a stale program would read)
    om3 = ObstacleMap.from_grid(OCC, CELL, tensor_args=TA(dtype))                       # the same offsets, the new cells
    om3.map = occ3.copy()
    om3.convert_map()
    prev, draw = a.particle_means.clone(), a._draw
    ca = a.step()[0].clone()
    for field, same in ((om3.distance_field(O.MARGIN), True), (fresh, False)):
        f = planar_planner(dtype, field, seed=7)
        f.particle_means.copy_(prev)
        f._draw = draw
        assert torch.equal(ca, f.step()[0]) == same
    # the field's own query engines follow: rebuilt in place they are kept, after a reallocation they are made anew
    X = torch.tensor([[0.3, 5.5], [1.0, -1.0]], **TA(dtype))
    assert torch.equal(fld.compute_cost(X), om3.distance_field(O.MARGIN).compute_cost(X))


# ------------------------------------------------------------------------------------------------ 4. dense cost and gradient
LIMITS = (([-0.5, -1.5], [3.0, 0.5]), [25., 20.], 0.5)        # q_limits, v_limits, sigma_limit: each binds somewhere


def dense_inputs(T, B, dtype, n_sub, tol):
    """B noisy lines through the box none of whose fine states, on the oracle, lies within `tol` cells of a kink: the first B
    such trajectories of a seeded pool (with n_sub = 31 about one candidate in two hundred qualifies at tol = 1e-2)."""
    key = (T, B, dtype, n_sub, tol)
    if key not in _REF:
        pool = O.gpmp_means(T, 8192, seed=100 + T + n_sub, noise=0.3).to(dtype)
        fine = DO.hermite_fine(pool.double(), n_sub, O.GPMP_C["dt"])
        line, lev = O.kink_distance(ref_sdf(), fine[:, 1:, :2].numpy(), CELL, OFF, O.MARGIN)
        good = np.nonzero((line.min(1) >= tol) & (lev.min(1) >= tol))[0]
        assert len(good) >= B, f"only {len(good)} of 8192 candidates keep their fine states off the kinks"
        _REF[key] = pool[torch.from_numpy(good[:B])].contiguous()
    return _REF[key]


def dense_oracle(x, T, n_sub, weight, sigma, limits, support):
    """(J [B], scale [B], dJ/dx [B,T,4]) in fp64: the oracle's Hermite interpolation + field + limit penalty, autograd through all."""
    xs = x.double().clone().requires_grad_(True)
    fine = DO.hermite_fine(xs, n_sub, O.GPMP_C["dt"])
    f = np.arange(fine.shape[1])
    sel = f % (n_sub + 1) != 0
    if support:
        sel |= (f % (n_sub + 1) == 0) & (f > 0)
    total = torch.zeros(x.shape[0], dtype=torch.float64)
    if sel.any() and weight > 0:
        h, _ = O.field_torch(ref_sdf(), fine[:, torch.from_numpy(f[sel]), :2], CELL, OFF, O.MARGIN)
        total = total + weight / sigma ** 2 * h.sum(1)
    if limits is not None:
        total = total + torch_limit_penalty(fine, *limits)
    g, = torch.autograd.grad(total.sum(), xs, allow_unused=True)
    return total.detach(), total.detach().abs(), torch.zeros_like(xs) if g is None else g


@pytest.mark.parametrize("support", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_cost_and_gradient_match_autograd_through_the_oracle(dtype, support):
    ta = TA(dtype)
    fld = make_field(dtype)
    sigma, weight, dt = 0.3, 0.7, O.GPMP_C["dt"]
    active = 0
    for T in (2, 5):
        eng = make_engine(2, T, dtype, costs=planar_descs(T, 1, ta)[:1] + [fld.descriptor(sigma)])
        for n_sub in (1, 4, 31):
            for B in (1, 5):
                x = dense_inputs(T, B, dtype, n_sub, 1e-3 if dtype == torch.float64 else 1e-2)
                xd = x.to(DEV).contiguous()
                what = f"T={T} n_sub={n_sub} B={B} support={int(support)}"
                ref, scale, gref = dense_oracle(x, T, n_sub, weight, sigma, LIMITS, support)
                ref_ins, _, _ = dense_oracle(x, T, n_sub, weight, sigma, LIMITS, False)
                active += int((gref.abs().sum((1, 2)) > 0).sum())
                value, grad = eng.dense_cost_grad(xd, n_sub, dt, weight=weight, q_limits=LIMITS[0], v_limits=LIMITS[1],
                                                  sigma_limit=LIMITS[2], support=support)
                assert "grid distance" in eng.last_dense_kernel()
                check(value, ref, scale, dtype, what + " value")
                check_grad(grad, gref, dtype, what)
                v2, g2 = eng.dense_cost_grad(xd, n_sub, dt, weight=weight, q_limits=LIMITS[0], v_limits=LIMITS[1],
                                             sigma_limit=LIMITS[2], support=support)
                assert torch.equal(v2, value) and torch.equal(g2, grad)                   # two calls, the same bits
                # sgpmp_dense_cost: the inserted states only, the no-FK kernel
                dc = eng.dense_cost(xd, n_sub, dt, weight=weight, q_limits=LIMITS[0], v_limits=LIMITS[1], sigma_limit=LIMITS[2],
                                    out64=torch.empty(B, device=DEV, dtype=torch.float64))
                assert "no FK" in eng.last_dense_kernel()
                check(dc, ref_ins, ref_ins.abs(), dtype, what + " sgpmp_dense_cost")
    assert active > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_gradient_accumulates_refuses_the_occupancy_grid_and_keeps_a_nan_to_its_trajectory(dtype):
    from stoch_gpmp_amd.envs.obst_map import ObstacleMap
    ta = TA(dtype)
    T, n_sub, B, dt = 5, 4, 5, O.GPMP_C["dt"]
    fld = make_field(dtype)
    eng = make_engine(2, T, dtype, costs=[fld.descriptor(0.3)])
    xd = dense_inputs(T, B, dtype, n_sub, 1e-2).to(DEV).contiguous()
    value, grad = eng.dense_cost_grad(xd, n_sub, dt, support=True)
    assert float(grad.abs().max()) > 0
    g0 = torch.randn(B, T, 4, generator=torch.Generator().manual_seed(2), dtype=torch.float64).to(**ta)
    acc = g0.clone()
    v2, g2 = eng.dense_cost_grad(xd, n_sub, dt, support=True, accumulate=True, grad=acc)
    assert torch.equal(v2, value) and torch.equal(g2, g0 + grad)
    # a NaN waypoint poisons its own trajectory only
    bad = xd.clone()
    bad[2, 3, 0] = float("nan")
    vb, gb = eng.dense_cost_grad(bad, n_sub, dt, support=True)
    keep = [0, 1, 3, 4]
    assert bool(torch.isnan(vb[2])) and bool(torch.isnan(gb[2]).all())
    assert torch.equal(vb[keep], value[keep]) and torch.equal(gb[keep], grad[keep])
    cb = eng.dense_cost(bad, n_sub, dt, out64=torch.empty(B, device=DEV, dtype=torch.float64))
    assert bool(torch.isnan(cb[2])) and bool(torch.isfinite(cb[keep]).all())
    # an occupancy GRID term with weight > 0 is still refused, also next to the new term
    om = ObstacleMap.from_grid(OCC, CELL, tensor_args=ta)
    both = make_engine(2, T, dtype, costs=[om.descriptor(0.5), fld.descriptor(0.3)])
    with pytest.raises(ValueError, match="grid lookup is piecewise constant"):
        both.dense_cost_grad(xd, n_sub, dt, weight=1.)
    both.dense_cost_grad(xd, n_sub, dt, weight=0., q_limits=LIMITS[0], sigma_limit=0.5)      # (the limit part alone is allowed)


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_cost_counts_the_term_next_to_link_fields(dtype, generic):
    """The generated-chain and the generic code path of dense_cost_kernel: a Panda program with the term appended (the planar point
    is (q[0], q[1])) gives the program without it + weight K sum of the hinge over the inserted states; the gradient call refuses
    the mixture."""
    from oracle.fk import PANDA_CHAIN
    from tests.test_gpu_dense_cost import DT, arm_inputs, panda_terms, spheres
    T, n_sub, weight, sigma = 6, 3, 0.7, 0.3
    fld = make_field(dtype)
    _, desc = panda_terms()
    with_f = make_engine(7, T, dtype, chain=PANDA_CHAIN, costs=desc + [fld.descriptor(sigma)], generic=generic)
    without = make_engine(7, T, dtype, chain=PANDA_CHAIN, costs=desc, generic=generic)
    xd, sph = arm_inputs(T, dtype).to(DEV), spheres().to(**TA(dtype))
    B = xd.shape[0]
    c1 = with_f.dense_cost(xd, n_sub, DT, spheres=sph, weight=weight, out64=torch.empty(B, device=DEV, dtype=torch.float64))
    assert ("generic FK" if generic else "generated chain") in with_f.last_dense_kernel()
    c0 = without.dense_cost(xd, n_sub, DT, spheres=sph, weight=weight, out64=torch.empty(B, device=DEV, dtype=torch.float64))
    fine = with_f.interpolate(xd, n_sub, DT).double().cpu().numpy()          # the device's own fine states
    ins = np.arange(fine.shape[1]) % (n_sub + 1) != 0
    h, _, _ = grid_sdf.field(ref_sdf(), fine[:, ins, :2], CELL, OFF, O.MARGIN)
    add = weight / sigma ** 2 * h.sum(1)
    assert float(add.min()) > 0
    check(c1, c0.cpu().numpy() + add, np.abs(c0.cpu().numpy()) + add, dtype, f"generic={generic}: the term next to link fields")
    with pytest.raises(ValueError, match="together with link-field terms"):
        with_f.dense_cost_grad(xd, n_sub, DT, spheres=sph, weight=weight)


def test_continuous_cost_differentiates_on_a_planar_cost_list():
    dtype = torch.float64
    fld = make_field(dtype)
    pl = planar_planner(dtype, fld, T=5, nppg=3, S=8)
    x = dense_inputs(5, 3, dtype, 4, 1e-3).to(DEV).requires_grad_(True)
    J = pl.continuous_cost(x, n_sub=4, weight=0.7, q_limits=LIMITS[0], v_limits=LIMITS[1], sigma_limit=LIMITS[2], support=True)
    g, = torch.autograd.grad(J.sum(), x)
    ref, scale, gref = dense_oracle(x.detach().cpu(), 5, 4, 0.7, O.GPMP_C["sigma_coll"], LIMITS, True)
    check(J.detach(), ref, scale, dtype, "continuous_cost value")
    check_grad(g, gref, dtype, "continuous_cost gradient")


# ------------------------------------------------------------------------------------------------ 5. GPMP
MODES = [("lm", 5.0, False), ("tr", 1e-2, True)]


def gpmp_planner(means, dtype, delta, trust, n_sub, field, limits=None, c=None):
    from stoch_gpmp_amd.costs.cost_functions import CostCollision, CostComposite, CostGP, CostGoalPrior
    c = dict(O.GPMP_C if c is None else c)
    ta = TA(dtype)
    P, T, _ = means.shape
    start, goals = torch.tensor(c["start"], **ta), torch.tensor([c["goal"]], **ta)
    cost = CostComposite(2, T, [
        CostGP(2, T, start, c["dt"], dict(sigma_start=c["cost_sigma_start"], sigma_gp=c["cost_sigma_gp"]), ta),
        CostGoalPrior(2, T, multi_goal_states=goals, num_particles_per_goal=P, num_samples=1, sigma_goal_prior=c["sigma_goal_prior"],
                      tensor_args=ta),
        CostCollision(2, T, field=field, sigma_coll=c["sigma_coll"], tensor_args=ta)], tensor_args=ta)
    dense = None
    if n_sub > 0 or limits is not None:
        dense = dict(n_sub=n_sub, weight=1.0 if n_sub > 0 else 0.)
        if limits is not None:
            dense.update(q_limits=(limits["q_lo"], limits["q_hi"]), v_limits=limits["v_max"], sigma_limit=limits["sigma_limit"])
    return hip_gpmp(means, goals, P, ta, delta, trust, dense_cost=dense, cost=cost, c=c, start=start)


def gpmp_limits(means):
    q, v = means[..., :2].reshape(-1, 2), means[..., 2:].reshape(-1, 2).abs()
    # (sigma_limit 0.5: the limit rows stay in the system -- they move the oracle's step by 1 - 17 % -- without drowning the field
    # rows, which with them move it by >= 0.19 at every tested shape; at 0.05 the field's share at T = 2 fell below the 0.05 bar)
    return dict(q_lo=torch.quantile(q, 0.2, dim=0), q_hi=torch.quantile(q, 0.8, dim=0), v_max=torch.quantile(v, 0.6, dim=0),
                sigma_limit=0.5)


@pytest.mark.parametrize("tag,delta,trust", MODES)
@pytest.mark.parametrize("n_sub", [0, 2, 31])
@pytest.mark.parametrize("T,P", [(2, 1), (3, 5), (16, 4)])
def test_gpmp_matches_the_oracle(T, P, n_sub, tag, delta, trust):
    """Two iterations against OracleGPMP with GP + goal prior + the field's rows (with dense_cost: + inserted and limit rows)."""
    sdf = ref_sdf()
    means = O.gpmp_means(T, P)
    limits = gpmp_limits(means) if n_sub > 0 else None
    ora = GP.OracleGPMP(means, O.gpmp_systems_fn(sdf, CELL, OFF, O.MARGIN, n_sub, limits=limits), 0.5, delta, trust, "inverse")
    ora0 = GP.OracleGPMP(means, O.gpmp_systems_fn(sdf, CELL, OFF, O.MARGIN, n_sub, field=False, limits=limits), 0.5, delta, trust,
                         "inverse")
    pl = gpmp_planner(means, torch.float64, delta, trust, n_sub, make_field(torch.float64), limits)
    d0, _ = ora0.step()
    for it in range(2):
        d_o, c_o = ora.step()
        if it == 0:
            moved = DO.rel_l2(d0, d_o)
            print(f"    T={T} P={P} n_sub={n_sub} {tag}: the field rows move d_theta by {moved:.3f} (relative L2)")
            assert moved >= 0.05, moved
        _, _, costs = pl.optimize()
        assert pl._engine.last_gpmp_kernel() == ("gpmp_thomas_kernel" if n_sub == 0 else "gpmp_dense_solve_kernel")
        e = (rel_err(pl._d_theta, d_o), rel_err(costs, c_o), rel_err(pl.particle_means, ora.particle_means))
        print(f"      iteration {it}: d_theta {e[0]:.2e} costs {e[1]:.2e} means {e[2]:.2e}")
        assert e[0] < 1e-7 and e[1] < 1e-9 and e[2] < 1e-8, (it, e)


@pytest.mark.parametrize("n_sub", [0, 3])
def test_gpmp_trust_region_diag_sum_matches_oracle(n_sub):
    T, P = 16, 4
    means = O.gpmp_means(T, P)
    limits = gpmp_limits(means) if n_sub > 0 else None
    fn = O.gpmp_systems_fn(ref_sdf(), CELL, OFF, O.MARGIN, n_sub, limits=limits)
    want = DO.field_dense_diag(fn(means))
    pl = gpmp_planner(means, torch.float64, 1e-2, True, n_sub, make_field(torch.float64), limits)
    diag = torch.zeros(T * 4, device=DEV, dtype=torch.float64)
    pl._engine.gpmp_linearize(pl.particle_means, diag_sum=diag)
    assert float(want.abs().max()) > 0
    assert rel_err(diag, want) < 1e-9


def test_gpmp_fp32_one_iteration_and_the_occupancy_grid_is_still_refused():
    from stoch_gpmp_amd import _lib
    from stoch_gpmp_amd.envs.obst_map import ObstacleMap
    T, P, n_sub = 16, 4, 2
    means = O.gpmp_means(T, P)
    limits = gpmp_limits(means)
    for k in (0, n_sub):
        lim = limits if k else None
        ora = GP.OracleGPMP(means, O.gpmp_systems_fn(ref_sdf(), CELL, OFF, O.MARGIN, k, limits=lim), 0.5, 5.0, False, "inverse")
        d_o, c_o = ora.step()
        pl = gpmp_planner(means, torch.float32, 5.0, False, k, make_field(torch.float32), lim)
        _, _, costs = pl.optimize()
        e = (rel_err(costs, c_o), rel_err(pl.particle_means, ora.particle_means))
        print(f"    fp32 GPMP n_sub={k}: costs {e[0]:.3e} means {e[1]:.3e} (relative, against the fp64 oracle)")
        assert e[0] < 1e-4 and e[1] < 1e-4, e
    occ = gpmp_planner(means, torch.float64, 5.0, False, 0, ObstacleMap.from_grid(OCC, CELL, tensor_args=TA(torch.float64)))
    before = occ.particle_means.clone()
    with pytest.raises((ValueError, _lib.SgpmpError), match=r"cost term without a linear system \(occupancy grid\)"):
        occ.optimize()
    assert torch.equal(occ.particle_means, before)


def test_the_distance_flag_is_a_query_and_no_cost():
    """SGPMP_FLAG_GRID_DISTANCE turns sgpmp_field_grad's answer into d and dd/dq: refused next to other terms and by GPMP."""
    from stoch_gpmp_amd import _lib
    from stoch_gpmp_amd.engine import Engine
    ta = TA(torch.float64)
    fld = make_field(torch.float64)
    flagged = dict(fld.descriptor(0.1), flags=_lib.FLAG_GRID_DISTANCE)
    eng = Engine(2, 4, 1, 1, tensor_args=ta)
    with pytest.raises(ValueError, match="query flag"):
        eng.set_costs(planar_descs(4, 1, ta) + [flagged])
    with pytest.raises(ValueError, match="query flag"):
        eng.set_costs([flagged, fld.descriptor(0.1)])
    eng.set_costs([flagged])                                                # alone: the query GridDistanceField.compute_distance makes
    with pytest.raises(ValueError, match="a query, not a cost"):
        eng.gpmp_linearize(O.gpmp_means(4, 1).to(**ta))


# ------------------------------------------------------------------------------------------------ 6. end to end
# Chosen with the oracle on the CPU (its own 30 iterations end with every fine state in a free cell, from 34 occupied ones): margin
# 1.0 (two cells), sigma_coll 0.05, Levenberg-Marquardt delta 1.0, step size 0.5 (hip_gpmp's), the line's y off the box's centre
# line -- through the centre the two sides' forces balance and Gauss-Newton stays inside the box.
E2E = dict(O.GPMP_C, start=[-1.5, 0.0, 0., 0.], goal=[4.0, 0.2, 0., 0.], sigma_coll=0.05)
E2E_MARGIN, E2E_DELTA, E2E_T, E2E_NSUB = 1.0, 1.0, 16, 4


def test_gpmp_plans_around_the_box_end_to_end():
    from stoch_gpmp_amd.envs.obst_map import ObstacleMap
    dtype, T, k = torch.float64, E2E_T, E2E_NSUB
    st, go = torch.tensor(E2E["start"], dtype=dtype), torch.tensor(E2E["goal"], dtype=dtype)
    w = torch.linspace(0, 1, T, dtype=dtype).reshape(1, T, 1)
    means = torch.zeros(1, T, 4, dtype=dtype)
    means[..., :2] = st[:2] + (go[:2] - st[:2]) * w
    means[..., 2:] = (go[:2] - st[:2]) / ((T - 1) * E2E["dt"])
    om = ObstacleMap.from_grid(OCC, CELL, tensor_args=TA(dtype))

    def occupied(m):
        fine = DO.hermite_fine(m.double().cpu(), k, E2E["dt"])
        return om.get_collisions(fine[..., :2].to(**TA(dtype)).contiguous())
    assert int((occupied(means) > 0).sum()) >= 10                # the straight line crosses the box
    ora = GP.OracleGPMP(means, O.gpmp_systems_fn(ref_sdf(), CELL, OFF, E2E_MARGIN, k, c=E2E), 0.5, E2E_DELTA, False, "inverse")
    for _ in range(30):
        ora.step()
    assert int((occupied(ora.particle_means) > 0).sum()) == 0    # the oracle's own 30 iterations get there
    pl = gpmp_planner(means, dtype, E2E_DELTA, False, k, om.distance_field(E2E_MARGIN), c=E2E)
    pl.optimize(opt_iters=30)
    assert pl._engine.last_gpmp_kernel() == "gpmp_dense_solve_kernel"
    assert int((occupied(pl.particle_means) > 0).sum()) == 0
    fine_dev = pl.interpolate_trajectories(n_sub=k)
    assert bool((om.get_collisions(fine_dev[..., :2].contiguous()) == 0).all())
