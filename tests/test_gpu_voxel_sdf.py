"""The voxel signed-distance field (SGPMP_COST_VOXEL_SDF) on the GPU: the distance transform (csrc/sdf.hip), the term in
sgpmp_field_grad, sgpmp_field_eval, the generic sweep on its three FK flavours, the step, and GPMP with and without
continuous-time factors, against the test-side oracle (tests/voxel_sdf_oracle.py: brute force / scipy transform, torch fp64 field
with autograd through oracle/fk.py).  Needs the MI355X: run with `-m gpu`.

fp64 bounds: 1e-12 max(1, cap) on field values (tests/test_gpu_grid_sdf.py's), the same times the chain's reach on gradients,
1e-12 relative for the sweep, tests/test_gpu_gpmp_dense.py's for GPMP (d_theta 1e-7, costs 1e-9, means 1e-8).
fp32 bounds: those of the existing fp32 field tests in tests/test_gpu_kernels.py -- 3e-4 relative plus 3e-4 of the largest
reference value for the field and its Jacobian, 2e-4 for the sweep.  The errors measured on the MI355X stay far below them, so
the existing bounds hold unchanged (profiles/r11/voxel_sdf.txt): over five seeds the field value is off by at most 3.2e-7 and the
gradient by 4.7e-7 of the largest reference value; a sweep cost by 1.2e-6 relative (generated chain), 5.6e-7 (generic FK)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import gpmp_equiv as GP
from tests import gpmp_dense_oracle as DO
from tests import voxel_sdf_oracle as O
from tests.test_gpu_gpmp_dense import hip_gpmp, rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
DTYPES = [torch.float64, torch.float32]
SEED = 4                            # tests/test_cpu_voxel_sdf.py holds this seed's configurations to the conditions, on the oracle
FP32_RTOL = 3e-4                    # tests/test_gpu_kernels.py::test_field_jacobian_matches_autograd_through_fk
FP32_SWEEP_RTOL = 2e-4              # tests/test_gpu_kernels.py::test_register_fk_path_equals_generic_lds_path_and_oracle
SOLVE = "cholesky"                  # OracleGPMP's solve of the SPD system A^T K A + delta I (residual 3e-15 at the tested shapes)


def TA(dtype):
    return {"device": DEV, "dtype": dtype}


def NP(dtype):
    return np.float64 if dtype == torch.float64 else np.float32


_REF = {}


def scene():
    """The arm scene with the oracle's distance volume, computed once."""
    if "scene" not in _REF:
        _REF["scene"] = O.arm_scene()
    return _REF["scene"]


def device_chain(which):
    from stoch_gpmp_amd.robots.panda_chain import PANDA_CHAIN
    return PANDA_CHAIN if which == "panda" else O.TOY_CHAIN


def make_field(dtype, ni=0, rng=(5, 7), margin=O.MARGIN, sc=None):
    from stoch_gpmp_amd.envs.voxel_map import VoxelMap
    sc = scene() if sc is None else sc
    vm = VoxelMap.from_grid(sc["occ"], sc["cell"], sc["lower"], tensor_args=TA(dtype))
    assert np.allclose(vm.origin, sc["origin"], rtol=0, atol=0)
    return vm.distance_field(margin, num_interpolate=ni, link_interpolate_range=list(rng))


def build(occ, cell, dtype, threshold=0.):
    from stoch_gpmp_amd.engine import Engine
    eng = Engine(1, 2, 0, 1, tensor_args=TA(dtype))
    return eng.voxel_sdf_build(torch.as_tensor(occ).to(**TA(dtype)).contiguous(), cell, threshold).cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. the transform
@pytest.mark.parametrize("dtype", DTYPES)
def test_build_kernel_equals_the_oracle_exactly(dtype):
    cases = {**O.small_volumes(), **O.mapping_volumes(), "arm scene": (scene()["occ"], scene()["cell"])}
    for name, (occ, cell) in cases.items():
        got, ref = build(occ, cell, dtype), O.brute_sdf_cached(occ, cell).astype(NP(dtype))
        assert got.dtype == NP(dtype) and got.shape == occ.shape
        assert np.array_equal(got, ref), f"{name} {dtype}: {int((got != ref).sum())} of {got.size} cells differ"
    # the threshold, and a volume the kernel must cap
    occ = np.array([0., 0.5, 1.0, 0.5, 0.]).reshape(1, 1, 5)
    assert np.array_equal(build(occ, 2., dtype, threshold=0.5), O.brute_sdf(occ, 2., 0.5).astype(NP(dtype)))
    assert np.array_equal(build(occ, 2., dtype, threshold=1.0), np.full((1, 1, 5), 14., dtype=NP(dtype)))
    assert np.array_equal(build(occ, 2., dtype, threshold=-1.0), np.full((1, 1, 5), -14., dtype=NP(dtype)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_build_kernel_equals_scipy_on_a_large_volume(dtype):
    pytest.importorskip("scipy.ndimage")
    occ, cell = O.large_volume()
    got, ref = build(occ, cell, dtype), O.scipy_sdf(occ, cell).astype(NP(dtype))
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} of {got.size} cells differ"


def test_build_refuses_bad_sizes_before_any_launch():
    from stoch_gpmp_amd import _lib
    from stoch_gpmp_amd.engine import Engine
    eng = Engine(1, 2, 0, 1, tensor_args=TA(torch.float64))
    buf = torch.full((8,), 7., **TA(torch.float64))
    out = torch.full((8,), -3., **TA(torch.float64))
    call = lambda nz, ny, nx, cell, thr, o, s: eng.lib.sgpmp_voxel_sdf_build(eng._ctx, _lib.ptr(o), nz, ny, nx, cell, thr,   # noqa: E731
                                                                               _lib.ptr(s), _lib.stream_ptr())
    for nz, ny, nx, cell, thr in ((0, 2, 4, 0.1, 0.), (2, 0, 4, 0.1, 0.), (2, 4, 0, 0.1, 0.), (513, 1, 1, 0.1, 0.), (1, 513, 1, 0.1, 0.),
                                  (1, 1, 513, 0.1, 0.), (1, 2, 4, 0., 0.), (1, 2, 4, -0.1, 0.), (1, 2, 4, float("nan"), 0.),
                                  (1, 2, 4, 0.1, float("nan"))):
        assert call(nz, ny, nx, cell, thr, buf, out) == _lib.EINVAL and "sgpmp_voxel_sdf_build" in _lib.last_error(), (nz, ny, nx, cell)
    assert call(1, 2, 4, 0.1, 0., buf, buf) == _lib.EINVAL                 # occ == sdf
    assert eng.lib.sgpmp_voxel_sdf_build(eng._ctx, None, 1, 2, 4, 0.1, 0., _lib.ptr(out), _lib.stream_ptr()) == _lib.EINVAL
    torch.cuda.synchronize()
    assert bool((out == -3.).all()) and bool((buf == 7.).all())           # nothing was written
    with pytest.raises(ValueError):
        eng.voxel_sdf_build(torch.zeros(1, 4, 513, **TA(torch.float64)), 0.1)
    with pytest.raises(ValueError):
        eng.voxel_sdf_build(torch.zeros(4, 4, **TA(torch.float64)), 0.1)


# ------------------------------------------------------------------------------------------------ 2. sgpmp_field_grad
def reach(chain):
    return float(sum(np.linalg.norm(j[3]) for j in chain))


def field_errors(dtype, which, ni, seed, B=200):
    """(value error, gradient error, reference scales, oracle pieces) of compute_cost_and_grad at the seed's configurations."""
    f64 = dtype == torch.float64
    sc = scene()
    chain, n, rng = O.CHAINS[which]
    q = O.draw_configs(which, B, seed)
    if not f64:
        q = q.astype(np.float32).astype(np.float64)              # the oracle at the configurations the device is given
    fld = make_field(dtype, ni, rng)
    fo, go, _, _ = O.config_field_and_grad(q, chain, sc, ni, rng)
    keep = O.regular(q, chain, sc, 1e-6 if f64 else 1e-3, ni, rng)
    h, g = fld.compute_cost_and_grad(torch.from_numpy(q).to(**TA(dtype)), device_chain(which))
    h, g = h.double().cpu().numpy(), g.double().cpu().numpy()
    assert h.shape == (B,) and g.shape == (B, n)
    return dict(fld=fld, q=q, fo=fo, go=go, keep=keep, h=h, g=g, ev=np.abs(h - fo), eg=np.abs(g - go)[keep])


@pytest.mark.parametrize("ni", [0, 2])
@pytest.mark.parametrize("which", ["toy", "panda"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_field_and_gradient_match_oracle_and_autograd(dtype, which, ni):
    f64 = dtype == torch.float64
    sc = scene()
    r = field_errors(dtype, which, ni, SEED)
    fo, go, keep, h, g = r["fo"], r["go"], r["keep"], r["h"], r["g"]
    assert np.array_equal(r["fld"].sdf.cpu().numpy(), sc["sdf"].astype(NP(dtype)))
    # the conditions, on the oracle alone
    assert (~keep).sum() <= 0.05 * len(keep), int((~keep).sum())
    assert (fo == 0).sum() >= 50 and (fo > 0).sum() >= 50
    # inactive everywhere: the value and the gradient are exactly zero
    off = (fo == 0) & keep
    assert np.array_equal(h[off], np.zeros(off.sum())) and np.array_equal(g[off], np.zeros_like(g[off]))
    cap = sc["cell"] * sum(sc["sdf"].shape)
    print(f"    {which} ni={ni} {dtype}: value error {r['ev'].max():.3e} (max |f| {fo.max():.3g}), gradient error {r['eg'].max():.3e} "
          f"(max |df/dq| {np.abs(go).max():.3g}), {int((~keep).sum())} of {len(keep)} configurations left out of the gradient")
    if f64:
        tol = 1e-12 * max(1., cap)
        assert r["ev"].max() <= tol and r["eg"].max() <= tol * max(1., reach(O.CHAINS[which][0]))
    else:
        assert np.all(r["ev"] <= FP32_RTOL * np.abs(fo) + FP32_RTOL * np.abs(fo).max())
        assert np.all(r["eg"] <= FP32_RTOL * np.abs(go[keep]) + FP32_RTOL * np.abs(go).max())


@pytest.mark.parametrize("dtype", DTYPES)
def test_distance_query_collision_and_nan(dtype):
    f64 = dtype == torch.float64
    sc = scene()
    chain, n, rng = O.CHAINS["panda"]
    dchain = device_chain("panda")
    q = O.draw_configs("panda", 130, SEED + 1).astype(np.float32).astype(np.float64)
    fld = make_field(dtype, 2, rng)
    _, _, dmin, gd = O.config_field_and_grad(q, chain, sc, 2, rng)
    qd = torch.from_numpy(q).to(**TA(dtype))
    d, g = fld.compute_distance(qd, dchain), fld._query(qd, dchain)[1]
    assert d.shape == (130,) and g.shape == (130, 7)
    tol = 1e-12 * max(1., sc["cell"] * sum(sc["sdf"].shape)) if f64 else FP32_RTOL * np.abs(dmin).max()
    assert np.abs(d.double().cpu().numpy() - dmin).max() <= tol
    # the gradient goes through the arg-min point: where the oracle's two best distinct distances are well apart and off the kinks
    pts = O.link_points(torch.from_numpy(q), chain, 2, rng)
    dist = np.sort(O.distance_torch(sc["sdf"], pts, sc["cell"], sc["origin"]).numpy(), axis=1)
    gap = np.array([row[row > row[0] + 1e-12][0] - row[0] for row in dist])
    keep = O.regular(q, chain, sc, 1e-6 if f64 else 1e-3, 2, rng) & (gap > 1e-4)
    assert keep.sum() >= 100
    gtol = tol * max(1., reach(chain)) if f64 else FP32_RTOL * np.abs(gd).max()
    assert np.abs(g.double().cpu().numpy() - gd)[keep].max() <= gtol
    assert (dmin < 0).sum() >= 5 and (dmin > 0.05).sum() >= 5
    hit = fld.compute_collision(qd, dchain, buffer=0.02).cpu().numpy()
    sure = np.abs(dmin - 0.02) > 1e-4
    assert hit.dtype == bool and np.array_equal(hit[sure], (dmin < 0.02)[sure])
    # a non-finite joint value: NaN in the value and the gradient of that configuration alone, for the hinge and for the query
    bad = qd.clone()
    bad[3, 2], bad[7, 6] = float("nan"), float("inf")
    h0, g0 = fld.compute_cost_and_grad(qd, dchain)
    h1, g1 = fld.compute_cost_and_grad(bad, dchain)
    rows = torch.tensor([3, 7], device=DEV)
    keep_t = torch.ones(130, dtype=torch.bool, device=DEV)
    keep_t[rows] = False
    assert bool(torch.isnan(h1[rows]).all()) and bool(torch.isnan(g1[rows]).all())
    assert torch.equal(h1[keep_t], h0[keep_t]) and torch.equal(g1[keep_t], g0[keep_t])
    assert bool(torch.isnan(fld.compute_distance(bad, dchain)[rows]).all())


# ------------------------------------------------------------------------------------------------ 3. compute_cost on frames
@pytest.mark.parametrize("which,ni", [("toy", 0), ("toy", 2), ("panda", 0), ("panda", 2)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_compute_cost_on_frames_equals_the_field_grad_value(dtype, which, ni):
    from stoch_gpmp_amd.engine import Engine
    f64 = dtype == torch.float64
    sc = scene()
    chain, n, rng = O.CHAINS[which]
    q = O.draw_configs(which, 130, SEED).astype(np.float32).astype(np.float64)
    fld = make_field(dtype, ni, rng)
    eng = Engine(n, 2, 0, 1, tensor_args=TA(dtype))
    eng.set_fk(device_chain(which), codegen=False)
    qd = torch.from_numpy(q).to(**TA(dtype))
    frames = eng.fk(qd).reshape(10, 13, len(chain) + 1, 4, 4)
    cost = fld.compute_cost(frames)
    assert cost.shape == (10, 13)
    value, _ = fld.compute_cost_and_grad(qd, device_chain(which))
    fo = O.frames_field(O.fk_all_links(torch.from_numpy(q), chain), sc, ni, rng).numpy()
    tol = 1e-12 * max(1., sc["cell"] * sum(sc["sdf"].shape)) if f64 else FP32_RTOL * np.abs(fo).max()
    assert float(fo.max()) > 0.3 and (fo == 0).any()
    assert np.abs(cost.double().cpu().numpy().ravel() - value.double().cpu().numpy()).max() <= tol
    assert np.abs(cost.double().cpu().numpy().ravel() - fo).max() <= tol
    assert np.array_equal(cost.cpu().numpy().ravel()[fo == 0], np.zeros((fo == 0).sum()))


def test_get_linear_system_through_the_field_factor():
    """CostCollision inside a CostComposite: FieldFactor.get_error -> compute_cost_and_grad with the composite's chain."""
    from oracle import ref_equiv as R
    from stoch_gpmp_amd.costs.cost_functions import CostCollision, CostComposite
    from stoch_gpmp_amd.robots.panda import DifferentiableFrankaPanda
    T, P, sigma = 5, 3, 0.02
    ta, sc = TA(torch.float64), scene()
    fk = DifferentiableFrankaPanda(gripper=False, device=DEV)
    comp = CostComposite(7, T, [CostCollision(7, T, field=make_field(torch.float64, 2), sigma_coll=sigma, tensor_args=ta)],
                         FK=fk.compute_forward_kinematics_all_links, tensor_args=ta)
    means = O.gpmp_means(T, P)
    A, b, K = comp.get_linear_system(means.to(**ta))
    Ao, bo, Ko = R.collision_linear_system(means, 7, O.fk_all_links, lambda fr: O.frames_field(fr, sc, 2), sigma)
    assert float(bo.abs().max()) > 0 and float(Ao.abs().max()) > 0
    assert rel_err(A, Ao) < 1e-12 and rel_err(b, bo) < 1e-12 and rel_err(K, Ko) < 1e-12


# ------------------------------------------------------------------------------------------------ 4. the sweep
SWEEP_SIGMA = 0.05
FLAVOURS = {"generated chain": ("panda", 0, None), "register FK": ("panda", 0, "no_chain_codegen"),
            "generic FK": ("panda", 0, "force_generic_fk"), "generic FK, toy chain": ("toy", 0, None),
            "generic FK, interpolated points": ("panda", 2, None)}


def sweep_trajs(which, T, B, seed):
    """B smooth random walks in joint space from configurations of the seeded pool whose field is active."""
    chain, n, rng = O.CHAINS[which]
    pool = O.draw_configs(which, 200, SEED)
    f, _, _, _ = O.config_field_and_grad(pool, chain, scene(), 0, rng)
    q0 = torch.from_numpy(pool[f > 0.2][:B])
    gen = torch.Generator().manual_seed(seed)
    steps = 0.04 * torch.randn(B, T, n, generator=gen, dtype=torch.float64)
    steps[:, 0] = 0
    x = torch.zeros(B, T, 2 * n, dtype=torch.float64)
    x[..., :n] = q0[:, None] + steps.cumsum(1)
    return x


@pytest.mark.parametrize("flavour", list(FLAVOURS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_sweep_adds_k_times_the_sum_of_the_field(dtype, flavour):
    from stoch_gpmp_amd import _lib as L
    from stoch_gpmp_amd.engine import Engine
    f64 = dtype == torch.float64
    which, ni, option = FLAVOURS[flavour]
    chain, n, rng = O.CHAINS[which]
    sc = scene()
    fld = make_field(dtype, ni, rng)
    K = 1. / SWEEP_SIGMA ** 2
    gp = dict(kind=L.COST_GP, flags=0, sigma=10., dt=0.05)
    worst = 0.
    for T in (3, 70):
        B = 5
        x = sweep_trajs(which, T, B, seed=T).to(dtype)
        xd = x.to(DEV).contiguous()
        out = []
        for descs in ([gp, fld.descriptor(SWEEP_SIGMA)], [gp]):
            eng = Engine(n, T, 0, 1, tensor_args=TA(dtype))
            eng.set_fk(device_chain(which), codegen=False)
            if option:
                eng.set_option(option, 1)
            eng.set_costs(descs)
            out.append(eng.cost_eval(xd, out64=torch.empty(B, device=DEV, dtype=torch.float64)).cpu().numpy())
            if len(descs) == 2:
                name = eng.last_cost_kernel()
                assert name.startswith("cost_sweep_kernel") and flavour.split(",")[0] in name, name
        f = O.frames_field(O.fk_all_links(x.double()[:, 1:, :n].reshape(-1, n), chain), sc, ni, rng).reshape(B, T - 1).numpy()
        add = K * f.sum(1)
        ref = out[1] + add
        assert float(add.min()) > 0 and float((add / ref).min()) > 0.3      # the term is there, and it is no rounding error of the rest
        err = float((np.abs(out[0] - ref) / np.abs(ref)).max())
        worst = max(worst, err)
    print(f"    {flavour} {dtype}: worst relative error of a cost {worst:.3e}")
    assert worst <= (1e-12 if f64 else FP32_SWEEP_RTOL), worst


# ------------------------------------------------------------------------------------------------ 5. the step
def arm_planner(dtype, field, T=16, nppg=2, S=8, seed=31, **kw):
    from stoch_gpmp_amd.costs.cost_functions import CostCollision, CostComposite, CostGP, CostGoalPrior
    from stoch_gpmp_amd.planner import StochGPMP
    from stoch_gpmp_amd.robots.panda import DifferentiableFrankaPanda
    c, ta, n = O.ARM_C, TA(dtype), 7
    start, goals = torch.tensor(c["start_q"] + [0.] * n, **ta), torch.tensor([c["goal_q"] + [0.] * n], **ta)
    fk = DifferentiableFrankaPanda(gripper=False, device=DEV)
    cost = CostComposite(n, T, [
        CostGP(n, T, start, c["dt"], dict(sigma_start=c["cost_sigma_start"], sigma_gp=c["cost_sigma_gp"]), ta),
        CostGoalPrior(n, T, multi_goal_states=goals, num_particles_per_goal=nppg, num_samples=S, sigma_goal_prior=c["sigma_goal_prior"],
                      tensor_args=ta),
        CostCollision(n, T, field=field, sigma_coll=c["sigma_coll"], tensor_args=ta)],
        FK=fk.compute_forward_kinematics_all_links, tensor_args=ta)
    return StochGPMP(num_particles_per_goal=nppg, num_samples=S, traj_len=T, opt_iters=1, dt=c["dt"], n_dof=n, step_size=0.5,
                     temperature=1., start_state=start, multi_goal_states=goals, cost=cost,
                     sigma_start_init=c["sigma_start_init"], sigma_start_sample=c["sigma_start_sample"],
                     sigma_goal_init=c["sigma_goal_init"], sigma_goal_sample=c["sigma_goal_sample"],
                     sigma_gp_init=c["sigma_gp_init"], sigma_gp_sample=c["sigma_gp_sample"], seed=seed, tensor_args=ta, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
def test_step_with_the_term_is_sampler_sweep_update_bit_for_bit(dtype):
    from stoch_gpmp_amd import _lib as L
    from stoch_gpmp_amd.engine import Engine
    fld = make_field(dtype)
    p, q = arm_planner(dtype, fld), arm_planner(dtype, fld)
    assert torch.equal(p.particle_means, q.particle_means)
    costs, grad = p.step()
    name = p._engine.last_cost_kernel()
    assert "fused" not in name and name.startswith("cost_sweep_kernel") and "generated chain" in name, name
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
    descs = q.cost.descriptors()
    assert descs[-1]["kind"] == L.COST_VOXEL_SDF
    bare = Engine(7, 16, 0, 1, tensor_args=TA(dtype))
    bare.set_fk(device_chain("panda"), codegen=False)
    bare.set_costs(descs[:-1])
    c1 = eng.cost_eval(smp, out64=torch.empty(P * S, device=DEV, dtype=torch.float64))
    c0 = bare.cost_eval(smp, out64=torch.empty(P * S, device=DEV, dtype=torch.float64))
    assert float((c1 - c0).min()) > 0


# ------------------------------------------------------------------------------------------------ 6. GPMP
def arm_gpmp(means, dtype, delta, trust, n_sub, field):
    from stoch_gpmp_amd.costs.cost_functions import CostCollision, CostComposite, CostGP, CostGoalPrior
    from stoch_gpmp_amd.robots.panda import DifferentiableFrankaPanda
    c, ta, n = O.ARM_C, TA(dtype), 7
    P, T, _ = means.shape
    start, goals = torch.tensor(c["start_q"] + [0.] * n, **ta), torch.tensor([c["goal_q"] + [0.] * n], **ta)
    fk = DifferentiableFrankaPanda(gripper=False, device=DEV)
    cost = CostComposite(n, T, [
        CostGP(n, T, start, c["dt"], dict(sigma_start=c["cost_sigma_start"], sigma_gp=c["cost_sigma_gp"]), ta),
        CostGoalPrior(n, T, multi_goal_states=goals, num_particles_per_goal=P, num_samples=1, sigma_goal_prior=c["sigma_goal_prior"],
                      tensor_args=ta),
        CostCollision(n, T, field=field, sigma_coll=c["sigma_coll"], tensor_args=ta)],
        FK=fk.compute_forward_kinematics_all_links, tensor_args=ta)
    dense = dict(n_sub=n_sub, weight=1.0) if n_sub > 0 else None
    return hip_gpmp(means, goals, P, ta, delta, trust, dense_cost=dense, cost=cost, c=c, start=start)


@pytest.mark.parametrize("n_sub", [0, 2])
@pytest.mark.parametrize("T,P", [(2, 1), (3, 5), (16, 4)])
def test_gpmp_rows_match_the_oracle(T, P, n_sub):
    """The term's rows of sgpmp_gpmp_linearize (value f, A = -df/dq, precision K; with n_sub also on the inserted states) through what
    is made of them: the trust-region diagonal sum_p diag(A^T K A), and two Gauss-Newton iterations against OracleGPMP."""
    sc = scene()
    means = O.gpmp_means(T, P)
    fn = O.gpmp_systems_fn(sc, n_sub)
    want = DO.field_dense_diag(fn(means))
    pl = arm_gpmp(means, torch.float64, 1e-2, True, n_sub, make_field(torch.float64))
    diag = torch.zeros(T * 14, device=DEV, dtype=torch.float64)
    pl._engine.gpmp_linearize(pl.particle_means, diag_sum=diag)
    assert float(want.abs().max()) > 0 and rel_err(diag, want) < 1e-9
    ora = GP.OracleGPMP(means, fn, 0.5, 5.0, False, SOLVE)
    ora0 = GP.OracleGPMP(means, O.gpmp_systems_fn(sc, n_sub, field=False), 0.5, 5.0, False, SOLVE)
    pl = arm_gpmp(means, torch.float64, 5.0, False, n_sub, make_field(torch.float64))
    d0, _ = ora0.step()
    for it in range(2):
        d_o, c_o = ora.step()
        if it == 0:
            moved = DO.rel_l2(d0, d_o)
            print(f"    T={T} P={P} n_sub={n_sub}: the field rows move d_theta by {moved:.3f} (relative L2)")
            assert moved >= 0.05, moved
        _, _, costs = pl.optimize()
        assert pl._engine.last_gpmp_kernel() == ("gpmp_thomas_kernel" if n_sub == 0 else "gpmp_dense_solve_kernel")
        e = (rel_err(pl._d_theta, d_o), rel_err(costs, c_o), rel_err(pl.particle_means, ora.particle_means))
        print(f"      iteration {it}: d_theta {e[0]:.2e} costs {e[1]:.2e} means {e[2]:.2e}")
        assert e[0] < 1e-7 and e[1] < 1e-9 and e[2] < 1e-8, (it, e)


def test_gpmp_fp32_one_iteration_and_the_query_flag_is_refused():
    from stoch_gpmp_amd import _lib
    from stoch_gpmp_amd.engine import Engine
    T, P = 16, 4
    sc = scene()
    means = O.gpmp_means(T, P)
    for k in (0, 2):
        ora = GP.OracleGPMP(means, O.gpmp_systems_fn(sc, k), 0.5, 5.0, False, SOLVE)
        d_o, c_o = ora.step()
        pl = arm_gpmp(means, torch.float32, 5.0, False, k, make_field(torch.float32))
        _, _, costs = pl.optimize()
        e = (rel_err(costs, c_o), rel_err(pl.particle_means, ora.particle_means))
        print(f"    fp32 GPMP n_sub={k}: costs {e[0]:.3e} means {e[1]:.3e} (relative, against the fp64 oracle)")
        assert e[0] < 1e-4 and e[1] < 1e-4, e
    # SGPMP_FLAG_GRID_DISTANCE turns sgpmp_field_grad's answer into min d and its gradient: refused next to other terms and by GPMP
    ta = TA(torch.float64)
    fld = make_field(torch.float64)
    flagged = fld.descriptor(0.1, distance=True)
    gp = [dict(kind=_lib.COST_GP, flags=0, sigma=0.5, dt=0.1)]
    eng = Engine(7, 4, 1, 1, tensor_args=ta)
    eng.set_fk(device_chain("panda"), codegen=False)
    with pytest.raises(ValueError, match="query flag"):
        eng.set_costs(gp + [flagged])
    with pytest.raises(ValueError, match="query flag"):
        eng.set_costs([flagged, fld.descriptor(0.1)])
    eng.set_costs([flagged])                                                # alone: the query compute_distance makes
    with pytest.raises(ValueError, match="GPMP"):
        eng.gpmp_linearize(O.gpmp_means(4, 1).to(**ta))
    eng.set_costs(gp + [fld.descriptor(0.1)])
    eng.gpmp_linearize(O.gpmp_means(4, 1).to(**ta))                          # the plain term is a GPMP field


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_dense_trajectory_entry_points_refuse_the_term_and_the_term_needs_a_chain():
    from stoch_gpmp_amd import _lib as L
    from stoch_gpmp_amd.engine import Engine
    dtype = torch.float64
    ta = TA(dtype)
    fld = make_field(dtype)
    T = 6
    gp = dict(kind=L.COST_GP, flags=0, sigma=1., dt=0.1)
    eng = Engine(7, T, 0, 1, tensor_args=ta)
    eng.set_fk(device_chain("panda"), codegen=False)
    eng.set_costs([gp, fld.descriptor(0.05)])
    xd = O.gpmp_means(T, 3).to(**ta).contiguous()
    with pytest.raises(ValueError, match=r"sgpmp_dense_cost: cost term 1 \(SGPMP_COST_VOXEL_SDF\)"):
        eng.dense_cost(xd, 2, 0.1, out64=torch.empty(3, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"sgpmp_dense_cost_grad: cost term 1 \(SGPMP_COST_VOXEL_SDF\)"):
        eng.dense_cost_grad(xd, 2, 0.1)
    with pytest.raises(ValueError, match=r"sgpmp_validate: cost term 1 \(SGPMP_COST_VOXEL_SDF\)"):
        eng.validate(xd, 2, 0.1)
    eng.cost_eval(xd, out64=torch.empty(3, device=DEV, dtype=torch.float64))     # (the sweep takes the list)
    # the planner's dense_cost= option: ValueError at the step that would evaluate it
    pl = arm_planner(dtype, fld, T=8, nppg=1, S=4, dense_cost=dict(n_sub=2, weight=1.0))
    with pytest.raises(ValueError, match="SGPMP_COST_VOXEL_SDF"):
        pl.step()
    # no FK chain: SGPMP_ESTATE from every consumer
    bare = Engine(7, T, 1, 1, tensor_args=ta)
    bare.set_costs([gp, fld.descriptor(0.05)])
    q = torch.zeros(2, 7, **ta)
    val, grad = torch.empty(2, **ta), torch.empty(2, 7, **ta)
    for rc in (bare.lib.sgpmp_field_grad(bare._ctx, 1, L.ptr(q), 2, None, 0, L.ptr(val), L.ptr(grad), L.stream_ptr()),
               bare.lib.sgpmp_cost_eval(bare._ctx, L.ptr(xd), 3, 0, None, 0, None, 1, None, L.ptr(torch.empty(3, device=DEV, dtype=torch.float64)),
                                        L.stream_ptr()),
               bare.lib.sgpmp_gpmp_linearize(bare._ctx, L.ptr(xd[:1].contiguous()), None, 0, None, L.stream_ptr())):
        assert rc == L.ESTATE, (rc, L.last_error())
    # bad descriptors
    for edit in (dict(reserved=0), dict(dim0=0), dict(p0=0.), dict(sigma2=-0.1), dict(num_interpolate=9)):
        with pytest.raises(ValueError):
            eng.set_costs([dict(fld.descriptor(0.05), **edit)])


# ------------------------------------------------------------------------------------------------ 8. update()
def test_update_rebuilds_on_the_device_and_planners_recompile():
    from stoch_gpmp_amd.envs.voxel_map import VoxelMap
    dtype = torch.float64
    sc = scene()
    vm = VoxelMap.from_grid(sc["occ"], sc["cell"], sc["lower"], tensor_args=TA(dtype))
    fld = vm.distance_field(O.MARGIN)
    a = arm_planner(dtype, fld, seed=7)
    a.step()
    v0, ptr0 = fld._version, fld.sdf.data_ptr()
    vm.occ.zero_()
    vm.add_box((0.3, -0.2, 0.4), (0.25, 0.3, 0.2)).add_sphere((0.1, 0.3, 0.5), 0.12)       # the scene changes
    occ2 = vm.occ.cpu().numpy()
    assert 20 < occ2.sum() < occ2.size / 2 and not np.array_equal(occ2, sc["occ"])
    assert fld.update() is fld.sdf and fld._version == v0 + 1 and fld.sdf.data_ptr() == ptr0
    assert np.array_equal(fld.sdf.cpu().numpy(), O.brute_sdf(occ2, sc["cell"]))
    fresh = VoxelMap.from_grid(occ2, sc["cell"], sc["lower"], tensor_args=TA(dtype)).distance_field(O.MARGIN)
    assert torch.equal(fresh.sdf, fld.sdf)

    def costs_of(field, prev, draw):
        f = arm_planner(dtype, field, seed=7)
        f.particle_means.copy_(prev)
        f._draw = draw
        return f.step()[0]
    # a's next step sees the new volume: its costs are those of a planner built on it at the same means and draw, not the old one's
    prev, draw = a.particle_means.clone(), a._draw
    ca = a.step()[0].clone()
    assert torch.equal(ca, costs_of(fresh, prev, draw))
    assert not torch.equal(ca, costs_of(make_field(dtype), prev, draw))
    # a volume of ANOTHER SHAPE (three more slices on top, a slab in them): update() has to hand out a new tensor, so only a planner
    # that re-compiled its cost program (the version moved) can see it
    occ3 = np.zeros((occ2.shape[0] + 3,) + occ2.shape[1:])
    occ3[:occ2.shape[0]] = occ2
    occ3[-2:, 2:9, 3:11] = 1.
    vm.occ = torch.as_tensor(occ3).to(**TA(dtype))
    old_sdf, v1 = fld.sdf, fld._version
    assert fld.update() is fld.sdf and fld.sdf is not old_sdf and tuple(fld.sdf.shape) == occ3.shape and fld._version == v1 + 1
    assert np.array_equal(fld.sdf.cpu().numpy(), O.brute_sdf(occ3, sc["cell"]))
    prev, draw = a.particle_means.clone(), a._draw
    ca = a.step()[0].clone()
    grown = VoxelMap.from_grid(occ3, sc["cell"], sc["lower"], tensor_args=TA(dtype)).distance_field(O.MARGIN)
    assert torch.equal(ca, costs_of(grown, prev, draw))
    assert not torch.equal(ca, costs_of(fresh, prev, draw))
    # the field's own query engines follow
    q = torch.from_numpy(O.draw_configs("panda", 9, 3)).to(**TA(dtype))
    assert torch.equal(fld.compute_cost_and_grad(q, device_chain("panda"))[0], grown.compute_cost_and_grad(q, device_chain("panda"))[0])


def test_voxel_map_painting_matches_numpy():
    from stoch_gpmp_amd.envs.voxel_map import VoxelMap
    vm = VoxelMap((1.04, 1.12, 0.8), 0.08, (-0.4, -0.5, 0.0), TA(torch.float64))
    assert tuple(vm.occ.shape) == (10, 14, 13) and np.allclose(vm.origin, (5.0, 6.25, 0.0))
    vm.add_box((0.3, -0.2, 0.4), (0.25, 0.3, 0.2)).add_sphere((0.1, 0.3, 0.5), 0.12)
    c = [lo + (np.arange(n) + 0.5) * 0.08 for lo, n in zip((-0.4, -0.5, 0.0), (13, 14, 10))]
    X, Y, Z = c[0][None, None, :], c[1][None, :, None], c[2][:, None, None]
    box = (np.abs(X - 0.3) <= 0.125) & (np.abs(Y + 0.2) <= 0.15) & (np.abs(Z - 0.4) <= 0.1)       # (no cell centre on a face)
    r2 = (X - 0.1) ** 2 + (Y - 0.3) ** 2 + (Z - 0.5) ** 2
    got = vm.occ.cpu().numpy()
    assert set(np.unique(got)) == {0., 1.} and box.sum() == 3 * 4 * 2 and (r2 <= 0.12 ** 2).sum() >= 7
    sure = np.abs(r2 - 0.12 ** 2) > 1e-12
    assert np.array_equal((got > 0)[sure], (box | (r2 <= 0.12 ** 2))[sure])


# ------------------------------------------------------------------------------------------------ 9. end to end
def test_gpmp_moves_the_panda_around_a_box_end_to_end():
    spec = importlib.util.spec_from_file_location("panda_voxel_gpmp", os.path.join(ROOT, "examples", "panda_voxel_gpmp.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    planner, field, chain, history, (first, last) = ex.main(verbose=False)
    s = ex.SETTINGS
    assert len(history) == s["opt_iters"] and planner._engine.last_gpmp_kernel() == "gpmp_dense_solve_kernel"
    # on the oracle: the straight line passes through the box, the result keeps every point of every support waypoint outside
    occ = field.voxel_map.occ.cpu().numpy()
    sdf = O.brute_sdf(occ, ex.CELL) if occ.size <= 4000 else O.scipy_sdf(occ, ex.CELL)
    assert np.array_equal(field.sdf.cpu().numpy(), sdf)
    origin = tuple(-c / ex.CELL for c in ex.LOWER)

    def point_distances(m):
        pts = O.link_points(m.double().cpu().reshape(-1, 14)[:, :7], O.PANDA_CHAIN)
        return O.distance_torch(sdf, pts, ex.CELL, origin)
    d0 = point_distances(ex.straight_line(s["traj_len"], s["dt"]))
    d1 = point_distances(planner.particle_means)
    print(f"    straight line: min d {float(d0.min()):+.4f} (device query {first:+.4f}); after {s['opt_iters']} iterations: "
          f"min d {float(d1.min()):+.4f} (device query {last:+.4f}); cost {history[0]:.4g} -> {history[-1]:.4g}")
    assert float(d0.min()) < 0 and abs(first - float(d0.min())) < 1e-9
    assert float(d1.min()) >= 0 and abs(last - float(d1.min())) < 1e-9
    assert history[-1] < history[0]
    assert bool(torch.isfinite(planner.particle_means).all()) and np.isfinite(history).all()
