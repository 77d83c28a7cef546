"""The body collision spheres on the voxel signed-distance field (SGPMP_COST_BODY_SDF, csrc/body_sdf.hip) on the GPU: the term in
sgpmp_field_grad, sgpmp_field_eval, the sweep (generic sweep + body_cost_kernel), the step, GPMP with and without continuous-time
factors, the clearance query and the refusals, against the test-side oracle (tests/body_sdf_oracle.py: torch fp64, autograd through
oracle/fk.py).  Needs the MI355X: run with `-m gpu`.

fp64 bounds: 1e-12 max(1, cap) on field values, the same times the chain's reach on gradients, 1e-12 relative for the sweep,
tests/test_gpu_gpmp_dense.py's for GPMP (d_theta 1e-7, costs 1e-9, means 1e-8).  fp32 bounds: 3e-4 relative plus 3e-4 of the
largest reference value for the field and its Jacobian, 2e-4 for the sweep, 1e-4 for one GPMP iteration -- the bounds of
tests/test_gpu_voxel_sdf.py.
Measured on the MI355X (profiles/r15/body_sdf.txt), worst over all cases: field value / value on frames / Jacobian 4.4e-15 /
3.6e-15 / 7.1e-15 in fp64 and 2.7e-6 / 1.6e-6 / 4.8e-6 in fp32 (the 64-sphere body; along_links 8.5e-7 / 5.1e-7 / 1.1e-6); the
zero-radius body against the voxel term 2.8e-17 / 2.7e-7; minimum clearance and its gradient 1.4e-16 / 9.6e-16 and 7.5e-8 / 3.4e-7; a
sweep cost 7.1e-16 / 3.2e-7 relative; GPMP fp64 d_theta 3.7e-13, costs 8.9e-14, means 1.7e-13, fp32 costs 1.4e-7, means 2.2e-7."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import gpmp_equiv as GP
from oracle.fk import fk_all_links
from tests import body_sdf_oracle as BO
from tests import gpmp_dense_oracle as DO
from tests import voxel_sdf_oracle as VO
from tests.test_gpu_gpmp_dense import rel_err
from tests.test_gpu_voxel_sdf import FP32_RTOL, FP32_SWEEP_RTOL, SOLVE, TA, arm_gpmp, arm_planner, device_chain, scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
DTYPES = [torch.float64, torch.float32]
SEED = 3                            # tests/test_cpu_body_sdf.py holds this seed's configurations to the conditions, on the oracle
SPACING, RADIUS = 0.12, 0.06
_REF = {}


def bodies(which):
    """name -> BodySpheres of chain `which`: along_links, one sphere, the largest table, link 0 only (no gradient), the last link
    only, and a sphere on the link behind the chain's first fixed joint."""
    from stoch_gpmp_amd.robots.body import BodySpheres
    chain = VO.CHAINS[which][0]
    L = len(chain) + 1
    rng = np.random.default_rng(5)
    fixed = [j for j, joint in enumerate(chain) if joint[1] == "fixed"][0]
    out = {"along_links": BodySpheres.along_links(chain, SPACING, RADIUS),
           "M=1": BodySpheres([L // 2], [(0.03, -0.02, 0.04)], [0.05]),
           "M=64": BodySpheres(rng.integers(0, L, 64), rng.uniform(-0.1, 0.1, (64, 3)), rng.uniform(0., 0.12, 64)),
           "link 0 only": BodySpheres([0, 0], [(0.1, 0., 0.2), (0.3, 0.1, 0.3)], [0.05, 0.2]),
           "last link only": BodySpheres([L - 1], [(0.02, -0.01, 0.03)], [0.07]),
           "behind a fixed joint": BodySpheres([fixed + 1], [(0., 0.03, 0.02)], [0.06])}
    return out


def reference(which, name, B):
    """The oracle's answers for body `name` on the seeded configurations, computed once and shared."""
    key = (which, name, B)
    if key not in _REF:
        chain, body, sc = VO.CHAINS[which][0], bodies(which)[name], scene()
        q = VO.draw_configs(which, 130, SEED)[:B]
        f, g, smin, gs, s = BO.config_field_and_grad(q, chain, body, sc)
        _REF[key] = dict(q=q, f=f, g=g, smin=smin, gs=gs, s=s, reg6=BO.regular(q, chain, body, sc, 1e-6),
                         reg3=BO.regular(q, chain, body, sc, 1e-3))
    return _REF[key]


def make_field(dtype, body, margin=VO.MARGIN, sc=None):
    from stoch_gpmp_amd.envs.voxel_map import VoxelMap
    sc = scene() if sc is None else sc
    vm = VoxelMap.from_grid(sc["occ"], sc["cell"], sc["lower"], tensor_args=TA(dtype))
    return vm.body_field(body, margin)


def reach(chain):
    return float(sum(np.linalg.norm(j[3]) for j in chain))


def cap():
    sc = scene()
    return sc["cell"] * sum(sc["sdf"].shape)


# ------------------------------------------------------------------------------------------------ 1. field and gradient
@pytest.mark.parametrize("name", ["along_links", "M=1", "M=64", "link 0 only", "last link only", "behind a fixed joint"])
@pytest.mark.parametrize("which", ["toy", "panda"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_field_and_gradient_match_the_oracle(dtype, which, name):
    f64 = dtype == torch.float64
    chain, body = VO.CHAINS[which][0], bodies(which)[name]
    fld = make_field(dtype, body)
    worst = [0., 0., 0.]
    for B in ((1, 63, 64, 65, 130) if name in ("along_links", "M=1", "M=64") else (65,)):
        r = reference(which, name, B)
        q = torch.from_numpy(r["q"]).to(**TA(dtype)).contiguous()
        val, grad = fld.compute_cost_and_grad(q, device_chain(which))
        val2, grad2 = fld.compute_cost_and_grad(q, device_chain(which))
        assert torch.equal(val, val2) and torch.equal(grad, grad2)               # two calls: the same bits
        frames = fk_all_links(torch.from_numpy(r["q"]), chain).to(**TA(dtype)).contiguous()
        on_frames = fld.compute_cost(frames)
        if name == "M=1" and B == 65:                    # frames of more links than a chain may have joints: only the body's links count
            pad = torch.eye(4, **TA(dtype)).expand(B, 20 - frames.shape[1], 4, 4)
            assert torch.equal(fld.compute_cost(torch.cat([frames, pad], 1).contiguous()), on_frames)
        val, grad, on_frames = val.cpu().double().numpy(), grad.cpu().double().numpy(), on_frames.cpu().double().numpy()
        reg = r["reg6"] if f64 else r["reg3"]
        vtol = 1e-12 * max(1., cap()) if f64 else FP32_RTOL * np.abs(r["f"]) + FP32_RTOL * np.abs(r["f"]).max()
        gtol = 1e-12 * max(1., cap()) * reach(chain) if f64 else FP32_RTOL * np.abs(r["g"]) + FP32_RTOL * np.abs(r["g"]).max()
        ev, ef = np.abs(val - r["f"]), np.abs(on_frames - r["f"])
        eg = np.abs(grad - r["g"])
        worst = [max(worst[0], float(ev.max())), max(worst[1], float(ef.max())), max(worst[2], float(eg[reg].max()) if reg.any() else 0.)]
        assert (ev <= vtol).all() and (ef <= vtol).all(), (B, float(ev.max()), float(ef.max()))
        assert (eg[reg] <= (gtol[reg] if not f64 else gtol)).all(), (B, float(eg[reg].max()))
        if name == "link 0 only":
            assert np.array_equal(grad, np.zeros_like(grad)) and (val > 0).all()   # exactly zero: no joint in front of link 0
    print(f"    {dtype} {which} {name}: worst |value - oracle| {worst[0]:.2e}, on frames {worst[1]:.2e}, |gradient - autograd| {worst[2]:.2e}")
    if name in ("along_links", "M=64"):
        r = reference(which, name, 65)
        assert (r["f"] > 0).any() and (np.abs(r["g"]) > 0).any()


@pytest.mark.parametrize("which", ["toy", "panda"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_offset_zero_radius_body_equals_the_voxel_term(dtype, which):
    from stoch_gpmp_amd.envs.voxel_map import VoxelMap
    from stoch_gpmp_amd.robots.body import BodySpheres
    chain = VO.CHAINS[which][0]
    L = len(chain) + 1
    sc = scene()
    vm = VoxelMap.from_grid(sc["occ"], sc["cell"], sc["lower"], tensor_args=TA(dtype))
    body_f = vm.body_field(BodySpheres(range(L), [(0., 0., 0.)] * L, [0.] * L), VO.MARGIN)
    point_f = vm.distance_field(VO.MARGIN, num_interpolate=0)
    q = torch.from_numpy(VO.draw_configs(which, 130, SEED)).to(**TA(dtype)).contiguous()
    vb, gb = body_f.compute_cost_and_grad(q, device_chain(which))
    vp, gp = point_f.compute_cost_and_grad(q, device_chain(which))
    tol = 1e-12 * max(1., cap()) if dtype == torch.float64 else FP32_RTOL * float(vp.abs().max())
    err = float((vb - vp).abs().max())
    print(f"    {dtype} {which}: |body - voxel term| {err:.2e}, gradients {float((gb - gp).abs().max()):.2e}")
    assert err <= tol and float(vp.max()) > 0
    if dtype == torch.float64:
        assert float((gb - gp).abs().max()) <= tol * reach(chain)


# ------------------------------------------------------------------------------------------------ 2. the query
@pytest.mark.parametrize("which", ["toy", "panda"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_clearance_query_collision_and_nan(dtype, which):
    f64 = dtype == torch.float64
    chain = VO.CHAINS[which][0]
    fld = make_field(dtype, bodies(which)["along_links"])
    r = reference(which, "along_links", 130)
    q = torch.from_numpy(r["q"]).to(**TA(dtype)).contiguous()
    smin, gs = fld._query(q, device_chain(which))
    assert torch.equal(fld.compute_distance(q, device_chain(which)), smin)
    smin, gs = smin.cpu().double().numpy(), gs.cpu().double().numpy()
    vtol = 1e-12 * max(1., cap()) if f64 else FP32_RTOL * np.abs(r["smin"]) + FP32_RTOL * np.abs(r["smin"]).max()
    assert (np.abs(smin - r["smin"]) <= vtol).all()
    ok = (BO.argmin_gap(r["s"]) > 1e-4) & (r["reg6"] if f64 else r["reg3"])
    gtol = 1e-12 * max(1., cap()) * reach(chain) if f64 else (FP32_RTOL * np.abs(r["gs"]) + FP32_RTOL * np.abs(r["gs"]).max())[ok]
    print(f"    {dtype} {which}: |min clearance - oracle| {np.abs(smin - r['smin']).max():.2e}, its gradient "
          f"{np.abs(gs - r['gs'])[ok].max():.2e} on {int(ok.sum())} of {len(ok)} configurations")
    assert ok.sum() >= 60 and (np.abs(gs - r["gs"])[ok] <= gtol).all()
    # compute_collision away from the threshold
    for buffer in (0., 0.05):
        far = np.abs(r["smin"] - buffer) > 1e-3
        hit = fld.compute_collision(q, device_chain(which), buffer=buffer).cpu().numpy()
        assert np.array_equal(hit[far], (r["smin"] < buffer)[far]) and hit[far].any() and not hit[far].all()
    # a non-finite joint value: NaN in the value and in EVERY gradient entry, of the field and of the query
    n = q.shape[1]
    bad = q[:4].clone()
    bad[1, n - 1] = float("nan")
    bad[2, 0] = float("inf")
    for val, grad in (fld._query(bad, device_chain(which)), fld.compute_cost_and_grad(bad, device_chain(which))):
        assert bool(torch.isnan(val[1:3]).all()) and bool(torch.isnan(grad[1:3]).all())
        assert bool(torch.isfinite(val[[0, 3]]).all()) and bool(torch.isfinite(grad[[0, 3]]).all())


# ------------------------------------------------------------------------------------------------ 3. the sweep
SWEEP_SIGMA = 0.05


def sweep_trajs(which, T, B, seed):
    """B smooth random walks in joint space from configurations of the seeded pool whose body field is active."""
    n = VO.CHAINS[which][1]
    r = reference(which, "along_links", 130)
    q0 = torch.from_numpy(r["q"][r["f"] > 0.2][:B])
    assert q0.shape[0] == B
    gen = torch.Generator().manual_seed(seed)
    steps = 0.04 * torch.randn(B, T, n, generator=gen, dtype=torch.float64)
    steps[:, 0] = 0
    x = torch.zeros(B, T, 2 * n, dtype=torch.float64)
    x[..., :n] = q0[:, None] + steps.cumsum(1)
    return x


@pytest.mark.parametrize("which,beside", [("toy", None), ("panda", None), ("panda", "spheres")])
@pytest.mark.parametrize("dtype", DTYPES)
def test_sweep_adds_k_times_the_sum_of_the_field(dtype, which, beside):
    """sgpmp_cost_eval of GP + body (+ a SPHERES term: the generated-chain sweep followed by the body launch) against the program
    without the body term plus the oracle's term; costs and costs64; one waypoint, a wave minus one, a wave, one over, two trips."""
    from stoch_gpmp_amd import _lib as L
    from stoch_gpmp_amd.engine import Engine
    from tests import scenarios as SC
    f64 = dtype == torch.float64
    chain, n, _ = VO.CHAINS[which]
    body = bodies(which)["along_links"]
    sc = scene()
    fld = make_field(dtype, body)
    gp = dict(kind=L.COST_GP, flags=0, sigma=10., dt=0.05)
    rest = [gp]
    sph = None
    if beside == "spheres":
        rest = [gp, dict(kind=L.COST_SPHERES, flags=L.FIELD_RBF, sigma=2.0)]
        sph = torch.as_tensor(SC.panda_spheres()).to(**TA(dtype)).contiguous()
    worst = 0.
    for T in (2, 64, 65, 66, 130):
        for B in (1, 5):
            x = sweep_trajs(which, T, B, seed=T).to(dtype)
            xd = x.to(DEV).contiguous()
            out = []
            for descs in (rest + [fld.descriptor(SWEEP_SIGMA)], rest):
                eng = Engine(n, T, 0, 1, tensor_args=TA(dtype))
                eng.set_fk(device_chain(which), codegen=False)
                eng.set_costs(descs)
                c, c64 = torch.empty(B, **TA(dtype)), torch.empty(B, device=DEV, dtype=torch.float64)
                eng.cost_eval(xd, spheres=sph, out=c, out64=c64)
                if len(descs) > len(rest):
                    c2, c64b = torch.empty_like(c), torch.empty_like(c64)
                    eng.cost_eval(xd, spheres=sph, out=c2, out64=c64b)
                    assert torch.equal(c, c2) and torch.equal(c64, c64b)             # two calls: the same bits
                    name = eng.last_cost_kernel()
                    assert name.startswith("cost_sweep_kernel") and name.endswith(" + body_cost_kernel"), name
                    assert ("generated chain" in name) == (beside == "spheres"), name
                out.append((c.cpu().double().numpy(), c64.cpu().numpy()))
            add = BO.sweep_term(x.double(), n, chain, body, sc, SWEEP_SIGMA).numpy()
            for k in (0, 1):
                ref = out[1][k] + add
                assert float(add.min()) > 0 and float((add / ref).min()) > 0.3    # the term is there, and no rounding error of the rest
                worst = max(worst, float((np.abs(out[0][k] - ref) / np.abs(ref)).max()))
    print(f"    {dtype} {which} beside {beside}: worst relative error of a cost {worst:.3e}")
    assert worst <= (1e-12 if f64 else FP32_SWEEP_RTOL), worst


# ------------------------------------------------------------------------------------------------ 4. the step
@pytest.mark.parametrize("dtype", DTYPES)
def test_step_is_sampler_sweep_body_launch_update_bit_for_bit(dtype):
    from stoch_gpmp_amd import _lib as L
    body = bodies("panda")["along_links"]
    fld = make_field(dtype, body)
    p, q = arm_planner(dtype, fld), arm_planner(dtype, fld)
    assert torch.equal(p.particle_means, q.particle_means)
    costs, grad = p.step()
    name = p._engine.last_cost_kernel()
    assert "fused" not in name and name.startswith("cost_sweep_kernel") and name.endswith(" + body_cost_kernel"), name
    # the voxel point term's step (sampler + generic sweep + update) plus ONE launch, body_cost_kernel; no store-free step
    from tests.test_gpu_voxel_sdf import make_field as make_point_field
    v = arm_planner(dtype, make_point_field(dtype))
    v.step()
    assert p._engine.last_step_launches() == v._engine.last_step_launches() + 1 and p._engine.store_free_steps() == 0
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
    assert q.cost.descriptors()[-1]["kind"] == L.COST_BODY_SDF
    # optimize(opt_iters=3) equals three steps
    a, b = arm_planner(dtype, fld, seed=9), arm_planner(dtype, fld, seed=9)
    a.optimize(opt_iters=3)
    for _ in range(3):
        b.step()
    assert torch.equal(a.particle_means, b.particle_means)
    assert a._engine.store_free_steps() == 0 and a._engine.last_cost_kernel().endswith(" + body_cost_kernel")


# ------------------------------------------------------------------------------------------------ 5. GPMP
@pytest.mark.parametrize("n_sub", [0, 2])
@pytest.mark.parametrize("T,P,iters", [(8, 2, 3), (2, 1, 1)])
def test_gpmp_rows_match_the_oracle(T, P, iters, n_sub):
    sc = scene()
    body = bodies("panda")["along_links"]
    means = VO.gpmp_means(T, P)
    fn = BO.gpmp_systems_fn(sc, body, n_sub=n_sub)
    want = DO.field_dense_diag(fn(means))
    pl = arm_gpmp(means, torch.float64, 1e-2, True, n_sub, make_field(torch.float64, body))
    diag = torch.zeros(T * 14, device=DEV, dtype=torch.float64)
    pl._engine.gpmp_linearize(pl.particle_means, diag_sum=diag)
    assert float(want.abs().max()) > 0 and rel_err(diag, want) < 1e-9
    ora = GP.OracleGPMP(means, fn, 0.5, 5.0, False, SOLVE)
    ora0 = GP.OracleGPMP(means, BO.gpmp_systems_fn(sc, body, n_sub=n_sub, field=False), 0.5, 5.0, False, SOLVE)
    pl = arm_gpmp(means, torch.float64, 5.0, False, n_sub, make_field(torch.float64, body))
    d0, _ = ora0.step()
    for it in range(iters):
        d_o, c_o = ora.step()
        if it == 0:
            moved = DO.rel_l2(d0, d_o)
            print(f"    T={T} P={P} n_sub={n_sub}: the body rows move d_theta by {moved:.3f} (relative L2)")
            assert moved >= 0.05, moved
        _, _, costs = pl.optimize()
        assert pl._engine.last_gpmp_kernel() == ("gpmp_thomas_kernel" if n_sub == 0 else "gpmp_dense_solve_kernel")
        e = (rel_err(pl._d_theta, d_o), rel_err(costs, c_o), rel_err(pl.particle_means, ora.particle_means))
        print(f"      iteration {it}: d_theta {e[0]:.2e} costs {e[1]:.2e} means {e[2]:.2e}")
        assert e[0] < 1e-7 and e[1] < 1e-9 and e[2] < 1e-8, (it, e)


def test_gpmp_fp32_one_iteration():
    T, P = 8, 2
    sc = scene()
    body = bodies("panda")["along_links"]
    means = VO.gpmp_means(T, P)
    for k in (0, 2):
        ora = GP.OracleGPMP(means, BO.gpmp_systems_fn(sc, body, n_sub=k), 0.5, 5.0, False, SOLVE)
        _, c_o = ora.step()
        pl = arm_gpmp(means, torch.float32, 5.0, False, k, make_field(torch.float32, body))
        _, _, costs = pl.optimize()
        e = (rel_err(costs, c_o), rel_err(pl.particle_means, ora.particle_means))
        print(f"    fp32 GPMP n_sub={k}: costs {e[0]:.3e} means {e[1]:.3e} (relative, against the fp64 oracle)")
        assert e[0] < 1e-4 and e[1] < 1e-4, e


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals():
    from stoch_gpmp_amd import _lib as L
    from stoch_gpmp_amd.engine import Engine
    from stoch_gpmp_amd.robots.body import BodySpheres
    dtype = torch.float64
    ta = TA(dtype)
    body = bodies("panda")["along_links"]
    fld = make_field(dtype, body)
    T = 6
    gp = dict(kind=L.COST_GP, flags=0, sigma=1., dt=0.1)
    xd = VO.gpmp_means(T, 3).to(**ta).contiguous()
    c64 = torch.empty(3, device=DEV, dtype=torch.float64)
    bare_desc = {k: v for k, v in fld.descriptor(0.05).items() if k != "body"}
    # the term without a body: SGPMP_ESTATE naming sgpmp_set_body, whatever the call order
    eng = Engine(7, T, 1, 1, tensor_args=ta)
    eng.set_fk(device_chain("panda"), codegen=False)
    eng.set_costs([gp, bare_desc])
    with pytest.raises(RuntimeError, match="sgpmp_set_body"):
        eng.cost_eval(xd, out64=c64)
    eng.set_body(body)                                       # after the program: the same context now evaluates
    eng.cost_eval(xd, out64=c64)
    first = c64.clone()
    eng.set_body(None)                                       # cleared
    with pytest.raises(RuntimeError, match="sgpmp_set_body"):
        eng.cost_eval(xd, out64=c64)
    eng.set_body(body)
    eng.set_fk(device_chain("panda"), codegen=False)         # sgpmp_set_fk clears the body
    q = torch.zeros(2, 7, **ta)
    for call in (lambda: eng.cost_eval(xd, out64=c64), lambda: eng.field_grad(1, q), lambda: eng.gpmp_linearize(xd[:1].contiguous())):
        with pytest.raises(RuntimeError, match="sgpmp_set_body"):
            call()
    eng.set_costs([gp, fld.descriptor(0.05)])                # Engine.set_costs hands the descriptor's body over itself
    assert torch.equal(eng.cost_eval(xd, out64=c64), first)
    # the dense-trajectory entry points refuse by name
    with pytest.raises(ValueError, match=r"sgpmp_dense_cost: cost term 1 \(SGPMP_COST_BODY_SDF\)"):
        eng.dense_cost(xd, 2, 0.1, out64=torch.empty(3, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"sgpmp_dense_cost_grad: cost term 1 \(SGPMP_COST_BODY_SDF\)"):
        eng.dense_cost_grad(xd, 2, 0.1)
    with pytest.raises(ValueError, match=r"sgpmp_validate: cost term 1 \(SGPMP_COST_BODY_SDF\)"):
        eng.validate(xd, 2, 0.1)
    pl = arm_planner(dtype, fld, T=8, nppg=1, S=4, dense_cost=dict(n_sub=2, weight=1.0))
    with pytest.raises(ValueError, match="SGPMP_COST_BODY_SDF"):
        pl.step()
    # the query flag beside other terms, and in GPMP
    flagged = fld.descriptor(0.1, distance=True)
    with pytest.raises(ValueError, match="query flag"):
        eng.set_costs([gp, flagged])
    with pytest.raises(ValueError, match="query flag"):
        eng.set_costs([flagged, fld.descriptor(0.1)])
    eng.set_costs([flagged])
    with pytest.raises(ValueError, match="GPMP"):
        eng.gpmp_linearize(VO.gpmp_means(T, 1).to(**ta))
    # bad descriptors and bad bodies
    for edit in (dict(num_interpolate=1), dict(reserved=0), dict(dim0=0), dict(p0=0.), dict(sigma2=-0.1)):
        with pytest.raises(ValueError):
            eng.set_costs([dict(fld.descriptor(0.05), **edit)])
    two = BodySpheres([1], [(0., 0., 0.)], [0.01])
    with pytest.raises(ValueError, match="two different bodies"):
        eng.set_costs([fld.descriptor(0.05), dict(fld.descriptor(0.05), body=two)])
    links = (L.C.c_int32 * 65)(*([0] * 65))
    sph = (L.C.c_double * 260)(*([0.01] * 260))
    call = lambda lk, sp, n: eng.lib.sgpmp_set_body(eng._ctx, lk, sp, n)                         # noqa: E731
    assert call(links, sph, 65) == L.EINVAL and "64" in L.last_error()
    assert call(None, sph, 2) == L.EINVAL and call(links, None, 2) == L.EINVAL and call(links, sph, -1) == L.EINVAL
    assert call((L.C.c_int32 * 3)(0, 2, 1), sph, 3) == L.EINVAL and "non-decreasing" in L.last_error()
    assert call((L.C.c_int32 * 2)(0, 11), sph, 2) == L.EINVAL and "past the chain" in L.last_error()      # the Panda's last frame is 10
    assert call((L.C.c_int32 * 2)(0, 10), sph, 2) == L.OK
    assert call(links, (L.C.c_double * 4)(0., 0., 0., -0.1), 1) == L.EINVAL and "radius" in L.last_error()
    assert call(links, (L.C.c_double * 4)(0., 0., 0., float("inf")), 1) == L.EINVAL
    assert call(links, (L.C.c_double * 4)(0., float("nan"), 0., 0.1), 1) == L.EINVAL and "centre" in L.last_error()
    nochain = Engine(7, T, 1, 1, tensor_args=ta)
    assert nochain.lib.sgpmp_set_body(nochain._ctx, links, sph, 2) == L.ESTATE
    # frames with fewer links than the body reaches
    with pytest.raises(ValueError, match="past the given frames"):
        eng.set_costs([fld.descriptor(0.05)])
        eng.field_eval(0, torch.eye(4, **ta).expand(2, 5, 4, 4).contiguous())


# ------------------------------------------------------------------------------------------------ 7. update()
def test_update_rebuilds_the_volume_and_planners_recompile():
    from stoch_gpmp_amd.envs.voxel_map import VoxelMap
    dtype = torch.float64
    sc = scene()
    body = bodies("panda")["along_links"]
    vm = VoxelMap.from_grid(sc["occ"], sc["cell"], sc["lower"], tensor_args=TA(dtype))
    fld = vm.body_field(body, VO.MARGIN)
    a = arm_planner(dtype, fld, seed=7)
    a.step()
    v0 = fld._version
    vm.occ.zero_()
    vm.add_box((0.3, -0.2, 0.4), (0.25, 0.3, 0.2)).add_sphere((0.1, 0.3, 0.5), 0.12)       # the scene changes
    occ2 = vm.occ.cpu().numpy()
    assert fld.update() is fld.sdf and fld._version == v0 + 1
    assert np.array_equal(fld.sdf.cpu().numpy(), VO.brute_sdf(occ2, sc["cell"]))
    fresh = VoxelMap.from_grid(occ2, sc["cell"], sc["lower"], tensor_args=TA(dtype)).body_field(body, VO.MARGIN)

    def costs_of(field, prev, draw):
        f = arm_planner(dtype, field, seed=7)
        f.particle_means.copy_(prev)
        f._draw = draw
        return f.step()[0]
    prev, draw = a.particle_means.clone(), a._draw
    ca = a.step()[0].clone()
    assert torch.equal(ca, costs_of(fresh, prev, draw))
    assert not torch.equal(ca, costs_of(make_field(dtype, body), prev, draw))
    q = torch.from_numpy(VO.draw_configs("panda", 9, 3)).to(**TA(dtype))
    assert torch.equal(fld.compute_distance(q, device_chain("panda")), fresh.compute_distance(q, device_chain("panda")))


# ------------------------------------------------------------------------------------------------ 8. end to end
def test_gpmp_moves_the_pandas_body_around_a_box_end_to_end():
    """examples/panda_body_gpmp.py: the iteration count was picked on the CPU oracle (OracleGPMP on the example's problem reaches
    a minimum body clearance >= 0 from its second iteration on); the device's plan is held to the same, measured by the oracle."""
    spec = importlib.util.spec_from_file_location("panda_body_gpmp", os.path.join(ROOT, "examples", "panda_body_gpmp.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out, body_field, chain = ex.main(verbose=False)
    vx = ex.scene
    occ = body_field.voxel_map.occ.cpu().numpy()
    sdf = VO.scipy_sdf(occ, vx.CELL)
    assert np.array_equal(body_field.sdf.cpu().numpy(), sdf)
    sc = dict(sdf=sdf, cell=vx.CELL, origin=tuple(-c / vx.CELL for c in vx.LOWER), margin=vx.SETTINGS["margin"])

    def clearance(m):
        frames = fk_all_links(m.double().cpu().reshape(-1, 14)[:, :7], VO.PANDA_CHAIN)
        return float(BO.frames_clearance(frames, ex.body(), sc).min())
    line = clearance(vx.straight_line(vx.SETTINGS["traj_len"], vx.SETTINGS["dt"]))
    got = {k: (clearance(v[0].particle_means), v[2]) for k, v in out.items()}
    print(f"    straight line {line:+.4f}; link-origin plan {got['link origins'][0]:+.4f}; body plan {got['body spheres'][0]:+.4f} "
          f"(device query {got['body spheres'][1]:+.4f})")
    assert line < 0
    for k, (ref, dev) in got.items():
        assert abs(ref - dev) < 1e-9, k                       # the device's query is the oracle's clearance
    assert got["body spheres"][0] >= 0 and got["link origins"][0] < 0
    assert out["body spheres"][1][-1] < out["body spheres"][1][0]
