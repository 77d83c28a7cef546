"""Gradient of the continuous-time collision and limit cost (sgpmp_dense_cost_grad) on the GPU -- through the C ABI (Engine) and as a
differentiable planner call -- against autograd through the oracle.  Needs the MI355X: run with `-m gpu`.

Oracle: the device's own fine states (read back through Engine.interpolate: the kernel sees the same bits, so the Hermite rounding
is out of the budget); in fp64 J = weight x sum K field(FK(q_f)) + limit penalty with oracle/fk.py, the oracle's fields
(oracle/ref_equiv.py) and a torch limit penalty; torch.autograd.grad with respect to the FINE states; dense.hermite_pullback onto
the support states.

Tolerance: gradients take the project's own for field Jacobians (test_gpu_kernels.py:
test_field_jacobian_matches_autograd_through_fk): rtol 1e-9 (fp64) / 3e-4 (fp32), atol = rtol x max |ref| of the trajectory; every
element of every trajectory is compared.  Values take test_gpu_dense_cost.py's `check`, unchanged."""
import numpy as np
import pytest
import torch

from oracle import ref_equiv as R
from oracle.fk import PANDA_CHAIN, fk_all_links
from stoch_gpmp_amd import dense
from tests import scenarios as SC
from tests.test_gpu_dense_cost import (ARM6, DEV, DT, DTYPES, GRID_CELL, Q_LIM, SIGMA_LIM, TA, V_LIM, arm_inputs, check,
                                       make_engine, panda_terms, planar_grid, planar_inputs, spheres)

pytestmark = pytest.mark.gpu

GRAD_RTOL = {torch.float64: 1e-9, torch.float32: 3e-4}
LIM = (Q_LIM, V_LIM, SIGMA_LIM)
# seeds of arm_inputs(B = 5) picked on the CPU (dense.interpolate in place of the device's fine states): the two best (point,
# sphere) pairs of every evaluated state are more than 7e-4 apart and, clamped, both regimes occur with the best unclamped value
# 1e-3 off the clamp; the tests assert 1e-4 on the device's states
SDF_SEED = {("sdf", 0): 15, ("sdf", 2): 173, ("sdf_clamp", 0): 70, ("sdf_clamp", 2): 7}


def torch_limit_penalty(x, q_limits, v_limits, sigma):
    n = x.shape[-1] // 2
    q, v = x[..., :n], x[..., n:]
    out = torch.zeros(x.shape[:-2], dtype=torch.float64)
    q_lo, q_hi = (None, None) if q_limits is None else q_limits
    if q_lo is not None:
        out = out + torch.clamp(torch.as_tensor(q_lo, dtype=torch.float64) - q, min=0.).square().sum((-2, -1))
    if q_hi is not None:
        out = out + torch.clamp(q - torch.as_tensor(q_hi, dtype=torch.float64), min=0.).square().sum((-2, -1))
    if v_limits is not None:
        out = out + torch.clamp(v.abs() - torch.as_tensor(v_limits, dtype=torch.float64), min=0.).square().sum((-2, -1))
    return out / float(sigma) ** 2


def evaluated(T, k, support):
    """Fine indices whose collision terms count: the inserted states, with `support` also the waypoints 1 .. T-1."""
    f = np.arange(dense.fine_length(T, k))
    sel = f % (k + 1) != 0
    if support:
        sel |= (f % (k + 1) == 0) & (f > 0)
    return torch.from_numpy(f[sel])


def field_of(t, frames, sph):
    if t["kind"] == "self":
        return R.field_self(frames, margin=t["margin"], num_interpolate=t.get("num_interpolate", 0))
    return R.field_spheres(frames, sph.double(), field_type=t["field_type"], clamp_sdf=t.get("clamp", False),
                           num_interpolate=t.get("num_interpolate", 0))


def oracle(fine, T, k, terms, chain=PANDA_CHAIN, sph=None, weight=1.0, limits=None, support=False):
    """(J [B], scale [B], grad [B,T,2n], per-state fields) in fp64 from the device's fine states `fine` [B,T_f,2n] (host tensor)."""
    x = fine.double().clone().requires_grad_()
    B, n = x.shape[0], x.shape[-1] // 2
    idx = evaluated(T, k, support)
    total, scale = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    fields = []
    if len(idx) and weight > 0 and terms:
        frames = fk_all_links(x[:, idx, :n].reshape(-1, n), chain=chain).reshape(B, len(idx), -1, 4, 4)
        for t in terms:
            f = field_of(t, frames, sph)
            fields.append(f.detach())
            K = 1. / t["sigma"] ** 2
            total = total + weight * K * f.sum(1)
            scale = scale + (weight * K * f.abs().sum(1)).detach()
    if limits is not None:
        lim = torch_limit_penalty(x, *limits)
        total = total + lim
        scale = scale + lim.detach()
    if total.requires_grad:
        g_fine, = torch.autograd.grad(total.sum(), x)
    else:
        g_fine = torch.zeros_like(x)
    grad = torch.from_numpy(dense.hermite_pullback(g_fine.numpy(), T, k, DT))
    return total.detach(), scale, grad, fields


def check_grad(got, ref, dtype, what=""):
    """|got - ref| <= rtol |ref| + rtol max_b |ref|, every element."""
    got, ref = got.detach().double().cpu().numpy(), torch.as_tensor(ref).double().cpu().numpy()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    rtol = GRAD_RTOL[dtype]
    top = np.abs(ref).reshape(ref.shape[0], -1).max(1).reshape(-1, 1, 1)
    bound = rtol * np.abs(ref) + rtol * top
    err = np.abs(got - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.
    print(f"    {what}: max |got - ref| = {err.max():.3e}, max |ref| = {np.abs(ref).max():.3e}, "
          f"worst error / bound = {worst:.3e}  (rtol {rtol:.0e})")
    assert np.all(np.isfinite(got)), f"{what}: non-finite gradient"
    assert np.all(err <= bound), f"{what}: error / bound up to {worst:.3e}"


# ------------------------------------------------------------------------------------------- 1. Panda, and 6. the value
@pytest.mark.parametrize("support", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_sub", [0, 1, 3, 31])
@pytest.mark.parametrize("T", [2, 6, 64, 65, 66])
def test_panda_gradient_matches_autograd(dtype, T, n_sub, support):
    """Self + rbf sphere terms, weight 0.7, joint and velocity limits that bind.  T = 64 ends on lane 63 with no second pass, 65
    puts the last waypoint alone in a second pass and feeds it lane 63's carry, 66 adds a real interval behind the carry.  Row 0
    and the velocity columns are compared like every other element; the value against the oracle and, without `support`,
    against sgpmp_dense_cost."""
    spec, desc = panda_terms()
    eng = make_engine(7, T, dtype, chain=PANDA_CHAIN, costs=desc)
    B = 33 if T <= 6 else 4
    xd, sph = arm_inputs(T, dtype, B=B).to(DEV), spheres().to(**TA(dtype))
    kw = dict(spheres=sph, weight=0.7, q_limits=Q_LIM, v_limits=V_LIM, sigma_limit=SIGMA_LIM)
    value, grad = eng.dense_cost_grad(xd, n_sub, DT, support=support, **kw)
    assert value.dtype == torch.float64 and value.shape == (B,) and grad.shape == (B, T, 14) and grad.dtype == dtype
    if n_sub > 0 or support:
        assert "dense_cost_grad_kernel" in eng.last_dense_kernel() and "10 joints" in eng.last_dense_kernel()
    fine = eng.interpolate(xd, n_sub, DT).cpu()
    ref, scale, gref, _ = oracle(fine, T, n_sub, spec, sph=sph.cpu(), weight=0.7, limits=LIM, support=support)
    assert float(dense.limit_penalty(fine.double().numpy(), *LIM).max()) > 0            # the limits bind somewhere
    what = f"panda T={T} n_sub={n_sub} support={int(support)}"
    check(value, ref, scale, dtype, what + " value")
    if not support:
        check(value, eng.dense_cost(xd, n_sub, DT, out64=torch.empty(B, device=DEV, dtype=torch.float64), **kw), scale, dtype,
              what + " value against sgpmp_dense_cost")
    check_grad(grad, gref, dtype, what)


# ------------------------------------------------------------------------------------------- 2. sdf, clamped sdf, self with points
def sdf_gap(frames, sph, interp, clamp):
    """Smallest distance between the two best (point, sphere) pairs of a state (exact ties -- link frames that coincide for
    every q -- and, clamped, ties at the clamp value 0 give the same gradient whichever is kept: left out)."""
    pts = R._link_points(frames.reshape(-1, *frames.shape[-3:]), interp, (5, 7)).unsqueeze(-2)
    sd = (sph[:, 3] - torch.linalg.norm(pts - sph[:, :3], dim=-1)).reshape(pts.shape[0], -1)
    if clamp:
        sd = sd.clamp(max=0.)
    gap = sd.max(-1, keepdim=True)[0] - sd
    gap[gap == 0] = float("inf")
    return float(gap.min())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which,interp", [("sdf", 0), ("sdf", 2), ("sdf_clamp", 0), ("sdf_clamp", 2), ("self", 3)])
def test_sdf_and_interpolated_points_on_the_generic_kernel(dtype, which, interp):
    """sdf / clamped sdf with 0 and 2 interpolated link points and the self field with 3, Panda through force_generic_fk.

    The self case stands alone (no limits, no spheres): trajectories that stay clear of themselves have a largest gradient entry
    of ~50 against 3e4 on the others, and the bound is 3e-4 of that -- the case that needs the kernel's double-precision force
    sums (fp32 sums of the equal and opposite pair forces, ~1e5 each, left 1.85 x the bound; now 0.09)."""
    from stoch_gpmp_amd.costs.fields import LinkSelfDistanceField
    T, n_sub = 6, 3
    c = SC.PANDA
    sph = spheres().double()
    if which == "self":
        spec = [dict(kind="self", sigma=c["sigma_self"], margin=0.08, num_interpolate=interp)]
        desc = [LinkSelfDistanceField(margin=0.08, num_interpolate=interp).descriptor(c["sigma_self"])]
        seed = None
    else:
        clamp = which == "sdf_clamp"
        if clamp:
            sph[:, 3] *= 1.6                                   # big spheres: the clamp really bites for some states
        spec, desc = panda_terms("sdf", clamp=clamp, num_interpolate=interp, with_self=False)
        seed = SDF_SEED[(which, interp)]
    eng = make_engine(7, T, dtype, chain=PANDA_CHAIN, costs=desc, generic=True)
    xd, sphd = arm_inputs(T, dtype, B=5, seed=seed).to(DEV), sph.to(**TA(dtype))
    value, grad = eng.dense_cost_grad(xd, n_sub, DT, spheres=sphd, weight=0.7, support=True)
    assert "generic" in eng.last_dense_kernel()
    fine = eng.interpolate(xd, n_sub, DT).cpu()
    ref, scale, gref, fields = oracle(fine, T, n_sub, spec, sph=sphd.cpu(), weight=0.7, support=True)
    if which != "self":
        idx = evaluated(T, n_sub, True)
        frames = fk_all_links(fine[:, idx, :7].double().reshape(-1, 7))
        gap = sdf_gap(frames, sphd.cpu().double(), interp, which == "sdf_clamp")
        print(f"    two best (point, sphere) pairs: at least {gap:.3e} apart")
        assert gap > 1e-4
        if which == "sdf_clamp":                               # the case is only a test if both regimes occur
            assert bool((fields[0] == 0).any()) and bool((fields[0] < 0).any())
    assert float(gref.abs().max()) > 0
    check(value, ref, scale, dtype, f"{which} interp={interp} value")
    check_grad(grad, gref, dtype, f"{which} interp={interp}")


# ------------------------------------------------------------------------------------------- 3. a non-Panda chain
@pytest.mark.parametrize("support", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_sub", [1, 3])
def test_six_dof_chain(dtype, n_sub, support):
    T, n = 6, 6
    spec, desc = panda_terms("rbf")
    eng = make_engine(n, T, dtype, chain=ARM6, costs=desc)
    xd = arm_inputs(T, dtype, q0=[0.1, -1.2, 1.4, -0.4, 0.8, 0.2], q1=[0.9, -0.7, 0.9, 0.3, 1.1, -0.4]).to(DEV)
    sph = torch.tensor([[-0.4, 0.1, 0.4, 0.15], [-0.6, -0.2, 0.2, 0.2], [0.2, 0.3, 0.5, 0.1]]).to(**TA(dtype))
    lim = (([-1.0] * n, None), [1.5] * n, 0.2)                           # a lower position limit alone, and a velocity limit
    value, grad = eng.dense_cost_grad(xd, n_sub, DT, spheres=sph, q_limits=lim[0], v_limits=lim[1], sigma_limit=lim[2],
                                      support=support)
    assert "generic" in eng.last_dense_kernel()
    fine = eng.interpolate(xd, n_sub, DT).cpu()
    ref, scale, gref, _ = oracle(fine, T, n_sub, spec, chain=ARM6, sph=sph.cpu(), limits=lim, support=support)
    check(value, ref, scale, dtype, f"6-DoF arm n_sub={n_sub} support={int(support)} value")
    check_grad(grad, gref, dtype, f"6-DoF arm n_sub={n_sub} support={int(support)}")


# ------------------------------------------------------------------------------------------- 4. limits alone
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["lower", "upper", "velocity"])
@pytest.mark.parametrize("T", [2, 66])
def test_limits_alone_on_a_planar_grid_program(dtype, T, which):
    """weight = 0 is always allowed: a program with a GRID term gives its limit gradient, each one-sided limit by itself."""
    from stoch_gpmp_amd.envs.obst_map import ObstacleMap
    n_sub, dt = 3, 0.02
    om = ObstacleMap.from_grid(planar_grid(), GRID_CELL, tensor_args=TA(dtype))
    eng = make_engine(2, T, dtype, costs=[om.descriptor(0.5)])
    xd = planar_inputs(T, dtype, 3).to(DEV)
    q_limits = {"lower": ([-5., -4.], None), "upper": (None, [5., 4.]), "velocity": None}[which]
    v_limits = [10., 12.] if which == "velocity" else None
    value, grad = eng.dense_cost_grad(xd, n_sub, dt, weight=0., q_limits=q_limits, v_limits=v_limits, sigma_limit=0.5)
    assert "no FK" in eng.last_dense_kernel()
    fine = eng.interpolate(xd, n_sub, dt).cpu().double().numpy()
    ref = dense.limit_penalty(fine, q_limits, v_limits, 0.5)
    gref = dense.hermite_pullback(dense.limit_penalty_grad(fine, q_limits, v_limits, 0.5), T, n_sub, dt)
    assert float(ref.max()) > 0                                          # (a trajectory inside the limit: exact zeros, compared too)
    check(value, ref, ref, dtype, f"planar limits {which} T={T} value")
    check_grad(grad, gref, dtype, f"planar limits {which} T={T}")
    with pytest.raises(ValueError, match="grid"):                         # the same call with the grid term switched on
        eng.dense_cost_grad(xd, n_sub, dt, weight=1., q_limits=q_limits, v_limits=v_limits, sigma_limit=0.5)


# ------------------------------------------------------------------------------------------- 5. consistency inside the library
@pytest.mark.parametrize("dtype", DTYPES)
def test_support_waypoints_alone_equal_the_field_jacobians(dtype):
    """n_sub = 0, support, no limits: the position columns of rows 1 .. T-1 are weight x sum K x sgpmp_field_grad at those
    waypoints; the velocity columns and row 0 are exactly 0."""
    T, B, w = 6, 33, 0.7
    spec, desc = panda_terms()
    eng = make_engine(7, T, dtype, chain=PANDA_CHAIN, costs=desc)
    xd, sph = arm_inputs(T, dtype).to(DEV), spheres().to(**TA(dtype))
    value, grad = eng.dense_cost_grad(xd, 0, DT, spheres=sph, weight=w, support=True)
    q = xd[:, 1:, :7].contiguous().reshape(-1, 7)
    ref, vref = torch.zeros(B, T, 14, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    for ti, t in enumerate(spec):
        f, g = eng.field_grad(ti, q, spheres=sph)
        K = 1. / t["sigma"] ** 2
        ref[:, 1:, :7] += w * K * g.double().cpu().reshape(B, T - 1, 7)
        vref += w * K * f.double().cpu().reshape(B, T - 1).sum(1)
    assert torch.all(grad[:, 0] == 0) and torch.all(grad[:, :, 7:] == 0)
    assert float(ref.abs().max()) > 0
    check_grad(grad, ref, dtype, "support waypoints against sgpmp_field_grad")
    check(value, vref, vref.abs(), dtype, "support waypoints value against sgpmp_field_grad")


# ------------------------------------------------------------------------------------------- 7. accumulate, determinism
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [6, 66])
def test_accumulate_and_identical_bits(dtype, T):
    _, desc = panda_terms()
    eng = make_engine(7, T, dtype, chain=PANDA_CHAIN, costs=desc)
    B = 5
    xd, sph = arm_inputs(T, dtype, B=B).to(DEV), spheres().to(**TA(dtype))
    kw = dict(spheres=sph, weight=0.7, q_limits=Q_LIM, v_limits=V_LIM, sigma_limit=SIGMA_LIM, support=True)
    v1, g1 = eng.dense_cost_grad(xd, 3, DT, **kw)
    v2, g2 = eng.dense_cost_grad(xd, 3, DT, **kw)
    assert torch.equal(v1, v2) and torch.equal(g1, g2)
    gen = torch.Generator().manual_seed(5)
    base = (torch.randn(B, T, 14, generator=gen, dtype=torch.float64) * float(g1.abs().max())).to(dtype).to(DEV)
    acc = base.clone()
    v3, g3 = eng.dense_cost_grad(xd, 3, DT, grad=acc, accumulate=True, **kw)
    assert g3 is acc and torch.equal(v3, v1)                             # the value is written, never accumulated
    assert torch.equal(acc, base + g1)                                   # one rounding of the add
    with pytest.raises(ValueError):
        eng.dense_cost_grad(xd, 3, DT, accumulate=True, **kw)


# ------------------------------------------------------------------------------------------- 8. refusals and NaN
def test_refusals_and_error_codes():
    from stoch_gpmp_amd import _lib as L
    from stoch_gpmp_amd.costs.fields import LinkDistanceField
    from stoch_gpmp_amd.envs.obst_map import ObstacleMap
    dtype, T = torch.float32, 4
    x = arm_inputs(T, dtype, B=3).to(DEV)
    sph = spheres().to(**TA(dtype))
    om = ObstacleMap.from_grid(planar_grid(), GRID_CELL, tensor_args=TA(dtype))
    planar = make_engine(2, T, dtype, costs=[om.descriptor(0.5)])
    xp = planar_inputs(T, dtype, 3, B=3).to(DEV)
    with pytest.raises(ValueError, match="piecewise constant"):
        planar.dense_cost_grad(xp, 1, 0.02)
    v, g = planar.dense_cost_grad(xp, 0, 0.02)                           # no inserted state: nothing would look the grid up
    assert torch.all(v == 0) and torch.all(g == 0)
    occ = make_engine(7, T, dtype, chain=PANDA_CHAIN, costs=[LinkDistanceField(field_type="occupancy").descriptor(1.0)])
    for kw in (dict(n_sub=1), dict(n_sub=0, support=True)):
        with pytest.raises(ValueError, match="occupancy"):
            occ.dense_cost_grad(x, dt=DT, spheres=sph, **kw)
    v, g = occ.dense_cost_grad(x, 1, DT, spheres=sph, weight=0., q_limits=Q_LIM, sigma_limit=1.0)
    assert torch.all(torch.isfinite(g))
    bare = make_engine(7, T, dtype)
    for kw in (dict(n_sub=-1), dict(n_sub=32), dict(dt=0.), dict(dt=float("nan")), dict(weight=-1.), dict(v_limits=V_LIM),
               dict(q_limits=Q_LIM, sigma_limit=-1.)):
        args = dict(n_sub=1, dt=DT)
        args.update(kw)
        with pytest.raises(ValueError):
            bare.dense_cost_grad(x, **args)
    lib, st, null = bare.lib, L.stream_ptr(), None
    grad, val = torch.empty(3, T, 14, **TA(dtype)), torch.empty(3, device=DEV, dtype=torch.float64)
    call = lambda ctx, xs, B, g: lib.sgpmp_dense_cost_grad(ctx, xs, B, 1, DT, null, 0, 1.0, null, null, null, 0., 0, 0, g,  # noqa: E731
                                                           null, L.ptr(val), st)
    assert call(bare._ctx, L.ptr(x), 3, null) == L.EINVAL                 # a null grad
    assert "sgpmp_dense_cost_grad" in L.last_error()
    assert call(bare._ctx, null, 3, L.ptr(grad)) == L.EINVAL
    assert call(null, L.ptr(x), 3, L.ptr(grad)) == L.EINVAL
    assert call(bare._ctx, null, 0, null) == L.OK                         # batch 0: a no-op
    assert call(bare._ctx, L.ptr(x), 3, L.ptr(grad)) == L.OK              # both values may be left out or given
    assert torch.all(grad == 0) and torch.all(val == 0)
    nochain = make_engine(7, T, dtype, costs=[LinkDistanceField().descriptor(1.0)])
    assert call(nochain._ctx, L.ptr(x), 3, L.ptr(grad)) == L.ESTATE       # SPHERES without a chain


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [8, 66])
@pytest.mark.parametrize("generic", [False, True])
def test_one_nan_poisons_its_trajectory_only(dtype, T, generic):
    n_sub, B = 3, 5
    _, desc = panda_terms()
    eng = make_engine(7, T, dtype, chain=PANDA_CHAIN, costs=desc, generic=generic)
    xd, sph = arm_inputs(T, dtype, B=B).to(DEV), spheres().to(**TA(dtype))
    kw = dict(spheres=sph, q_limits=Q_LIM, v_limits=V_LIM, sigma_limit=SIGMA_LIM, support=True)
    v0, g0 = eng.dense_cost_grad(xd, n_sub, DT, **kw)
    assert torch.all(torch.isfinite(v0)) and torch.all(torch.isfinite(g0))
    for row, t, k in ((1, 0, 3), (3, T - 1, 9), (2, T // 2, 0)):         # first, last (its lane holds one state), inner waypoint
        y = xd.clone()
        y[row, t, k] = float("nan")
        keep = torch.arange(B, device=DEV) != row
        v, g = eng.dense_cost_grad(y, n_sub, DT, **kw)
        assert torch.isnan(v[row]) and torch.all(torch.isnan(g[row]))
        assert torch.equal(v[keep], v0[keep]) and torch.equal(g[keep], g0[keep])
        acc = torch.ones_like(g0)
        eng.dense_cost_grad(y, n_sub, DT, grad=acc, accumulate=True, **kw)
        assert torch.all(torch.isnan(acc[row])) and torch.equal(acc[keep], 1 + g0[keep])


# ------------------------------------------------------------------------------------------- 9. planner
DENSE = dict(n_sub=3, weight=0.5, q_limits=Q_LIM, v_limits=V_LIM, sigma_limit=SIGMA_LIM)


def build_planner(dtype, **kw):
    from stoch_gpmp_amd.workloads import hip_panda_planner
    return hip_panda_planner(SC.PANDA, 16, 4, 8, TA(dtype), seed=21, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
def test_planner_continuous_cost_is_differentiable(dtype):
    sph = spheres().to(**TA(dtype))
    p = build_planner(dtype, dense_cost=DENSE)
    eng = p._engine
    g = torch.Generator().manual_seed(3)
    x = (p.particle_means.cpu().double() + 0.3 * torch.randn(4, 16, 14, generator=g, dtype=torch.float64)).to(dtype).to(DEV)
    vref, gref = eng.dense_cost_grad(x, 3, DT, spheres=sph, weight=0.5, q_limits=Q_LIM, v_limits=V_LIM, sigma_limit=SIGMA_LIM,
                                     support=True)
    assert float(gref.abs().max()) > 0
    # defaults come from the dense_cost= setting
    xr = x.clone().requires_grad_()
    J = p.continuous_cost(xr, obstacle_spheres=sph)
    assert J.shape == (4,) and J.requires_grad and torch.equal(J.detach().double(), vref)
    J.sum().backward()
    assert torch.equal(xr.grad, gref)
    with pytest.raises(RuntimeError):                                    # a second backward raises
        J.sum().backward()
    # per-trajectory upstream weights scale the rows
    w = torch.tensor([0.5, -2.0, 0.0, 3.0], dtype=torch.float64, device=DEV)
    xr2 = x.clone().requires_grad_()
    (p.continuous_cost(xr2, obstacle_spheres=sph).double() * w).sum().backward()
    assert torch.equal(xr2.grad, w.to(dtype)[:, None, None] * gref)
    # explicit arguments override the setting; `support` reaches the call
    xr3 = x.clone().requires_grad_()
    p.continuous_cost(xr3, n_sub=1, weight=0.25, support=False, obstacle_spheres=sph).sum().backward()
    _, g3 = eng.dense_cost_grad(x, 1, DT, spheres=sph, weight=0.25, q_limits=Q_LIM, v_limits=V_LIM, sigma_limit=SIGMA_LIM)
    assert torch.equal(xr3.grad, g3)
    # without requires_grad: a plain evaluation; trajs default to the particle means
    plain = p.continuous_cost(x, obstacle_spheres=sph)
    assert not plain.requires_grad and torch.equal(plain.double(), vref)
    own = p.continuous_cost(obstacle_spheres=sph)
    vm, _ = eng.dense_cost_grad(p.particle_means, 3, DT, spheres=sph, weight=0.5, q_limits=Q_LIM, v_limits=V_LIM,
                                sigma_limit=SIGMA_LIM, support=True)
    assert torch.equal(own.double(), vm)
    # no setting: set_dense_cost's defaults (n_sub 4, weight 1, no limits)
    q = build_planner(dtype)
    vd, _ = q._engine.dense_cost_grad(x, 4, DT, spheres=sph, weight=1.0, support=True)
    assert torch.equal(q.continuous_cost(x, obstacle_spheres=sph).double(), vd)
