"""Continuous-time collision and limit cost (sgpmp_dense_cost) on the GPU -- through the C ABI (Engine) and inside the planner --
against a CPU restatement in fp64: the fine states read back from sgpmp_interpolate (the kernel sees the same bits, so the
Hermite rounding is out of the budget), oracle/fk.py, the oracle's fields (oracle/ref_equiv.py) and dense.limit_penalty.
Needs the MI355X: run with `-m gpu`.

Tolerance, everywhere a value is compared: the project's own for link fields (test_gpu_kernels.py:
test_register_fk_path_equals_generic_lds_path_and_oracle), rtol 1e-10 (fp64) / 2e-4 (fp32) with atol = rtol x 1e-2 x the sum of
the ABSOLUTE terms of the trajectory (sdf values cancel)."""
import numpy as np
import pytest
import torch

from oracle import ref_equiv as R
from oracle.fk import PANDA_CHAIN, fk_all_links
from stoch_gpmp_amd import dense
from tests import scenarios as SC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DT = SC.PANDA["dt"]
RTOL = {torch.float64: 1e-10, torch.float32: 2e-4}
EPS = {torch.float64: 2.0 ** -52, torch.float32: 2.0 ** -23}
DTYPES = [torch.float64, torch.float32]
Q_LIM, V_LIM, SIGMA_LIM = ([-2.8] * 7, [2.8] * 7), [2.0] * 7, 0.1
GEN, GENERIC, PLAIN = "generated chain", "generic FK", "no FK"
H = 1.57079632679
ARM6 = [("j1", "revolute", (0.0, 0.0, 0.0), (0.0, 0.0, 0.1625)), ("j2", "revolute", (H, 0.0, 0.0), (0.0, 0.0, 0.0)),
        ("j3", "revolute", (0.0, 0.0, 0.0), (-0.425, 0.0, 0.0)), ("j4", "revolute", (0.0, 0.0, 0.0), (-0.3922, 0.0, 0.1333)),
        ("j5", "revolute", (H, 0.0, 0.0), (0.0, -0.0997, 0.0)), ("j6", "revolute", (-H, 0.0, 0.0), (0.0, 0.0996, 0.0)),
        ("tool", "fixed", (0.0, 0.0, 0.0), (0.0, 0.0, 0.12))]
# seeds picked on the CPU (dense.interpolate in place of the device's fine states) for which no looked-up point lies within
# 1e-4 of a cell boundary / no link point within 1e-4 of a sphere surface; the tests assert it on the device's states
GRID_SEED = {(2, 0): 0, (2, 1): 0, (2, 3): 0, (2, 31): 0, (6, 0): 0, (6, 1): 0, (6, 3): 0, (6, 31): 0,
             (66, 0): 0, (66, 1): 0, (66, 3): 0, (66, 31): 0}
OCC_SEED = 0
GRID_CELL = 8.0


def TA(dtype):
    return {"device": DEV, "dtype": dtype}


def make_engine(n, T, dtype, chain=None, costs=None, generic=False):
    from stoch_gpmp_amd.engine import Engine
    eng = Engine(n, T, 0, 1, tensor_args=TA(dtype))
    if chain is not None:
        eng.set_fk(chain, codegen=False)
    if generic:                                      # (the Panda is recognised whatever `codegen` says: route it by the option)
        eng.set_option("force_generic_fk", 1)
    if costs is not None:
        eng.set_costs(costs)
    return eng


# ------------------------------------------------------------------------------------------- inputs (CPU, seeded)
def arm_inputs(T, dtype, B=33, seed=None, q0=SC.PANDA["start_q"], q1=SC.PANDA["goal_q"]):
    """B trajectories about the start -> goal line: N(0, 0.15) on the positions, N(0, 0.5) on the line's velocity; drawn in fp64,
    rounded to the dtype (host tensor)."""
    g = torch.Generator().manual_seed(1000 + T if seed is None else seed)
    q0, q1 = torch.tensor(q0, dtype=torch.float64), torch.tensor(q1, dtype=torch.float64)
    n = q0.numel()
    w = torch.linspace(0., 1., T, dtype=torch.float64).reshape(1, T, 1)
    q = q0 + (q1 - q0) * w + 0.15 * torch.randn(B, T, n, generator=g, dtype=torch.float64)
    v = (q1 - q0) / ((T - 1) * DT) + 0.5 * torch.randn(B, T, n, generator=g, dtype=torch.float64)
    return torch.cat([q, v], dim=-1).to(dtype).contiguous()


def planar_inputs(T, dtype, seed, B=5, dt=0.02):
    g = torch.Generator().manual_seed(seed)
    w = torch.linspace(0., 1., T, dtype=torch.float64).reshape(1, T, 1)
    a, b = (torch.rand(B, 1, 2, generator=g, dtype=torch.float64) * 32 - 16 for _ in range(2))
    q = a + (b - a) * w + 0.3 * torch.randn(B, T, 2, generator=g, dtype=torch.float64)
    v = (b - a) / ((T - 1) * dt) + 5. * torch.randn(B, T, 2, generator=g, dtype=torch.float64)
    return torch.cat([q, v], dim=-1).to(dtype).contiguous()


def planar_grid():
    rng = np.random.default_rng(5)
    return rng.integers(0, 4, size=(10, 10)).astype(np.float64)


def spheres(seed=0, num=5):
    return torch.as_tensor(SC.panda_spheres(num, seed).reshape(-1, 4))


# ------------------------------------------------------------------------------------------- CPU restatement
def grid_margin(fine_q, cell):
    """Smallest distance (world units) of a looked-up point from a cell boundary."""
    u = np.asarray(fine_q, dtype=np.float64) / cell
    return float((np.abs(u - np.round(u)) * cell).min()) if u.size else float("inf")


def surface_margin(frames, sph, num_interpolate=0):
    """Smallest | |p - c| - r | over the link points (with a term's interpolated points) and the spheres."""
    pts = R._link_points(frames, num_interpolate, (5, 7)).unsqueeze(-2)
    s = sph.double().reshape(1, -1, 4)
    return float((torch.linalg.norm(pts - s[..., :3], dim=-1) - s[..., 3]).abs().min())


def restate(fine, T, k, terms, chain=PANDA_CHAIN, sph=None, weight=1.0, limits=None, ctx_dtype=torch.float64):
    """(dense [B], scale [B], frames) in fp64 from the device's fine states `fine` [B,T_f,2n] (host tensor of the ctx dtype).
    terms: dicts kind='self' (sigma, margin) | 'spheres' (sigma, field_type, clamp, num_interpolate) | 'grid' (sigma, grid, cell,
    offset).  scale = the sum of the absolute terms."""
    B, n = fine.shape[0], fine.shape[-1] // 2
    ins = torch.from_numpy(dense.inserted_indices(T, k))
    total, scale = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    frames = None
    if len(ins) and weight > 0:
        q = fine[:, ins, :n]
        if any(t["kind"] != "grid" for t in terms):
            frames = fk_all_links(q.double().reshape(-1, n), chain=chain).reshape(B, len(ins), -1, 4, 4)
        for t in terms:
            if t["kind"] == "self":
                f = R.field_self(frames, margin=t["margin"], num_interpolate=t.get("num_interpolate", 0))
            elif t["kind"] == "spheres":
                f = R.field_spheres(frames, sph.double(), field_type=t["field_type"], clamp_sdf=t.get("clamp", False),
                                    num_interpolate=t.get("num_interpolate", 0)).double()
            else:                                    # the lookup in the ctx dtype: multiply, then add, each rounded
                f = R.grid_lookup(q[..., :2].to(ctx_dtype), torch.as_tensor(t["grid"]).to(ctx_dtype), t["cell"],
                                  torch.as_tensor(t["offset"]).to(ctx_dtype)).double()
            K = 1. / t["sigma"] ** 2
            total += weight * K * f.sum(1)
            scale += weight * K * f.abs().sum(1)
    if limits is not None:
        lim = torch.from_numpy(dense.limit_penalty(fine.double().numpy(), *limits))
        total += lim
        scale += lim
    return total, scale, frames


def check(got, ref, scale, dtype, what=""):
    got, ref, scale = (np.asarray(torch.as_tensor(v).detach().double().cpu()) for v in (got, ref, scale))
    rtol = RTOL[dtype]
    bound = rtol * np.abs(ref) + rtol * 1e-2 * scale
    err = np.abs(got - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.
    print(f"    {what}: max |got - ref| = {err.max() if err.size else 0.:.3e}, max |ref| = {np.abs(ref).max() if ref.size else 0.:.3e}, "
          f"worst error / bound = {worst:.3e}  (rtol {rtol:.0e})")
    assert np.all(err <= bound), f"{what}: error / bound up to {worst:.3e}"


def panda_terms(field_type="rbf", clamp=False, num_interpolate=0, with_self=True):
    from stoch_gpmp_amd.costs.fields import LinkDistanceField, LinkSelfDistanceField
    c = SC.PANDA
    spec, desc = [], []
    if with_self:
        spec.append(dict(kind="self", sigma=c["sigma_self"], margin=c["self_margin"]))
        desc.append(LinkSelfDistanceField(margin=c["self_margin"]).descriptor(c["sigma_self"]))
    spec.append(dict(kind="spheres", sigma=c["sigma_coll"], field_type=field_type, clamp=clamp, num_interpolate=num_interpolate))
    desc.append(LinkDistanceField(field_type=field_type, clamp_sdf=clamp, num_interpolate=num_interpolate).descriptor(c["sigma_coll"]))
    return spec, desc


# ------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_sub", [0, 1, 3, 31])
@pytest.mark.parametrize("T", [2, 6, 66])
def test_panda_values_match_the_restatement(dtype, T, n_sub):
    """Self + rbf sphere terms on the inserted states, weight 0.7, and the limit penalty on all fine states; T = 66 takes a
    second pass of 64 lanes and the lane-63 neighbour load."""
    spec, desc = panda_terms()
    eng = make_engine(7, T, dtype, chain=PANDA_CHAIN, costs=desc)
    x = arm_inputs(T, dtype)
    xd, sph = x.to(DEV), spheres().to(**TA(dtype))
    lim = (Q_LIM, V_LIM, SIGMA_LIM)
    got = eng.dense_cost(xd, n_sub, DT, spheres=sph, weight=0.7, q_limits=Q_LIM, v_limits=V_LIM, sigma_limit=SIGMA_LIM)
    if n_sub > 0:
        assert GEN in eng.last_dense_kernel()
    fine = eng.interpolate(xd, n_sub, DT).cpu()
    ref, scale, _ = restate(fine, T, n_sub, spec, sph=sph.cpu(), weight=0.7, limits=lim)
    assert float(dense.limit_penalty(fine.double().numpy(), *lim).max()) > 0            # the limits bind somewhere
    check(got, ref, scale, dtype, f"panda T={T} n_sub={n_sub}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_sub", [0, 1, 3, 31])
@pytest.mark.parametrize("T", [2, 6, 66])
def test_planar_grid_values_match_the_restatement(dtype, T, n_sub):
    from stoch_gpmp_amd.envs.obst_map import ObstacleMap
    om = ObstacleMap.from_grid(planar_grid(), GRID_CELL, tensor_args=TA(dtype))
    eng = make_engine(2, T, dtype, costs=[om.descriptor(0.5)])
    x = planar_inputs(T, dtype, GRID_SEED[(T, n_sub)])
    xd = x.to(DEV)
    got = eng.dense_cost(xd, n_sub, 0.02)
    assert PLAIN in eng.last_dense_kernel()
    fine = eng.interpolate(xd, n_sub, 0.02).cpu()
    ins = dense.inserted_indices(T, n_sub)
    margin = grid_margin(fine[:, ins, :2].double().numpy(), GRID_CELL)
    print(f"    closest cell boundary: {margin:.3e}")
    assert margin > 1e-4
    spec = [dict(kind="grid", sigma=0.5, grid=planar_grid(), cell=GRID_CELL, offset=[om.origin_xi, om.origin_yi])]
    ref, scale, _ = restate(fine, T, n_sub, spec, ctx_dtype=dtype)
    if n_sub > 0:
        assert float(ref.max()) > 0
    else:
        assert torch.all(got == 0)
    check(got, ref, scale, dtype, f"planar T={T} n_sub={n_sub}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("field_type,clamp", [("rbf", False), ("sdf", False), ("sdf", True), ("occupancy", False)])
def test_field_types_on_both_code_paths(dtype, field_type, clamp):
    """Every sphere field, the same Panda inputs through the built-in chain code and through the generic LDS path: each names
    its kernel, each matches the restatement, and the two agree."""
    occ = field_type == "occupancy"
    T, n_sub = 6, (1 if occ else 3)
    spec, desc = panda_terms(field_type, clamp, with_self=False)        # (the self term's constant part would swamp the spheres)
    x = arm_inputs(T, dtype, seed=OCC_SEED if occ else None)
    xd, sph = x.to(DEV), spheres().to(**TA(dtype))
    fast = make_engine(7, T, dtype, chain=PANDA_CHAIN, costs=desc)
    slow = make_engine(7, T, dtype, chain=PANDA_CHAIN, costs=desc, generic=True)
    a = fast.dense_cost(xd, n_sub, DT, spheres=sph)
    assert GEN in fast.last_dense_kernel()
    b = slow.dense_cost(xd, n_sub, DT, spheres=sph)
    assert GENERIC in slow.last_dense_kernel()
    fine = fast.interpolate(xd, n_sub, DT).cpu()
    ref, scale, frames = restate(fine, T, n_sub, spec, sph=sph.cpu())
    if occ:
        margin = surface_margin(frames, sph.cpu())
        print(f"    closest sphere surface: {margin:.3e}")
        assert margin > 1e-4
        assert float(ref.max()) > 0                                        # some link point is inside a sphere
    check(a, ref, scale, dtype, f"{field_type} built-in")
    check(b, ref, scale, dtype, f"{field_type} generic")
    check(a, b, scale, dtype, f"{field_type} built-in against generic")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("generic", [False, True])
def test_sphere_term_alone_through_the_second_pass(dtype, generic):
    """T = 66 without the self term: the sphere field of the second pass of 64 lanes (and of the lane-63 neighbour load) on its
    own scale, on both kernels."""
    T, n_sub = 66, 3
    spec, desc = panda_terms("rbf", with_self=False)
    eng = make_engine(7, T, dtype, chain=PANDA_CHAIN, costs=desc, generic=generic)
    xd, sph = arm_inputs(T, dtype).to(DEV), spheres().to(**TA(dtype))
    got = eng.dense_cost(xd, n_sub, DT, spheres=sph)
    assert (GENERIC if generic else GEN) in eng.last_dense_kernel()
    fine = eng.interpolate(xd, n_sub, DT).cpu()
    ref, scale, _ = restate(fine, T, n_sub, spec, sph=sph.cpu())
    # the intervals 63 and 64 alone carry a visible share: leaving them out would be well outside the bound
    tail = [dict(spec[0])]
    head, _, _ = restate(fine[:, :63 * (n_sub + 1) + 1], 64, n_sub, tail, sph=sph.cpu())
    assert float(((ref - head) / ref).min()) > 10 * RTOL[dtype]
    check(got, ref, scale, dtype, f"spheres alone, T=66, {'generic' if generic else 'built-in'}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_interpolated_link_points_take_the_generic_kernel(dtype):
    T, n_sub = 6, 3
    spec, desc = panda_terms("rbf", num_interpolate=2, with_self=False)
    eng = make_engine(7, T, dtype, chain=PANDA_CHAIN, costs=desc)
    xd, sph = arm_inputs(T, dtype).to(DEV), spheres().to(**TA(dtype))
    got = eng.dense_cost(xd, n_sub, DT, spheres=sph)
    assert GENERIC in eng.last_dense_kernel()
    ref, scale, _ = restate(eng.interpolate(xd, n_sub, DT).cpu(), T, n_sub, spec, sph=sph.cpu())
    check(got, ref, scale, dtype, "num_interpolate=2")


# distance error the project grants its forward kinematics (tests/test_gpu_dense.py: DIST_TOL, 4 x the FK tolerance)
DIST_ERR = {torch.float64: 4e-12, torch.float32: 8e-6}


@pytest.mark.parametrize("dtype", DTYPES)
def test_self_term_on_both_code_paths(dtype):
    """The Panda self term alone: self_field_cg (host constant + the table of moving pairs) against the generic full L x L sum
    and the oracle.  On these trajectories the field is, to 1e-8, its constant part (diagonal, coincident and rigid pairs: ~25
    per state), so what is compared is that constant, and the project's 2e-4 would be 50 times too loose for it.  Bound here,
    from reasoning: 32 ulps of the whole sum -- the generic path adds L^2 = 121 terms one after the other in the compute type
    (worst case 60 ulps, ~ sqrt(121) typical), then K, the states of a lane and the lanes -- plus, for each moving pair,
    d dd / m^2 of its exp(-d^2 / 2 m^2) for a distance error dd = DIST_ERR."""
    from tests.test_gpu_dense import moving_pairs
    T, n_sub = 6, 3
    spec, desc = panda_terms()
    spec, desc = spec[:1], desc[:1]
    xd = arm_inputs(T, dtype).to(DEV)
    fast = make_engine(7, T, dtype, chain=PANDA_CHAIN, costs=desc)
    slow = make_engine(7, T, dtype, chain=PANDA_CHAIN, costs=desc, generic=True)
    a = fast.dense_cost(xd, n_sub, DT, out64=torch.empty(33, device=DEV, dtype=torch.float64)).cpu()
    assert GEN in fast.last_dense_kernel()
    b = slow.dense_cost(xd, n_sub, DT, out64=torch.empty(33, device=DEV, dtype=torch.float64)).cpu()
    assert GENERIC in slow.last_dense_kernel()
    ref, scale, frames = restate(fast.interpolate(xd, n_sub, DT).cpu(), T, n_sub, spec)
    K, m2 = 1. / spec[0]["sigma"] ** 2, spec[0]["margin"] ** 2
    p = frames[..., :3, 3]
    d = torch.linalg.norm(p.unsqueeze(-2) - p.unsqueeze(-3), dim=-1)
    mask = torch.from_numpy(moving_pairs())
    e = torch.exp(-d * d / (2 * m2)) * mask
    moving = 2 * K * e.sum((1, 2, 3))
    bound = 2 * K * (e * d * DIST_ERR[dtype] / m2).sum((1, 2, 3)) + 32 * EPS[dtype] * scale
    print(f"    self term: whole {float(ref.max()):.4e}, moving part {float(moving.min()):.3e} .. {float(moving.max()):.3e}, "
          f"bound {float(bound.max()):.3e}; |built-in - ref| {float((a - ref).abs().max()):.3e}, "
          f"|generic - ref| {float((b - ref).abs().max()):.3e}, |built-in - generic| {float((a - b).abs().max()):.3e}")
    assert torch.all((a - ref).abs() <= bound) and torch.all((b - ref).abs() <= bound)
    assert torch.all((a - b).abs() <= 2 * bound)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,n_sub", [(2, 0), (66, 0), (66, 3), (66, 31)])
def test_limit_part_alone(dtype, T, n_sub):
    """weight = 0: the limit penalty over ALL fine states on its own scale -- at T = 66 through the second pass of 64 lanes and
    the last waypoint's lane (one state), on both kernels that can carry it."""
    _, desc = panda_terms()
    xd, sph = arm_inputs(T, dtype).to(DEV), spheres().to(**TA(dtype))
    lim = (Q_LIM, V_LIM, SIGMA_LIM)
    bare = make_engine(7, T, dtype)
    eng = make_engine(7, T, dtype, chain=PANDA_CHAIN, costs=desc)
    ref = torch.from_numpy(dense.limit_penalty(bare.interpolate(xd, n_sub, DT).cpu().double().numpy(), *lim))
    assert float(ref.min()) > 0
    kw = dict(q_limits=Q_LIM, v_limits=V_LIM, sigma_limit=SIGMA_LIM)
    check(bare.dense_cost(xd, n_sub, DT, **kw), ref, ref, dtype, f"limits, no program, T={T} n_sub={n_sub}")
    assert PLAIN in bare.last_dense_kernel()
    check(eng.dense_cost(xd, n_sub, DT, spheres=sph, weight=0., **kw), ref, ref, dtype, f"limits, weight 0, T={T} n_sub={n_sub}")
    # only the last waypoint breaks a limit: its lane holds that one state
    y = torch.zeros_like(xd)
    y[:, T - 1, 2] = 3.0
    one = bare.dense_cost(y, n_sub, DT, q_limits=Q_LIM, sigma_limit=1.0)
    last = torch.from_numpy(dense.limit_penalty(bare.interpolate(y, n_sub, DT).cpu().double().numpy(), Q_LIM, None, 1.0))
    assert float(last.min()) >= 0.2 ** 2 * 0.999
    check(one, last, last, dtype, "last waypoint")


@pytest.mark.parametrize("dtype", DTYPES)
def test_six_dof_chain_on_the_generic_path(dtype):
    T, n_sub, n = 6, 3, 6
    spec, desc = panda_terms("rbf")
    eng = make_engine(n, T, dtype, chain=ARM6, costs=desc)
    x = arm_inputs(T, dtype, q0=[0.1, -1.2, 1.4, -0.4, 0.8, 0.2], q1=[0.9, -0.7, 0.9, 0.3, 1.1, -0.4])
    xd = x.to(DEV)
    sph = torch.tensor([[-0.4, 0.1, 0.4, 0.15], [-0.6, -0.2, 0.2, 0.2], [0.2, 0.3, 0.5, 0.1]]).to(**TA(dtype))
    lim = (([-1.0] * n, None), [1.5] * n, 0.2)                           # a lower position limit alone, and a velocity limit
    got = eng.dense_cost(xd, n_sub, DT, spheres=sph, q_limits=lim[0], v_limits=lim[1], sigma_limit=lim[2])
    assert GENERIC in eng.last_dense_kernel()
    fine = eng.interpolate(xd, n_sub, DT).cpu()
    ref, scale, _ = restate(fine, T, n_sub, spec, chain=ARM6, sph=sph.cpu(), limits=lim)
    check(got, ref, scale, dtype, "6-DoF arm")


# ------------------------------------------------------------------------------------------- 3. composition
@pytest.mark.parametrize("dtype", DTYPES)
def test_composition_with_cost_eval(dtype):
    from stoch_gpmp_amd.costs.cost_functions import CostGPTrajectory
    T, B, n_sub = 6, 33, 3
    gp = CostGPTrajectory(7, T, None, DT, dict(sigma_gp=1.), TA(dtype)).descriptors()
    eng = make_engine(7, T, dtype, chain=PANDA_CHAIN, costs=gp + panda_terms()[1])
    xd, sph = arm_inputs(T, dtype).to(DEV), spheres().to(**TA(dtype))
    kw = dict(spheres=sph, q_limits=Q_LIM, v_limits=V_LIM, sigma_limit=SIGMA_LIM)
    c, c64 = torch.empty(B, **TA(dtype)), torch.empty(B, device=DEV, dtype=torch.float64)
    eng.cost_eval(xd, spheres=sph, out=c, out64=c64)
    base, base64 = c.clone(), c64.clone()
    d, d64 = torch.empty(B, **TA(dtype)), torch.empty(B, device=DEV, dtype=torch.float64)
    eng.dense_cost(xd, n_sub, DT, out=d, out64=d64, **kw)
    assert float(d64.min()) > 0
    eng.dense_cost(xd, n_sub, DT, out=c, out64=c64, accumulate=True, **kw)
    assert torch.equal(c64, base64 + d64)                               # one double add
    assert torch.equal(c, c64.to(dtype)) and torch.equal(d, d64.to(dtype))     # the same number, rounded once
    assert torch.all((c.double() - (base.double() + d.double())).abs() <= 2 * EPS[dtype] * c64.abs())
    # each output alone
    only = eng.dense_cost(xd, n_sub, DT, **kw)
    only64 = eng.dense_cost(xd, n_sub, DT, out64=torch.empty_like(d64), **kw)
    assert torch.equal(only, d) and torch.equal(only64, d64)
    acc = base.clone()
    eng.dense_cost(xd, n_sub, DT, out=acc, accumulate=True, **kw)
    assert torch.equal(acc, (base.double() + d64).to(dtype))
    # n_sub = 0 without limits adds exactly 0
    z, z64 = base.clone(), base64.clone()
    eng.dense_cost(xd, 0, DT, spheres=sph, out=z, out64=z64, accumulate=True)
    assert torch.equal(z64, base64) and torch.equal(z, base)
    assert torch.all(eng.dense_cost(xd, 0, DT, spheres=sph) == 0)
    # weight = 0 leaves the limit part
    w0 = eng.dense_cost(xd, n_sub, DT, weight=0., out64=torch.empty_like(d64), **kw)
    fine = eng.interpolate(xd, n_sub, DT).cpu()
    lim = torch.from_numpy(dense.limit_penalty(fine.double().numpy(), Q_LIM, V_LIM, SIGMA_LIM))
    assert float(lim.max()) > 0
    check(w0, lim, lim, dtype, "weight = 0")
    no_lim = eng.dense_cost(xd, n_sub, DT, spheres=sph, out64=torch.empty_like(d64))
    check(d64, no_lim.cpu() + lim, d64.cpu(), dtype, "collision part + limit part")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("generic", [False, True])
def test_non_finite_waypoint_gives_nan_for_that_trajectory_only(dtype, bad, generic):
    T, n_sub, B = 8, 3, 5
    _, desc = panda_terms()
    eng = make_engine(7, T, dtype, chain=PANDA_CHAIN, costs=desc, generic=generic)
    xd, sph = arm_inputs(T, dtype, B=B).to(DEV), spheres().to(**TA(dtype))
    kw = dict(spheres=sph, q_limits=Q_LIM, v_limits=V_LIM, sigma_limit=SIGMA_LIM)
    clean = eng.dense_cost(xd, n_sub, DT, **kw)
    assert torch.all(torch.isfinite(clean))
    for row, t, k in ((1, 0, 3), (3, T - 1, 9), (2, 4, 0)):             # first, last (its lane holds one state), inner waypoint
        y = xd.clone()
        y[row, t, k] = bad
        out = torch.zeros(B, **TA(dtype))
        out64 = torch.zeros(B, device=DEV, dtype=torch.float64)
        eng.dense_cost(y, n_sub, DT, out=out, out64=out64, accumulate=True, **kw)
        keep = torch.arange(B, device=DEV) != row
        assert torch.isnan(out[row]) and torch.isnan(out64[row])
        assert torch.equal(out[keep], clean[keep])
    y = xd.clone()
    y[0, 2, 1] = bad
    assert torch.isnan(eng.dense_cost(y, 0, DT, weight=0.)[0])           # no field, no limit: still NaN


def test_error_codes():
    from stoch_gpmp_amd import _lib as L
    from stoch_gpmp_amd.costs.fields import LinkDistanceField, LinkSelfDistanceField
    dtype, T = torch.float32, 4
    x = arm_inputs(T, dtype, B=3).to(DEV)
    sph = spheres().to(**TA(dtype))
    bare = make_engine(7, T, dtype)
    for kw in (dict(n_sub=-1), dict(n_sub=32), dict(dt=0.), dict(dt=-0.05), dict(dt=float("nan")), dict(weight=-1.),
               dict(v_limits=V_LIM), dict(v_limits=V_LIM, sigma_limit=0.), dict(q_limits=Q_LIM, sigma_limit=-1.),
               dict(q_limits=(Q_LIM[0], None))):
        args = dict(n_sub=1, dt=DT)
        args.update(kw)
        with pytest.raises(ValueError):
            bare.dense_cost(x, **args)
    assert torch.all(bare.dense_cost(x, 31, DT) == 0)                    # no program, no limits: nothing to add
    assert torch.all(bare.dense_cost(x, 1, DT, spheres=sph) == 0)        # spheres are only read by a SPHERES term
    out = torch.empty(3, **TA(dtype))
    lib, ctx, st, null = bare.lib, bare._ctx, L.stream_ptr(), None
    call = lambda ctx, xs, B, o, o64: lib.sgpmp_dense_cost(ctx, xs, B, 1, DT, null, 0, 1.0, null, null, null, 0., 0, o, o64, st)  # noqa: E731
    assert call(ctx, null, 3, L.ptr(out), null) == L.EINVAL
    assert call(ctx, L.ptr(x), 3, null, null) == L.EINVAL
    assert "sgpmp_dense_cost" in L.last_error()
    assert call(null, L.ptr(x), 3, L.ptr(out), null) == L.EINVAL
    assert call(ctx, null, 0, null, null) == L.OK                        # batch 0: a no-op
    assert bare.dense_cost(x[:0].contiguous(), 1, DT).shape == (0,)
    # a link-field term without a chain; a SPHERES term told of spheres it is not given
    for field in (LinkSelfDistanceField(), LinkDistanceField()):
        eng = make_engine(7, T, dtype, costs=[field.descriptor(1.0)])
        with pytest.raises(RuntimeError):
            eng.dense_cost(x, 1, DT, spheres=sph)
    eng = make_engine(7, T, dtype, chain=PANDA_CHAIN, costs=[LinkDistanceField().descriptor(1.0)])
    assert lib.sgpmp_dense_cost(eng._ctx, L.ptr(x), 3, 1, DT, null, 5, 1.0, null, null, null, 0., 0, L.ptr(out), null, st) == L.ESTATE
    assert "sgpmp_dense_cost" in L.last_error()
    assert torch.all(torch.isfinite(eng.dense_cost(x, 1, DT, spheres=sph)))


# ------------------------------------------------------------------------------------------- 4. the point of the feature
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_thin_obstacle_between_two_waypoints_changes_the_ranking(dtype):
    """Straight line A from (-3, 0) to (3, 0), T = 4: its waypoints x = -3, -1, 1, 3 straddle a block |x|, |y| <= 0.4 that the
    waypoint-only cost cannot see; detour B passes at y = 1.5.  cost_eval ranks A below B, cost_eval + dense_cost B below A."""
    from stoch_gpmp_amd.costs.cost_functions import CostGPTrajectory
    from stoch_gpmp_amd.envs.obst_map import ObstacleMap
    T, dt, cell, sigma, val = 4, 0.5, 0.1, 0.01, 3.0
    grid = np.zeros((100, 100))
    om = ObstacleMap.from_grid(grid, cell, tensor_args=TA(dtype))
    ox, oy = int(om.origin_xi), int(om.origin_yi)
    grid[oy - 4:oy + 4, ox - 4:ox + 4] = val                            # world [-0.4, 0.4) x [-0.4, 0.4): 0 -+ a rounding is inside
    om = ObstacleMap.from_grid(grid, cell, tensor_args=TA(dtype))
    xs = torch.tensor([-3., -1., 1., 3.], dtype=torch.float64)
    A = torch.zeros(T, 4, dtype=torch.float64)
    A[:, 0], A[:, 2] = xs, 2. / dt
    Bt = A.clone()
    Bt[1:3, 1] = 1.5
    Bt[0, 3], Bt[3, 3] = 1.5 / dt, -1.5 / dt                            # (zero vertical velocity on the detour's flat part)
    x = torch.stack([A, Bt]).to(dtype).contiguous()
    # the construction, on the CPU with the oracle
    off = torch.tensor([om.origin_xi, om.origin_yi], dtype=torch.float64)
    gt = torch.from_numpy(grid)
    assert torch.all(R.grid_lookup(x[..., :2].double(), gt, cell, off) == 0)              # no support waypoint is in the block
    fine = torch.from_numpy(dense.interpolate(x.double().numpy(), 3, dt))
    ins = dense.inserted_indices(T, 3)
    look = R.grid_lookup(fine[:, ins, :2], gt, cell, off)
    assert look[0].tolist() == [0, 0, 0, 0, val, 0, 0, 0, 0] and torch.all(look[1] == 0)
    xd = x.to(DEV)
    coll = make_engine(2, T, dtype, costs=[om.descriptor(sigma)])
    full = make_engine(2, T, dtype, costs=CostGPTrajectory(2, T, None, dt, dict(sigma_gp=1.), TA(dtype)).descriptors()
                       + [om.descriptor(sigma)])
    assert torch.all(coll.cost_eval(xd) == 0)                            # A's (and B's) collision cost at the waypoints: exactly 0
    c = full.cost_eval(xd, out64=torch.empty(2, device=DEV, dtype=torch.float64))
    assert float(c[0]) < float(c[1])
    d = full.dense_cost(xd, 3, dt, out64=torch.empty(2, device=DEV, dtype=torch.float64))
    # K x the grid values at A's inserted states inside the block, on the device's own states
    fd = full.interpolate(xd, 3, dt)
    inside = coll.grid_lookup(0, fd[0, torch.from_numpy(ins).to(DEV), :2].contiguous()).double()
    assert inside.tolist() == [0, 0, 0, 0, val, 0, 0, 0, 0]
    assert abs(float(d[0]) - float(inside.sum()) / sigma ** 2) <= 4 * EPS[dtype] * val / sigma ** 2
    assert float(d[1]) == 0.
    tot = c + d
    assert float(tot[1]) < float(tot[0])
    print(f"    cost_eval A {float(c[0]):.4g} B {float(c[1]):.4g}; dense A {float(d[0]):.4g} B {float(d[1]):.4g}")


# ------------------------------------------------------------------------------------------- 5. planner
DENSE = dict(n_sub=3, weight=0.5, q_limits=Q_LIM, v_limits=V_LIM, sigma_limit=SIGMA_LIM)


def build_planner(dtype, **kw):
    from stoch_gpmp_amd.workloads import hip_panda_planner
    return hip_panda_planner(SC.PANDA, 16, 4, 8, TA(dtype), seed=21, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
def test_planner_step_is_the_four_calls(dtype):
    from stoch_gpmp_amd import _lib as L
    sph = spheres().to(**TA(dtype))
    p = build_planner(dtype, dense_cost=DENSE)
    q = build_planner(dtype)
    assert torch.equal(p.particle_means, q.particle_means)
    costs, grad = p.step(obstacle_spheres=sph)
    assert len(p._step_calls) == 0 and GEN in p._engine.last_dense_kernel()
    eng, S = q._engine, q.num_samples
    means = q.particle_means
    smp = eng.sample(L.PRIOR_SAMPLE, q.seed, q._draw, means, S, mode_offset=q.p0)
    isw = eng.is_weights(means, q.temperature)
    c, c64 = torch.empty(4, S, **TA(dtype)), torch.empty(4, S, device=DEV, dtype=torch.float64)
    eng.cost_eval(smp, spheres=sph, is_weights=isw, rows_per_particle=S, out=c, out64=c64)
    plain = c64.clone()
    eng.dense_cost(smp, 3, DT, spheres=sph, weight=0.5, q_limits=Q_LIM, v_limits=V_LIM, sigma_limit=SIGMA_LIM, out=c, out64=c64,
                   accumulate=True)
    assert float((c64 - plain).min()) > 0                                 # the term is there
    w, g, mp = torch.empty(4, S, **TA(dtype)), torch.empty_like(means), torch.empty_like(means)
    eng.update(c64, smp, means, q.temperature, q.step_size, weights=w, grad=g, means_prev=mp)
    assert torch.equal(p.state_samples, smp)
    assert torch.equal(costs, c) and torch.equal(p._costs64, c64)
    assert torch.equal(p._weights_buf, w) and torch.equal(grad, g)
    assert torch.equal(p.particle_means, means) and torch.equal(p._means_prev, mp)
    # sample_and_eval includes the term too
    out = p.sample_and_eval(obstacle_spheres=sph)[-1]
    assert out is p._costs
    smp2 = p.state_samples.reshape(-1, 16, 14)
    isw2 = p._engine.is_weights(p.particle_means, p.temperature)
    r64 = torch.empty(4 * S, device=DEV, dtype=torch.float64)
    p._engine.cost_eval(smp2, spheres=sph, is_weights=isw2, rows_per_particle=S, out64=r64)
    d64 = p._engine.dense_cost(smp2, 3, DT, spheres=sph, weight=0.5, q_limits=Q_LIM, v_limits=V_LIM, sigma_limit=SIGMA_LIM,
                               out64=torch.empty_like(r64))
    assert torch.equal(p._costs64.reshape(-1), r64 + d64)


@pytest.mark.parametrize("dtype", DTYPES)
def test_planner_optimize_returns_the_costs_with_the_term(dtype):
    sph = spheres().to(**TA(dtype))
    p = build_planner(dtype, dense_cost=DENSE)
    sp, cp, st, cs, costs, grad = p.optimize(3, obstacle_spheres=sph)
    assert len(p._opt_calls) == 0 and p._engine.multi_iteration_launches() == 0      # the Python loop over step()
    S = p.num_samples
    smp = torch.cat([st, cs], dim=-1).contiguous().reshape(-1, 16, 14)
    prev = torch.cat([sp, cp], dim=-1).contiguous()
    eng = p._engine
    isw = eng.is_weights(prev, p.temperature)
    r64 = eng.cost_eval(smp, spheres=sph, is_weights=isw, rows_per_particle=S, out64=torch.empty(4 * S, device=DEV, dtype=torch.float64))
    d64 = eng.dense_cost(smp, 3, DT, spheres=sph, weight=0.5, q_limits=Q_LIM, v_limits=V_LIM, sigma_limit=SIGMA_LIM,
                         out64=torch.empty(4 * S, device=DEV, dtype=torch.float64))
    assert float(d64.min()) > 0
    ref = (r64 + d64).cpu()
    check(costs.reshape(-1), ref, ref.abs(), dtype, "optimize(3) costs")
    # best_trajectories scores each mean with the term
    best = p.best_trajectories(n_sub=3, obstacle_spheres=sph)
    m = p.particle_means
    s64 = eng.cost_eval(m, spheres=sph, out64=torch.empty(4, device=DEV, dtype=torch.float64)) \
        + eng.dense_cost(m, 3, DT, spheres=sph, weight=0.5, q_limits=Q_LIM, v_limits=V_LIM, sigma_limit=SIGMA_LIM,
                         out64=torch.empty(4, device=DEV, dtype=torch.float64))
    check(best.costs, s64.cpu(), s64.abs().cpu(), dtype, "best_trajectories scores")


def test_planner_without_the_option_is_unchanged():
    import warnings
    dtype = torch.float32
    sph = spheres().to(**TA(dtype))
    a, b = build_planner(dtype), build_planner(dtype, dense_cost=None)
    ra, rb = a.optimize(3, obstacle_spheres=sph), b.optimize(3, obstacle_spheres=sph)
    for u, v in zip(ra, rb):
        assert torch.equal(u, v)
    assert torch.equal(a.particle_means, b.particle_means)
    assert len(b._opt_calls) == 1                                          # the one-call path (sgpmp_optimize)
    # switching on and off on a live planner; the setting travels with the state
    assert b.state_dict()["dense_cost"] is None
    b.set_dense_cost(DENSE)
    b.optimize(1, obstacle_spheres=sph)
    assert len(b._opt_calls) == 1 and GEN in b._engine.last_dense_kernel()
    sd = b.state_dict()
    assert sd["dense_cost"]["n_sub"] == 3 and sd["dense_cost"]["v_limits"] == V_LIM
    with pytest.warns(UserWarning, match="dense_cost"):
        a.load_state_dict(sd)
    b.set_dense_cost(None)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*load_state_dict.*")
        b.load_state_dict(a.state_dict())
    with pytest.raises(ValueError):
        b.set_dense_cost(dict(n_sub=40))
    with pytest.raises(ValueError):
        b.set_dense_cost(dict(v_limits=V_LIM))                             # limits without sigma_limit
    with pytest.raises(ValueError):
        b.set_dense_cost(dict(substeps=2))


def test_foreign_cost_with_the_option_raises():
    from stoch_gpmp_amd.planner import StochGPMP
    ta = TA(torch.float32)

    class Foreign:
        def eval(self, trajs, **observation):
            return trajs[..., 0].sum(-1)
    kw = dict(num_particles_per_goal=2, num_samples=4, traj_len=8, opt_iters=1, dt=0.05, n_dof=2, start_state=torch.zeros(4, **ta),
              multi_goal_states=torch.ones(1, 4, **ta), cost=Foreign(), sigma_start_init=1e-3, sigma_start_sample=1e-3,
              sigma_goal_init=1e-3, sigma_goal_sample=1e-3, sigma_gp_init=1., sigma_gp_sample=1., seed=1, tensor_args=ta)
    with pytest.raises(ValueError, match="dense_cost"):
        StochGPMP(dense_cost=dict(n_sub=2), **kw)
