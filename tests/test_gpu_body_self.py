"""The body's self-collision term (SGPMP_COST_BODY_SELF, csrc/body_self.hip) on the GPU: the term in sgpmp_field_grad,
sgpmp_field_eval, the sweep (generic sweep + body_self_cost_kernel), the step, GPMP with and without continuous-time factors, the
clearance query and the refusals, against the test-side oracle (tests/body_self_oracle.py: torch fp64, autograd through
oracle/fk.py).  Needs the MI355X: run with `-m gpu`.

The bounds are tests/test_gpu_body_sdf.py's.  fp64: 1e-12 max(1, cap) on field values, cap the largest reference value of the
case, the same times the chain's reach on gradients, 1e-12 relative for the sweep, d_theta 1e-7, costs 1e-9, means 1e-8 for GPMP.
fp32: 3e-4 relative plus 3e-4 of the largest reference value for the field and its Jacobian, 2e-4 for the sweep, 1e-4 for one GPMP
iteration.  Every random case asserts about its own inputs, on the oracle, that each counted pair keeps |margin - s_ij| >= 1e-5 m
and D_ij >= 1e-3 m (tests/test_cpu_body_self.py shows the same on the CPU); no case is left out."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import gpmp_equiv as GP
from oracle.fk import fk_all_links
from tests import body_self_oracle as SO
from tests import gpmp_dense_oracle as DO
from tests import voxel_sdf_oracle as VO
from tests.test_gpu_gpmp_dense import rel_err
from tests.test_gpu_voxel_sdf import FP32_RTOL, FP32_SWEEP_RTOL, SOLVE, TA, arm_gpmp, device_chain

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
DTYPES = [torch.float64, torch.float32]
CASES = ["M=2", "along_links", "M=64", "behind a fixed joint", "link 0 against the last"]
_REF = {}
# a placeholder chain with exactly representable positions: a revolute joint about z at the origin, then a fixed offset of 0.25 along x
PLACEHOLDER = [("j0", "revolute", (0., 0., 0.), (0., 0., 0.)), ("j1", "fixed", (0., 0., 0.), (0.25, 0., 0.))]


def reference(which, name):
    """The oracle's answers for case `name` on the 130 seeded configurations, computed once and shared (the batch sizes are
    prefixes)."""
    key = (which, name)
    if key not in _REF:
        chain = VO.CHAINS[which][0]
        body, rows, margin = SO.cases(which)[name]
        q = VO.draw_configs(which, 130, SO.SEED)
        f, g, smin, gs, s, D = SO.config_field_and_grad(q, chain, body, rows, margin)
        _REF[key] = dict(q=q, f=f, g=g, smin=smin, gs=gs, s=s, D=D)
    return _REF[key]


def make_field(dtype, which="panda", name="along_links", margin=None):
    from stoch_gpmp_amd.costs.fields import BodySelfDistanceField
    body, rows, m = SO.cases(which)[name]
    return BodySelfDistanceField(body, m if margin is None else margin, pairs=rows, tensor_args=TA(dtype))


def reach(chain):
    return float(sum(np.linalg.norm(j[3]) for j in chain))


# ------------------------------------------------------------------------------------------------ 1. field, Jacobian, frames
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("which", ["toy", "panda"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_field_and_gradient_match_the_oracle(dtype, which, name):
    f64 = dtype == torch.float64
    chain = VO.CHAINS[which][0]
    body, rows, margin = SO.cases(which)[name]
    fld = make_field(dtype, which, name)
    r = reference(which, name)
    kink, dmin = SO.conditions(r["s"], r["D"], margin)
    assert kink >= 1e-5 and dmin >= 1e-3, (kink, dmin)                      # the test's own inputs
    cap = float(np.abs(r["f"]).max())
    worst = [0., 0., 0.]
    for B in (1, 63, 64, 65, 130):
        q = torch.from_numpy(r["q"][:B]).to(**TA(dtype)).contiguous()
        fo, go = r["f"][:B], r["g"][:B]
        val, grad = fld.compute_cost_and_grad(q, device_chain(which))
        val2, grad2 = fld.compute_cost_and_grad(q, device_chain(which))
        assert torch.equal(val, val2) and torch.equal(grad, grad2)               # two calls: the same bits
        frames = fk_all_links(torch.from_numpy(r["q"][:B]), chain).to(**TA(dtype)).contiguous()
        on_frames = fld.compute_cost(frames)
        if name == "M=2" and B == 65:                    # frames of more links than a chain may have joints: only the body's links count
            pad = torch.eye(4, **TA(dtype)).expand(B, 20 - frames.shape[1], 4, 4)
            assert torch.equal(fld.compute_cost(torch.cat([frames, pad], 1).contiguous()), on_frames)
        val, grad, on_frames = val.cpu().double().numpy(), grad.cpu().double().numpy(), on_frames.cpu().double().numpy()
        # (the fp32 bounds carry the fp64 bound as well: it is the reference's own error, all there is of a gradient that is
        # analytically zero, where autograd returns rounding noise of 1e-16 and the kernel an exact 0)
        vtol = 1e-12 * max(1., cap)
        gtol = vtol * reach(chain)
        if not f64:
            vtol = vtol + FP32_RTOL * np.abs(fo) + FP32_RTOL * np.abs(fo).max()
            gtol = gtol + FP32_RTOL * np.abs(go) + FP32_RTOL * np.abs(go).max()
        ev, ef, eg = np.abs(val - fo), np.abs(on_frames - fo), np.abs(grad - go)
        worst = [max(worst[0], float(ev.max())), max(worst[1], float(ef.max())), max(worst[2], float(eg.max()))]
        print(f"      B={B}: |value - oracle| {ev.max():.2e}, on frames {ef.max():.2e}, |gradient - autograd| {eg.max():.2e}")
        assert (ev <= vtol).all() and (ef <= vtol).all(), (B, float(ev.max()), float(ef.max()))
        assert (eg <= gtol).all(), (B, float(eg.max()))
        if name == "behind a fixed joint":
            assert np.array_equal(grad, np.zeros_like(grad)) and (val > 0).all()   # exactly zero: no revolute joint between the links
    print(f"    {dtype} {which} {name}: worst |value - oracle| {worst[0]:.2e}, on frames {worst[1]:.2e}, |gradient - autograd| {worst[2]:.2e}")
    assert (r["f"] > 0).any()
    if name != "behind a fixed joint":
        assert (np.abs(r["g"]) > 0).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_seven_joint_chain_takes_the_other_compiled_in_form(dtype):
    """The Panda without its three fixed hand joints: 7 joints with n_dof 7, the second chain length body_self_grad_kernel has
    compiled in (the full Panda takes the first, the toy chain the generic form).  Value, Jacobian and query against the oracle."""
    from stoch_gpmp_amd.costs.fields import BodySelfDistanceField
    from stoch_gpmp_amd.robots.body import BodySpheres
    from stoch_gpmp_amd.robots.panda_chain import PANDA_CHAIN
    f64 = dtype == torch.float64
    arm, oracle_arm, margin = PANDA_CHAIN[:7], VO.PANDA_CHAIN[:7], 0.15
    body = BodySpheres.along_links(oracle_arm, SO.SPACING, SO.RADIUS)
    rows = SO.rows_by_gap(body.links, 2, SO.PANDA_CONSTANT)                    # (no pair at a constant distance)
    qn = VO.draw_configs("panda", 130, SO.SEED)[:65]
    fo, go, so, gso, s, D = SO.config_field_and_grad(qn, oracle_arm, body, rows, margin)
    kink, dmin = SO.conditions(s, D, margin)
    assert kink >= 1e-5 and dmin >= 1e-3, (kink, dmin)                        # the test's own inputs
    fld = BodySelfDistanceField(body, margin, pairs=rows, tensor_args=TA(dtype))
    q = torch.from_numpy(qn).to(**TA(dtype)).contiguous()
    val, grad = fld.compute_cost_and_grad(q, arm)
    smin, gs = fld._query(q, arm)
    val, grad, smin, gs = (t.cpu().double().numpy() for t in (val, grad, smin, gs))
    ok = SO.argmin_gap(s) > 1e-4
    cap = float(np.abs(fo).max())
    if f64:
        vtol = stol = 1e-12 * max(1., cap)
        gtol = gstol = vtol * reach(oracle_arm)
    else:
        vtol, stol = FP32_RTOL * np.abs(fo) + FP32_RTOL * np.abs(fo).max(), FP32_RTOL * np.abs(so) + FP32_RTOL * np.abs(so).max()
        gtol = FP32_RTOL * np.abs(go) + FP32_RTOL * np.abs(go).max()
        gstol = (FP32_RTOL * np.abs(gso) + FP32_RTOL * np.abs(gso).max())[ok]
    print(f"    {dtype}: |value - oracle| {np.abs(val - fo).max():.2e}, Jacobian {np.abs(grad - go).max():.2e}, min clearance "
          f"{np.abs(smin - so).max():.2e}, its gradient {np.abs(gs - gso)[ok].max():.2e} on {int(ok.sum())} of 65")
    assert (fo > 0).any() and (np.abs(go).max(1) > 1e-3).sum() >= 30 and (np.abs(gso).max(1) > 1e-3).sum() >= 30 and ok.sum() >= 30
    assert (np.abs(val - fo) <= vtol).all() and (np.abs(grad - go) <= gtol).all()
    assert (np.abs(smin - so) <= stol).all() and (np.abs(gs - gso)[ok] <= gstol).all()


# ------------------------------------------------------------------------------------------------ 2. exact cases
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_cases_on_a_placeholder_chain(dtype):
    """Sphere A on link 0 at (0.25, 0.5, 0), sphere B at the origin of link 2, which is (0.25, 0, 0) at q = 0: D = 0.5 exactly, and
    B moves along +y, towards A, at 0.25 per radian.  Radii 0.125 each."""
    from stoch_gpmp_amd.costs.fields import BodySelfDistanceField
    from stoch_gpmp_amd.robots.body import BodySpheres
    ta = TA(dtype)
    ab = BodySpheres([0, 2], [(0.25, 0.5, 0.), (0., 0., 0.)], [0.125, 0.125])
    q0 = torch.zeros(3, 1, **ta)
    frames0 = fk_all_links(torch.zeros(3, 1, dtype=torch.float64), PLACEHOLDER).to(**ta).contiguous()

    def both(body, margin, q, frames, rows=(2, 0)):
        fld = BodySelfDistanceField(body, margin, pairs=rows, tensor_args=ta)
        val, grad = fld.compute_cost_and_grad(q, PLACEHOLDER)
        smin, gs = fld._query(q, PLACEHOLDER)
        return val.cpu(), grad.cpu(), fld.compute_cost(frames).cpu(), smin.cpu(), gs.cpu()
    # D exactly at margin + r_i + r_j: 0 and a zero gradient; the clearance and its gradient are those of the pair
    val, grad, onf, smin, gs = both(ab, 0.25, q0, frames0)
    assert torch.equal(val, torch.zeros(3)) and torch.equal(grad, torch.zeros(3, 1)) and torch.equal(onf, torch.zeros(3))
    assert torch.equal(smin.double(), torch.full((3,), 0.25, dtype=torch.float64))
    assert torch.equal(gs.double(), torch.full((3, 1), -0.25, dtype=torch.float64))
    # farther apart than the margin: exactly 0
    val, grad, onf, _, _ = both(ab, 0.125, q0, frames0)
    assert torch.equal(val, torch.zeros(3)) and torch.equal(grad, torch.zeros(3, 1)) and torch.equal(onf, torch.zeros(3))
    # active: h = (0.5 + 0.25) - 0.5, dh/dq = +0.25
    val, grad, onf, _, _ = both(ab, 0.5, q0, frames0)
    assert torch.equal(val.double(), torch.full((3,), 0.25, dtype=torch.float64)) and torch.equal(onf, val)
    assert torch.equal(grad.double(), torch.full((3, 1), 0.25, dtype=torch.float64))
    # D = 0: both spheres at the joint's origin, whatever q: margin + r_i + r_j, a zero gradient, no NaN, also in the query
    zero = BodySpheres([0, 1], [(0., 0., 0.), (0., 0., 0.)], [0.125, 0.25])
    q = torch.tensor([[0.3], [1.1], [-2.]], **ta)
    frames = fk_all_links(q.double().cpu(), PLACEHOLDER).to(**ta).contiguous()
    val, grad, onf, smin, gs = both(zero, 0.5, q, frames)
    assert torch.equal(val.double(), torch.full((3,), 0.875, dtype=torch.float64)) and torch.equal(onf, val)
    assert torch.equal(grad, torch.zeros(3, 1)) and torch.equal(gs, torch.zeros(3, 1))
    assert torch.equal(smin.double(), torch.full((3,), -0.375, dtype=torch.float64))
    # a NaN joint value: NaN everywhere, and only in that row
    qn = torch.tensor([[0.], [float("nan")], [0.]], **ta)
    fn = frames0.clone()
    fn[1, 2, 0, 3] = float("inf")                                           # a non-finite coordinate of B's link frame
    val, grad, onf, smin, gs = both(ab, 0.5, qn, fn)
    for arr in (val, grad, onf, smin, gs):
        assert bool(torch.isnan(arr[1]).all()) and bool(torch.isfinite(arr[[0, 2]]).all())
    # the query's tie: C at (0, 1, 0) of link 2 is (0.25, 1, 0) at q = 0, as far from A as B; the first pair in summation order, (A, B),
    # gives the gradient -0.25 ((A, C) alone gives +0.25)
    abc = BodySpheres([0, 2, 2], [(0.25, 0.5, 0.), (0., 0., 0.), (0., 1., 0.)], [0.125, 0.125, 0.125])
    _, _, _, smin, gs = both(abc, 0.25, q0, frames0, rows=(6, 0, 0))
    assert torch.equal(smin.double(), torch.full((3,), 0.25, dtype=torch.float64))
    assert torch.equal(gs.double(), torch.full((3, 1), -0.25, dtype=torch.float64))
    _, _, _, smin, gs = both(abc, 0.25, q0, frames0, rows=(4, 0, 0))
    assert torch.equal(smin.double(), torch.full((3,), 0.25, dtype=torch.float64))
    assert torch.equal(gs.double(), torch.full((3, 1), 0.25, dtype=torch.float64))


# ------------------------------------------------------------------------------------------------ 3. the query
@pytest.mark.parametrize("which", ["toy", "panda"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_clearance_query_and_collision(dtype, which):
    f64 = dtype == torch.float64
    chain = VO.CHAINS[which][0]
    for name in ("along_links", "M=64"):
        fld = make_field(dtype, which, name)
        r = reference(which, name)
        q = torch.from_numpy(r["q"]).to(**TA(dtype)).contiguous()
        smin, gs = fld._query(q, device_chain(which))
        assert torch.equal(fld.compute_distance(q, device_chain(which)), smin)
        smin, gs = smin.cpu().double().numpy(), gs.cpu().double().numpy()
        vtol = 1e-12 if f64 else FP32_RTOL * np.abs(r["smin"]) + FP32_RTOL * np.abs(r["smin"]).max()
        assert (np.abs(smin - r["smin"]) <= vtol).all()
        ok = SO.argmin_gap(r["s"]) > 1e-4
        # (as above, the fp32 bound carries the fp64 bound: the closest pair of the Panda's along_links body is at a constant
        # distance, so the gradient through it is analytically zero -- rounding noise of 1e-16 from autograd)
        gtol = 1e-12 * reach(chain)
        if not f64:
            gtol = gtol + (FP32_RTOL * np.abs(r["gs"]) + FP32_RTOL * np.abs(r["gs"]).max())[ok]
        print(f"    {dtype} {which} {name}: |min clearance - oracle| {np.abs(smin - r['smin']).max():.2e}, its gradient "
              f"{np.abs(gs - r['gs'])[ok].max():.2e} on {int(ok.sum())} of {len(ok)} configurations")
        assert ok.sum() >= 60 and (np.abs(gs - r["gs"])[ok] <= gtol).all()
    if which == "panda":
        # the same body without the pairs at a constant distance: the closest pair moves, so the gradient through it is the
        # arg-min torque (with them, above, the closest pair is a constant one and the gradient analytically zero)
        body = SO.cases("panda")["along_links"][0]
        rows = SO.rows_by_gap(body.links, 2, SO.PANDA_CONSTANT)
        if "moving" not in _REF:
            _REF["moving"] = SO.config_field_and_grad(reference("panda", "along_links")["q"], chain, body, rows, 0.15)
        _, _, so, gso, s, _ = _REF["moving"]
        from stoch_gpmp_amd.costs.fields import BodySelfDistanceField
        fld = BodySelfDistanceField(body, 0.15, pairs=rows, tensor_args=TA(dtype))
        q = torch.from_numpy(reference("panda", "along_links")["q"]).to(**TA(dtype)).contiguous()
        smin, gs = (t.cpu().double().numpy() for t in fld._query(q, device_chain("panda")))
        ok = SO.argmin_gap(s) > 1e-4
        stol = 1e-12 if f64 else FP32_RTOL * np.abs(so) + FP32_RTOL * np.abs(so).max()
        gtol = 1e-12 * reach(chain) if f64 else (FP32_RTOL * np.abs(gso) + FP32_RTOL * np.abs(gso).max())[ok]
        print(f"    {dtype} panda along_links, moving pairs only: |min clearance - oracle| {np.abs(smin - so).max():.2e}, its gradient "
              f"{np.abs(gs - gso)[ok].max():.2e} on {int(ok.sum())} of {len(ok)} configurations")
        assert ok.sum() >= 60 and (np.abs(gso)[ok].max(1) > 1e-3).sum() >= 60
        assert (np.abs(smin - so) <= stol).all() and (np.abs(gs - gso)[ok] <= gtol).all()
    # compute_collision away from the threshold (the toy chain's along_links body: some configurations overlap, some do not)
    fld = make_field(dtype, "toy", "along_links")
    r = reference("toy", "along_links")
    q = torch.from_numpy(r["q"]).to(**TA(dtype)).contiguous()
    for buffer in (0., 0.05):
        far = np.abs(r["smin"] - buffer) > 1e-3
        hit = fld.compute_collision(q, device_chain("toy"), buffer=buffer).cpu().numpy()
        assert np.array_equal(hit[far], (r["smin"] < buffer)[far]) and hit[far].any() and not hit[far].all()


# ------------------------------------------------------------------------------------------------ 4. the sweep
SWEEP_SIGMA = 0.05


def sweep_trajs(which, T, B, seed):
    """B smooth random walks in joint space from configurations of the seeded pool."""
    n = VO.CHAINS[which][1]
    q0 = torch.from_numpy(VO.draw_configs(which, 130, SO.SEED)[:B])
    gen = torch.Generator().manual_seed(seed)
    steps = 0.04 * torch.randn(B, T, n, generator=gen, dtype=torch.float64)
    steps[:, 0] = 0
    x = torch.zeros(B, T, 2 * n, dtype=torch.float64)
    x[..., :n] = q0[:, None] + steps.cumsum(1)
    return x


@pytest.mark.parametrize("which,beside", [("toy", None), ("panda", None), ("panda", "spheres"), ("panda", "body_sdf")])
@pytest.mark.parametrize("dtype", DTYPES)
def test_sweep_adds_k_times_the_sum_of_the_field(dtype, which, beside):
    """sgpmp_cost_eval of GP + the term (+ a SPHERES term: the generated-chain sweep; + SGPMP_COST_BODY_SDF in the same list:
    body_cost_kernel, then body_self_cost_kernel) against the program without the term plus the oracle's term; costs and costs64;
    one waypoint, a wave minus one, a wave, one over, two trips."""
    from stoch_gpmp_amd import _lib as L
    from stoch_gpmp_amd.engine import Engine
    from tests import scenarios as SC
    f64 = dtype == torch.float64
    chain, n, _ = VO.CHAINS[which]
    body, rows, margin = SO.cases(which)["along_links"]
    fld = make_field(dtype, which)
    gp = dict(kind=L.COST_GP, flags=0, sigma=10., dt=0.05)
    rest, sph = [gp], None
    if beside == "spheres":
        rest = [gp, dict(kind=L.COST_SPHERES, flags=L.FIELD_RBF, sigma=2.0)]
        sph = torch.as_tensor(SC.panda_spheres()).to(**TA(dtype)).contiguous()
    elif beside == "body_sdf":
        from tests.test_gpu_body_sdf import make_field as make_body_field
        rest = [gp, make_body_field(dtype, body).descriptor(SWEEP_SIGMA)]
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
                    assert name.startswith("cost_sweep_kernel") and name.endswith(" + body_self_cost_kernel"), name
                    assert ("generated chain" in name) == (beside == "spheres"), name
                    assert (" + body_cost_kernel + body_self_cost_kernel" in name) == (beside == "body_sdf"), name
                out.append((c.cpu().double().numpy(), c64.cpu().numpy()))
            add = SO.sweep_term(x.double(), n, chain, body, rows, margin, SWEEP_SIGMA).numpy()
            for k in (0, 1):
                ref = out[1][k] + add
                print(f"      T={T} B={B} {'costs64' if k else 'costs'}: the term is {float((add / ref).min()):.2f} of the cost at least")
                assert float(add.min()) > 0 and float((add / ref).min()) > 0.1    # the term is there, and no rounding error of the rest
                worst = max(worst, float((np.abs(out[0][k] - ref) / np.abs(ref)).max()))
    print(f"    {dtype} {which} beside {beside}: worst relative error of a cost {worst:.3e}")
    assert worst <= (1e-12 if f64 else FP32_SWEEP_RTOL), worst


# ------------------------------------------------------------------------------------------------ 5. the step
def arm_planner(dtype, fields, T=16, nppg=2, S=8, seed=31, **kw):
    """tests/test_gpu_voxel_sdf.py's arm_planner with one CostCollision per field."""
    from stoch_gpmp_amd.costs.cost_functions import CostCollision, CostComposite, CostGP, CostGoalPrior
    from stoch_gpmp_amd.planner import StochGPMP
    from stoch_gpmp_amd.robots.panda import DifferentiableFrankaPanda
    c, ta, n = VO.ARM_C, TA(dtype), 7
    start, goals = torch.tensor(c["start_q"] + [0.] * n, **ta), torch.tensor([c["goal_q"] + [0.] * n], **ta)
    fk = DifferentiableFrankaPanda(gripper=False, device=DEV)
    cost = CostComposite(n, T, [
        CostGP(n, T, start, c["dt"], dict(sigma_start=c["cost_sigma_start"], sigma_gp=c["cost_sigma_gp"]), ta),
        CostGoalPrior(n, T, multi_goal_states=goals, num_particles_per_goal=nppg, num_samples=S, sigma_goal_prior=c["sigma_goal_prior"],
                      tensor_args=ta)] + [CostCollision(n, T, field=f, sigma_coll=c["sigma_coll"], tensor_args=ta) for f in fields],
        FK=fk.compute_forward_kinematics_all_links, tensor_args=ta)
    return StochGPMP(num_particles_per_goal=nppg, num_samples=S, traj_len=T, opt_iters=1, dt=c["dt"], n_dof=n, step_size=0.5,
                     temperature=1., start_state=start, multi_goal_states=goals, cost=cost,
                     sigma_start_init=c["sigma_start_init"], sigma_start_sample=c["sigma_start_sample"],
                     sigma_goal_init=c["sigma_goal_init"], sigma_goal_sample=c["sigma_goal_sample"],
                     sigma_gp_init=c["sigma_gp_init"], sigma_gp_sample=c["sigma_gp_sample"], seed=seed, tensor_args=ta, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
def test_step_is_sampler_sweep_self_launch_update_bit_for_bit(dtype):
    from stoch_gpmp_amd import _lib as L
    from tests.test_gpu_body_sdf import make_field as make_body_field
    from tests.test_gpu_voxel_sdf import make_field as make_point_field
    fld = make_field(dtype)
    p, q = arm_planner(dtype, [fld]), arm_planner(dtype, [fld])
    assert torch.equal(p.particle_means, q.particle_means)
    costs, grad = p.step()
    name = p._engine.last_cost_kernel()
    assert "fused" not in name and name.startswith("cost_sweep_kernel") and name.endswith(" + body_self_cost_kernel"), name
    # the voxel point term's step (sampler + generic sweep + update) plus ONE launch, body_self_cost_kernel; with the body term
    # in the list as well, plus two; no store-free step
    v = arm_planner(dtype, [make_point_field(dtype)])
    v.step()
    base = v._engine.last_step_launches()
    assert p._engine.last_step_launches() == base + 1 and p._engine.store_free_steps() == 0
    body_fld = make_body_field(dtype, SO.cases("panda")["along_links"][0])
    two = arm_planner(dtype, [body_fld, fld])
    two.step()
    assert two._engine.last_step_launches() == base + 2 and two._engine.store_free_steps() == 0
    assert two._engine.last_cost_kernel().endswith(" + body_cost_kernel + body_self_cost_kernel")
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
    assert q.cost.descriptors()[-1]["kind"] == L.COST_BODY_SELF
    # optimize(opt_iters=3) equals three steps
    a, b = arm_planner(dtype, [fld], seed=9), arm_planner(dtype, [fld], seed=9)
    a.optimize(opt_iters=3)
    for _ in range(3):
        b.step()
    assert torch.equal(a.particle_means, b.particle_means)
    assert a._engine.store_free_steps() == 0 and a._engine.last_cost_kernel().endswith(" + body_self_cost_kernel")


# ------------------------------------------------------------------------------------------------ 6. GPMP
@pytest.mark.parametrize("n_sub", [0, 2])
@pytest.mark.parametrize("T,P", [(2, 1), (3, 5), (16, 4)])
def test_gpmp_rows_match_the_oracle(T, P, n_sub):
    """The term's rows of sgpmp_gpmp_linearize through what is made of them: the trust-region diagonal, and two Gauss-Newton
    iterations against OracleGPMP.  The rows must move d_theta by 1e-3 (relative L2) at least: ten thousand times the 1e-7 to
    which d_theta is compared, so a linearisation that dropped the rows fails the comparison."""
    body, rows, margin = SO.cases("panda")["along_links"]
    means = VO.gpmp_means(T, P)
    fn = SO.gpmp_systems_fn(body, rows, margin, n_sub=n_sub)
    want = DO.field_dense_diag(fn(means))
    pl = arm_gpmp(means, torch.float64, 1e-2, True, n_sub, make_field(torch.float64))
    diag = torch.zeros(T * 14, device=DEV, dtype=torch.float64)
    pl._engine.gpmp_linearize(pl.particle_means, diag_sum=diag)
    assert float(want.abs().max()) > 0 and rel_err(diag, want) < 1e-9
    ora = GP.OracleGPMP(means, fn, 0.5, 5.0, False, SOLVE)
    ora0 = GP.OracleGPMP(means, SO.gpmp_systems_fn(body, rows, margin, n_sub=n_sub, field=False), 0.5, 5.0, False, SOLVE)
    pl = arm_gpmp(means, torch.float64, 5.0, False, n_sub, make_field(torch.float64))
    d0, _ = ora0.step()
    for it in range(2):
        d_o, c_o = ora.step()
        if it == 0:
            moved = DO.rel_l2(d0, d_o)
            print(f"    T={T} P={P} n_sub={n_sub}: the term's rows move d_theta by {moved:.3f} (relative L2)")
            assert moved >= 1e-3, moved
        _, _, costs = pl.optimize()
        assert pl._engine.last_gpmp_kernel() == ("gpmp_thomas_kernel" if n_sub == 0 else "gpmp_dense_solve_kernel")
        e = (rel_err(pl._d_theta, d_o), rel_err(costs, c_o), rel_err(pl.particle_means, ora.particle_means))
        print(f"      iteration {it}: d_theta {e[0]:.2e} costs {e[1]:.2e} means {e[2]:.2e}")
        assert e[0] < 1e-7 and e[1] < 1e-9 and e[2] < 1e-8, (it, e)


def test_gpmp_fp32_one_iteration():
    T, P = 8, 2
    body, rows, margin = SO.cases("panda")["along_links"]
    means = VO.gpmp_means(T, P)
    for k in (0, 2):
        ora = GP.OracleGPMP(means, SO.gpmp_systems_fn(body, rows, margin, n_sub=k), 0.5, 5.0, False, SOLVE)
        _, c_o = ora.step()
        pl = arm_gpmp(means, torch.float32, 5.0, False, k, make_field(torch.float32))
        _, _, costs = pl.optimize()
        e = (rel_err(costs, c_o), rel_err(pl.particle_means, ora.particle_means))
        print(f"    fp32 GPMP n_sub={k}: costs {e[0]:.3e} means {e[1]:.3e} (relative, against the fp64 oracle)")
        assert e[0] < 1e-4 and e[1] < 1e-4, e


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals():
    from stoch_gpmp_amd import _lib as L
    from stoch_gpmp_amd.engine import Engine
    from stoch_gpmp_amd.robots.body import BodySpheres
    dtype = torch.float64
    ta = TA(dtype)
    body, rows, margin = SO.cases("panda")["along_links"]
    fld = make_field(dtype)
    T = 6
    gp = dict(kind=L.COST_GP, flags=0, sigma=1., dt=0.1)
    xd = VO.gpmp_means(T, 3).to(**ta).contiguous()
    c64 = torch.empty(3, device=DEV, dtype=torch.float64)
    bare_desc = {k: v for k, v in fld.descriptor(0.05).items() if k not in ("body", "body_pairs")}
    q = torch.zeros(2, 7, **ta)
    # the term without a chain, without a body, without pairs: SGPMP_ESTATE naming sgpmp_set_body_pairs, whatever the call order
    eng = Engine(7, T, 1, 1, tensor_args=ta)
    eng.set_costs([gp, bare_desc])
    with pytest.raises(RuntimeError, match="sgpmp_set_body_pairs"):          # no chain
        eng.cost_eval(xd, out64=c64)
    eng.set_fk(device_chain("panda"), codegen=False)
    with pytest.raises(RuntimeError, match="sgpmp_set_body_pairs"):          # no body
        eng.cost_eval(xd, out64=c64)
    eng.set_body(body)
    for call in (lambda: eng.cost_eval(xd, out64=c64), lambda: eng.field_grad(1, q), lambda: eng.gpmp_linearize(xd[:1].contiguous())):
        with pytest.raises(RuntimeError, match="sgpmp_set_body_pairs"):      # no pairs
            call()
    eng.set_body_pairs(rows)                                 # after the program: the same context now evaluates
    eng.cost_eval(xd, out64=c64)
    first = c64.clone()
    eng.set_body_pairs(None)                                 # cleared
    with pytest.raises(RuntimeError, match="sgpmp_set_body_pairs"):
        eng.cost_eval(xd, out64=c64)
    eng.set_body_pairs(rows)
    eng.set_body(body)                                       # sgpmp_set_body clears the pairs
    with pytest.raises(RuntimeError, match="sgpmp_set_body_pairs"):
        eng.cost_eval(xd, out64=c64)
    eng.set_body_pairs(rows)
    eng.set_fk(device_chain("panda"), codegen=False)         # sgpmp_set_fk clears the body and the pairs
    with pytest.raises(RuntimeError, match="sgpmp_set_body_pairs"):
        eng.cost_eval(xd, out64=c64)
    eng.set_costs([gp, fld.descriptor(0.05)])                # Engine.set_costs hands the descriptor's body and pairs over itself
    assert torch.equal(eng.cost_eval(xd, out64=c64), first)
    # the dense-trajectory entry points refuse by name
    with pytest.raises(ValueError, match=r"sgpmp_dense_cost: cost term 1 \(SGPMP_COST_BODY_SELF\)"):
        eng.dense_cost(xd, 2, 0.1, out64=torch.empty(3, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"sgpmp_dense_cost_grad: cost term 1 \(SGPMP_COST_BODY_SELF\)"):
        eng.dense_cost_grad(xd, 2, 0.1)
    with pytest.raises(ValueError, match=r"sgpmp_validate: cost term 1 \(SGPMP_COST_BODY_SELF\)"):
        eng.validate(xd, 2, 0.1)
    pl = arm_planner(dtype, [fld], T=8, nppg=1, S=4, dense_cost=dict(n_sub=2, weight=1.0))
    with pytest.raises(ValueError, match="SGPMP_COST_BODY_SELF"):
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
    # bad descriptors
    for edit in (dict(num_interpolate=1), dict(sigma2=-0.1), dict(sigma2=float("nan")), dict(device_tensor=torch.zeros(4, **ta))):
        with pytest.raises(ValueError):
            eng.set_costs([dict(fld.descriptor(0.05), **edit)])
    two = BodySpheres([1, 4], [(0., 0., 0.)] * 2, [0.01] * 2)
    with pytest.raises(ValueError, match="two different bodies"):
        eng.set_costs([fld.descriptor(0.05), dict(fld.descriptor(0.05), body=two, body_pairs=[2, 0])])
    with pytest.raises(ValueError, match="two different pair tables"):
        eng.set_costs([fld.descriptor(0.05), dict(fld.descriptor(0.05), body_pairs=body.pair_rows(3))])
    # each argument error of sgpmp_set_body_pairs
    M = len(body)
    eng.set_body(body)
    arr = lambda vals: (L.C.c_uint64 * len(vals))(*vals)                                          # noqa: E731
    call = lambda r, n: eng.lib.sgpmp_set_body_pairs(eng._ctx, r, n)                              # noqa: E731
    good = arr(rows)
    assert call(good, M - 1) == L.EINVAL and "sphere count" in L.last_error()
    assert call(good, M + 1) == L.EINVAL and call(good, -1) == L.EINVAL
    assert call(None, M) == L.EINVAL and "null table" in L.last_error()
    assert call(arr([1 << M] + [0] * (M - 1)), M) == L.EINVAL and "j >= n" in L.last_error()
    assert call(arr([1 << 63] + [0] * (M - 1)), M) == L.EINVAL
    one_link = [0] * M
    one_link[0] = 1 << 1                                     # spheres 0 and 1 of along_links are both on link 0
    assert body.links[0] == body.links[1]
    assert call(arr(one_link), M) == L.EINVAL and "one link" in L.last_error()
    assert call(arr([0] * M), M) == L.EINVAL and "no counted pair" in L.last_error()
    low = [(1 << (k + 1)) - 1 for k in range(M)]             # only bits j <= i: not read, so nothing is counted
    assert call(arr(low), M) == L.EINVAL and "no counted pair" in L.last_error()
    assert call(arr([r | low[k] for k, r in enumerate(rows)]), M) == L.OK        # ... and they do no harm beside counted ones
    assert call(good, M) == L.OK and call(good, 0) == L.OK
    nobody = Engine(7, T, 1, 1, tensor_args=ta)
    assert nobody.lib.sgpmp_set_body_pairs(nobody._ctx, good, M) == L.ESTATE
    nobody.set_fk(device_chain("panda"), codegen=False)
    assert nobody.lib.sgpmp_set_body_pairs(nobody._ctx, good, M) == L.ESTATE and "sgpmp_set_body" in L.last_error()
    # frames with fewer links than the body reaches
    with pytest.raises(ValueError, match="past the given frames"):
        eng.set_costs([fld.descriptor(0.05)])
        eng.field_eval(0, torch.eye(4, **ta).expand(2, 5, 4, 4).contiguous())


# ------------------------------------------------------------------------------------------------ 8. update()
def test_update_changes_the_term_and_planners_recompile():
    dtype = torch.float64
    fld = make_field(dtype)
    a = arm_planner(dtype, [fld], seed=7)
    a.step()
    v0 = fld._version
    body, rows, margin = SO.cases("panda")["along_links"]
    fewer = body.pair_rows(min_link_gap=3)
    assert fld.update(margin=0.08, pairs=fewer) is fld and fld._version == v0 + 1 and fld.num_pairs < 119
    from stoch_gpmp_amd.costs.fields import BodySelfDistanceField
    fresh = BodySelfDistanceField(body, 0.08, pairs=fewer, tensor_args=TA(dtype))

    def costs_of(field, prev, draw):
        f = arm_planner(dtype, [field], seed=7)
        f.particle_means.copy_(prev)
        f._draw = draw
        return f.step()[0]
    prev, draw = a.particle_means.clone(), a._draw
    ca = a.step()[0].clone()
    assert torch.equal(ca, costs_of(fresh, prev, draw))
    assert not torch.equal(ca, costs_of(make_field(dtype), prev, draw))
    q = torch.from_numpy(VO.draw_configs("panda", 9, 3)).to(**TA(dtype))
    assert torch.equal(fld.compute_distance(q, device_chain("panda")), fresh.compute_distance(q, device_chain("panda")))
    assert torch.equal(fld.compute_cost_and_grad(q, device_chain("panda"))[0], fresh.compute_cost_and_grad(q, device_chain("panda"))[0])


# ------------------------------------------------------------------------------------------------ 9. end to end
def test_gpmp_keeps_the_pandas_hand_out_of_its_upper_arm_end_to_end():
    """examples/panda_body_self_gpmp.py: the plan with the term has a strictly larger minimum self-clearance over its support
    waypoints than the plan with the body term alone, measured by the oracle; the device's query agrees with the oracle.  No
    absolute threshold.  Both figures go to profiles/r16/body_self.txt (tools/body_self_timing.py prints them)."""
    spec = importlib.util.spec_from_file_location("panda_body_self_gpmp", os.path.join(ROOT, "examples", "panda_body_self_gpmp.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out, self_field, chain = ex.main(verbose=False)
    rows = ex.pair_rows()
    assert list(self_field.pairs) == rows

    def clearance(m):
        frames = fk_all_links(m.double().cpu().reshape(-1, 14)[:, :7], VO.PANDA_CHAIN)
        return float(SO.frames_clearance(frames, ex.body(), rows).min())
    line = clearance(ex.straight_line(ex.SETTINGS["traj_len"], ex.SETTINGS["dt"]))
    got = {k: (clearance(v[0].particle_means), v[2]) for k, v in out.items()}
    print(f"    straight line {line:+.4f}; body term alone {got['body term alone'][0]:+.4f}; body and self terms "
          f"{got['body and self terms'][0]:+.4f} (device query {got['body and self terms'][1]:+.4f})")
    assert line < 0
    for k, (ref, dev) in got.items():
        assert abs(ref - dev) < 1e-9, k                       # the device's query is the oracle's clearance
    assert got["body and self terms"][0] > got["body term alone"][0]
    assert out["body and self terms"][1][-1] < out["body and self terms"][1][0]
