"""Dense (GP-interpolated) trajectories on the GPU -- sgpmp_interpolate / sgpmp_validate through the C ABI (Engine) and the planner
methods on top -- against a CPU restatement: the Hermite formula in numpy fp64, oracle/fk.py, numpy min / max.  Needs the
MI355X: run with `-m gpu`."""
import functools

import numpy as np
import pytest
import torch

from oracle.fk import PANDA_CHAIN, fk_all_links
from tests import scenarios as SC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DT = SC.PANDA["dt"]
ULP = {torch.float64: 2.0 ** -52, torch.float32: 2.0 ** -23}
# 4 x the project's own FK tolerance (test_gpu_kernels.py: test_panda_fk_and_composite_match_reference_fixture): a distance
# takes two positions, and the interpolated q carries its own rounding
DIST_TOL = {torch.float64: dict(atol=4e-12, rtol=4e-12), torch.float32: dict(atol=8e-6, rtol=4e-5)}
Q_LIM, V_LIM = 2.8, 2.0


def TA(dtype):
    return {"device": DEV, "dtype": dtype}


def make_engine(n, T, dtype, chain=None, costs=None):
    from stoch_gpmp_amd.engine import Engine
    eng = Engine(n, T, 0, 1, tensor_args=TA(dtype))
    if chain is not None:
        eng.set_fk(chain, codegen=False)
    if costs is not None:
        eng.set_costs(costs)
    return eng


# ------------------------------------------------------------------------------------------- CPU restatement
def hermite_np(x, k, dt):
    """Cubic Hermite interpolation on (q, v), fp64: x [B,T,2n] -> [B,(T-1)(k+1)+1,2n]; support rows are copies."""
    x = np.asarray(x, dtype=np.float64)
    B, T, d = x.shape
    n, k1 = d // 2, k + 1
    out = np.empty((B, (T - 1) * k1 + 1, d))
    qa, va, qb, vb = x[:, :-1, :n], x[:, :-1, n:], x[:, 1:, :n], x[:, 1:, n:]
    for m in range(k1):
        s = m / k1
        h00, h10, h01, h11 = 2 * s ** 3 - 3 * s ** 2 + 1, s ** 3 - 2 * s ** 2 + s, -2 * s ** 3 + 3 * s ** 2, s ** 3 - s ** 2
        g00, g10, g11 = 6 * s ** 2 - 6 * s, 3 * s ** 2 - 4 * s + 1, 3 * s ** 2 - 2 * s
        with np.errstate(invalid="ignore"):                            # (the non-finite test feeds inf on purpose)
            out[:, m:-1:k1, :n] = h00 * qa + h10 * dt * va + h01 * qb + h11 * dt * vb
            out[:, m:-1:k1, n:] = (g00 * qa - g00 * qb) / dt + g10 * va + g11 * vb
    out[:, 0:-1:k1] = x[:, :-1]
    out[:, -1] = x[:, -1]
    return out


def _inv_ld(A):
    """Gauss-Jordan inverse with partial pivoting in extended precision (numpy's solvers stop at fp64)."""
    m = A.shape[0]
    M = np.concatenate([A.astype(np.longdouble), np.eye(m, dtype=np.longdouble)], axis=1)
    for c in range(m):
        p = c + int(np.argmax(np.abs(M[c:, c])))
        M[[c, p]] = M[[p, c]]
        M[c] = M[c] / M[c, c]
        for r in range(m):
            if r != c:
                M[r] = M[r] - M[r, c] * M[c]
    return M[:, m:]


@functools.lru_cache(maxsize=None)
def gp_weights(n, k, dt):
    """Lambda, Psi [k+1,2n,2n] of the constant-velocity GP by their DEFINITION (dense Phi, Q, a random non-isotropic SPD Q_c
    that must cancel), in extended precision so that the reference's own error (Q(dt) has condition ~ 1/dt^2) stays far
    below the fp64 bound."""
    ld = np.longdouble
    rng = np.random.default_rng(100 * n + k)
    A = rng.normal(size=(n, n))
    Qc = (A @ A.T + n * np.eye(n)).astype(ld)
    I, Z = np.eye(n, dtype=ld), np.zeros((n, n), dtype=ld)
    dt = ld(dt)

    def Phi(t):
        return np.block([[I, t * I], [Z, I]])

    def Q(t):
        return np.block([[t ** 3 / 3 * Qc, t ** 2 / 2 * Qc], [t ** 2 / 2 * Qc, t * Qc]])
    Qi = _inv_ld(Q(dt))
    lam, psi = [], []
    for m in range(k + 1):
        tau = ld(m) / ld(k + 1) * dt
        P = Q(tau) @ Phi(dt - tau).T @ Qi
        lam.append(Phi(tau) - P @ Phi(dt))
        psi.append(P)
    return np.stack(lam), np.stack(psi)


def gp_interpolate(x, k, dt):
    x = np.asarray(x, dtype=np.longdouble)
    B, T, d = x.shape
    lam, psi = gp_weights(d // 2, k, dt)
    out = np.empty((B, (T - 1) * (k + 1) + 1, d), dtype=np.longdouble)
    for m in range(k + 1):
        out[:, m:-1:k + 1] = x[:, :-1] @ lam[m].T + x[:, 1:] @ psi[m].T
    out[:, -1] = x[:, -1]
    return out.astype(np.float64)


@functools.lru_cache(maxsize=None)
def moving_pairs():
    """[L,L] bool: pairs i - j >= 2 whose distance moves with q -- by the spread of the distance over 64 random q (on the Panda
    the rigid group spreads < 1e-12, the moving one > 0.16)."""
    g = torch.Generator().manual_seed(11)
    q = (torch.rand(64, 7, generator=g, dtype=torch.float64) * 2 - 1) * 3.0
    p = fk_all_links(q)[:, :, :3, 3].numpy()
    D = np.linalg.norm(p[:, :, None] - p[:, None], axis=-1)
    spread = D.max(0) - D.min(0)
    L = spread.shape[0]
    low = np.tril(np.ones((L, L), dtype=bool), -2)
    assert not np.any((spread > 1e-9) & (spread < 1e-2) & low)          # the two groups are far apart
    return (spread > 1e-6) & low


def restate(x, k, dt, spheres=None, q_lim=None, v_lim=None):
    """Per fine state: obstacle clearance, self-clearance, limit excess [B,T_f] each (None: inputs absent), fp64."""
    fine = hermite_np(x, k, dt)
    B, Tf, d = fine.shape
    n = d // 2
    p = fk_all_links(torch.from_numpy(fine[..., :n].reshape(-1, n)))[:, :, :3, 3].numpy().reshape(B, Tf, -1, 3)
    obs = None
    if spheres is not None:
        s = np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
        obs = (np.linalg.norm(p[:, :, :, None] - s[None, None, None, :, :3], axis=-1) - s[:, 3]).min(axis=(2, 3))
    D = np.linalg.norm(p[:, :, :, None] - p[:, :, None], axis=-1)
    slf = np.where(moving_pairs(), D, np.inf).min(axis=(2, 3))
    lim = None
    if q_lim is not None or v_lim is not None:
        parts = []
        if q_lim is not None:
            parts += [q_lim[0] - fine[..., :n], fine[..., :n] - q_lim[1]]
        if v_lim is not None:
            parts += [np.abs(fine[..., n:]) - v_lim]
        lim = np.max(np.concatenate(parts, axis=-1), axis=-1)
    return fine, obs, slf, lim


def panda_inputs(T, dtype, B=33):
    """B Panda trajectories about the start -> goal line of workloads.PANDA: N(0, 0.15) on the positions, N(0, 0.5) on the
    line's velocity; the same values for both dtypes (drawn in fp64, rounded to the dtype, handed back in fp64 too)."""
    torch.manual_seed(T)
    c = SC.PANDA
    q0, q1 = torch.tensor(c["start_q"], dtype=torch.float64), torch.tensor(c["goal_q"], dtype=torch.float64)
    w = torch.linspace(0., 1., T, dtype=torch.float64).reshape(1, T, 1)
    q = q0 + (q1 - q0) * w + 0.15 * torch.randn(B, T, 7, dtype=torch.float64)
    v = (q1 - q0) / ((T - 1) * DT) + 0.5 * torch.randn(B, T, 7, dtype=torch.float64)
    x = torch.cat([q, v], dim=-1).to(dtype)
    return x.to(DEV).contiguous(), x.double().numpy()


def assert_close(a, b, atol, rtol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    err = np.abs(a - b) - rtol * np.abs(b)
    print(f"    max |a - b| = {np.abs(a - b).max():.3e}   (atol {atol:.1e}, rtol {rtol:.1e})")
    assert np.all(err <= atol), f"max excess {np.max(err - atol):.3e}"


# ------------------------------------------------------------------------------------------- 1. interpolation
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n,T", [(2, 2), (2, 6), (2, 66), (7, 2), (7, 6), (7, 66)])
def test_interpolation_is_gp_conditioning(dtype, n, T):
    """sgpmp_interpolate against x(tau) = Lambda x_i + Psi x_{i+1} from dense Phi / Q with a random Q_c.  Bounds from rounding:
    eight weights rounded once, one multiply and three fmas per coordinate -> a few ulp of the largest term; 64 ulp of
    (max|q| + dt max|v|) for positions, of (max|q| / dt + max|v|) for velocities (the q-weights of a velocity are O(1 / dt))."""
    B, dt = 5, 0.02 if n == 2 else 0.05
    g = torch.Generator().manual_seed(17 * n + T)
    x = torch.randn(B, T, 2 * n, generator=g, dtype=torch.float64).to(dtype)
    x64 = x.double().numpy()
    eng = make_engine(n, T, dtype)
    xd = x.to(DEV).contiguous()
    mq, mv = np.abs(x64[..., :n]).max(), np.abs(x64[..., n:]).max()
    for k in (0, 1, 3, 31):
        out = eng.interpolate(xd, k, dt)
        assert out.shape == (B, (T - 1) * (k + 1) + 1, 2 * n) and out.dtype == dtype
        assert torch.equal(out[:, ::k + 1], xd)                          # support rows: the input, bit for bit
        if k == 0:
            assert torch.equal(out, xd)
        ref = gp_interpolate(x64, k, dt)
        got = out.double().cpu().numpy()
        ep, ev = np.abs(got[..., :n] - ref[..., :n]).max(), np.abs(got[..., n:] - ref[..., n:]).max()
        bp, bv = 64 * ULP[dtype] * (mq + dt * mv), 64 * ULP[dtype] * (mq / dt + mv)
        print(f"    k={k}: position error {ep:.3e} (bound {bp:.3e}), velocity error {ev:.3e} (bound {bv:.3e})")
        assert ep <= bp and ev <= bv


# ------------------------------------------------------------------------------------------- 2. validation
def check_against_restatement(dtype, vals, where, per_f, tols):
    """vals / where [B,C] of the kernel against per-fine-state references per_f[c] [B,T_f] (sense[c]: 'min' | 'max')."""
    qualified = total = 0
    for c, (ref, sense, tol) in enumerate(zip(per_f, ("min", "min", "max"), tols)):
        r = ref if sense == "min" else -ref
        order = np.sort(r, axis=1)
        best_f = np.argmin(r, axis=1)                                   # first extreme
        gap = order[:, 1] - order[:, 0] if r.shape[1] > 1 else np.full(r.shape[0], np.inf)
        extreme = np.take_along_axis(ref, best_f[:, None], 1)[:, 0]
        print(f"  column {c}:")
        assert_close(vals[:, c], extreme, **tol)
        clear = gap > 1e-4
        qualified += int(clear.sum())
        total += clear.size
        assert np.array_equal(where[clear, c], best_f[clear]), (c, where[clear, c], best_f[clear])
        w = where[~clear, c]
        assert np.all((w >= 0) & (w < ref.shape[1]))
        if w.size:                                                      # near-ties: any index that attains the extreme
            at = np.take_along_axis(ref[~clear], w[:, None].astype(np.int64), 1)[:, 0]
            assert_close(at, extreme[~clear], **tol)
    print(f"  where: {qualified} of {total} (trajectory, column) cases have a gap > 1e-4")
    assert qualified >= 0.9 * total


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("T", [2, 8, 66])
@pytest.mark.parametrize("k", [0, 3])
def test_validation_matches_the_cpu_restatement(dtype, T, k):
    """sgpmp_validate on the Panda (33 trajectories, 5 spheres, limits +-2.8 rad / +-2.0 rad/s) against the restatement.
    Measured maxima of |kernel - restatement| over the twelve cases (MI355X; the test prints them per case):
    fp64 -- clearance 1.9e-16, self-clearance 1.7e-16, limit excess 2.1e-14;
    fp32 -- clearance 1.1e-7, self-clearance 6.6e-8, limit excess 4.5e-6 (the forward kinematics here use the device
    library's sincosf, not the fast hardware sine); all 99 (trajectory, column) cases of every case have a gap > 1e-4."""
    xd, x64 = panda_inputs(T, dtype)
    sph = SC.panda_spheres(5, 0).reshape(-1, 4)
    eng = make_engine(7, T, dtype, chain=PANDA_CHAIN)
    lo, hi, vm = [-Q_LIM] * 7, [Q_LIM] * 7, [V_LIM] * 7
    vals, where = eng.validate(xd, k, DT, spheres=torch.as_tensor(sph).to(**TA(dtype)), q_limits=(lo, hi), v_limits=vm)
    assert vals.shape == (33, 4) and where.shape == (33, 4) and where.dtype == torch.int32
    vals, where = vals.double().cpu().numpy(), where.cpu().numpy()
    _, obs, slf, lim = restate(x64, k, DT, spheres=sph, q_lim=(-Q_LIM, Q_LIM), v_lim=V_LIM)
    vel_bound = 64 * ULP[dtype] * (np.abs(x64[..., :7]).max() / DT + np.abs(x64[..., 7:]).max())
    check_against_restatement(dtype, vals, where, (obs, slf, lim),
                              (DIST_TOL[dtype], DIST_TOL[dtype], dict(atol=vel_bound, rtol=0.)))
    assert np.all(vals[:, 3] == -np.inf) and np.all(where[:, 3] == -1)           # no grid term


# ------------------------------------------------------------------------------------------- 3. composition
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_validation_equals_the_composed_ops(dtype):
    """Columns 0 and 1 against interpolate -> sgpmp_fk -> sgpmp_link_distances(mode 0) -> amin, all on the GPU."""
    T, k = 8, 3
    xd, _ = panda_inputs(T, dtype)
    sph = torch.as_tensor(SC.panda_spheres(5, 0).reshape(-1, 4)).to(**TA(dtype))
    eng = make_engine(7, T, dtype, chain=PANDA_CHAIN)
    vals, where = eng.validate(xd, k, DT, spheres=sph)
    fine = eng.interpolate(xd, k, DT)
    B, Tf = fine.shape[:2]
    frames = eng.fk(fine[..., :7].reshape(-1, 7).contiguous())
    D_obs = eng.link_distances(frames, sph, mode=0).reshape(B, -1)
    D_self = eng.link_distances(frames, None, mode=0).reshape(B, Tf, 11, 11)
    mask = torch.as_tensor(moving_pairs()).to(DEV)
    D_self = torch.where(mask, D_self, torch.full_like(D_self, float("inf")))
    tol = DIST_TOL[dtype]
    print("  column 0:")
    assert_close(vals[:, 0].double().cpu().numpy(), D_obs.amin(dim=1).double().cpu().numpy(), **tol)
    print("  column 1:")
    assert_close(vals[:, 1].double().cpu().numpy(), D_self.reshape(B, -1).amin(dim=1).double().cpu().numpy(), **tol)
    f_obs = D_obs.reshape(B, Tf, -1).amin(dim=2)
    at = torch.gather(f_obs, 1, where[:, :1].long())[:, 0]
    assert_close(at.double().cpu().numpy(), vals[:, 0].double().cpu().numpy(), **tol)
    assert torch.all(torch.isinf(vals[:, 2]) & (vals[:, 2] < 0)) and torch.all(where[:, 2] == -1)   # no limits given


# ------------------------------------------------------------------------------------------- 4. planar grid
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("T", [4, 66])
def test_grid_column_is_the_lookup_of_the_interpolated_points(dtype, T):
    """Column 3 and its index equal max / first argmax of grid_lookup(interpolate(...)) EXACTLY: both entry points evaluate
    the fine states with one device function in one fma order, so the looked-up points are the same bits."""
    from stoch_gpmp_amd.envs.obst_map import ObstacleMap
    n, k, B, dt = 2, 3, 9, 0.02
    rng = np.random.default_rng(5)
    grid = rng.integers(0, 4, size=(20, 20)).astype(np.float64)         # few distinct values: ties test "lowest f"
    om = ObstacleMap.from_grid(grid, 0.5, tensor_args=TA(dtype))
    eng = make_engine(n, T, dtype, costs=[om.descriptor(1.0)])
    g = torch.Generator().manual_seed(T)
    w = torch.linspace(0., 1., T, dtype=torch.float64).reshape(1, T, 1)
    a, b = torch.rand(B, 1, 2, generator=g, dtype=torch.float64) * 8 - 4, torch.rand(B, 1, 2, generator=g, dtype=torch.float64) * 8 - 4
    q = a + (b - a) * w + 0.3 * torch.randn(B, T, 2, generator=g, dtype=torch.float64)
    v = (b - a) / ((T - 1) * dt) + 5. * torch.randn(B, T, 2, generator=g, dtype=torch.float64)
    xd = torch.cat([q, v], dim=-1).to(**TA(dtype)).contiguous()
    vals, where = eng.validate(xd, k, dt, grid_term=0)
    fine = eng.interpolate(xd, k, dt)
    Tf = fine.shape[1]
    occ = eng.grid_lookup(0, fine[..., :2].reshape(-1, 2).contiguous()).reshape(B, Tf)
    best = occ.max(dim=1).values
    first = (occ == best[:, None]).int().argmax(dim=1)                 # first index of the maximum
    assert torch.equal(vals[:, 3], best)
    assert torch.equal(where[:, 3].long(), first)
    assert float(best.min()) >= 1.0 and len(torch.unique(first)) > 1
    assert torch.all(torch.isinf(vals[:, :2]) & (vals[:, :2] > 0)) and torch.all(where[:, :3] == -1)   # no chain, no limits


# ------------------------------------------------------------------------------------------- 5. overshoot
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_hermite_overshoot_between_waypoints_is_seen(dtype):
    """Both waypoints 0.01 inside the upper limit, velocity +1 then -1: the spline peaks at hi + 0.0025 in between
    (h10 dt v_0 + h11 dt v_1 = 2 * 0.125 * 0.05 at s = 1/2) -- invisible to a waypoint-only check."""
    n, T, dt, hi = 2, 2, 0.05, 1.0
    x = torch.zeros(1, T, 2 * n, **TA(dtype))
    x[0, :, 0] = hi - 0.01
    x[0, 0, n], x[0, 1, n] = 1., -1.
    eng = make_engine(n, T, dtype)
    lim = ([-10.] * n, [hi] * n)
    tol = 8 * ULP[dtype]                                              # |q| <= 1: a few roundings of numbers of size 1
    v0, w0 = eng.validate(x, 0, dt, q_limits=lim)
    assert abs(float(v0[0, 2]) + 0.01) <= tol and int(w0[0, 2]) == 0              # tie between f = 0 and f = 1: the lower
    v1, w1 = eng.validate(x, 1, dt, q_limits=lim)
    assert abs(float(v1[0, 2]) - 0.0025) <= tol and int(w1[0, 2]) == 1


# ------------------------------------------------------------------------------------------- 6. NaN
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_trajectory_reports_nan_and_leaves_the_others(dtype, bad):
    T, k = 8, 3
    xd, _ = panda_inputs(T, dtype, B=5)
    sph = torch.as_tensor(SC.panda_spheres(5, 0).reshape(-1, 4)).to(**TA(dtype))
    eng = make_engine(7, T, dtype, chain=PANDA_CHAIN)
    kw = dict(spheres=sph, q_limits=([-Q_LIM] * 7, [Q_LIM] * 7), v_limits=[V_LIM] * 7)
    v_ok, w_ok = eng.validate(xd, k, DT, **kw)
    assert bool(torch.isfinite(v_ok[:, :3]).all())
    for wp, dof in ((5, 2), (0, 9), (7, 0)):
        xb = xd.clone()
        xb[3, wp, dof] = bad
        v, w = eng.validate(xb, k, DT, **kw)
        fine = hermite_np(xb.double().cpu().numpy(), k, DT)
        first = int(np.argmax(~np.isfinite(fine[3]).all(axis=1)))     # (a NaN waypoint also spoils the interval before it)
        assert first == (max(wp - 1, 0) * (k + 1) + 1 if wp > 0 else 0)
        assert bool(torch.isnan(v[3]).all()) and w[3].tolist() == [first] * 4
        keep = [0, 1, 2, 4]
        assert torch.equal(v[keep], v_ok[keep]) and torch.equal(w[keep], w_ok[keep])
    xb = xd.clone()
    xb[3, 5, 2] = bad
    v, w = eng.validate(xb, 0, DT, **kw)                               # k = 0: the waypoint itself
    assert bool(torch.isnan(v[3]).all()) and w[3].tolist() == [5] * 4


# ------------------------------------------------------------------------------------------- 7. statuses
def test_statuses_and_absent_inputs():
    from stoch_gpmp_amd import _lib as L
    dtype, T = torch.float32, 4
    x = torch.randn(3, T, 14, **TA(dtype))
    sph = torch.as_tensor(SC.panda_spheres(5, 0).reshape(-1, 4)).to(**TA(dtype))
    bare = make_engine(7, T, dtype)
    for n_sub, dt in ((-1, DT), (32, DT), (1, 0.), (1, -0.05), (1, float("nan"))):
        with pytest.raises(ValueError):
            bare.validate(x, n_sub, dt)
        with pytest.raises(ValueError):
            bare.interpolate(x, n_sub, dt)
    assert bare.interpolate(x, 31, DT).shape == (3, 3 * 32 + 1, 14)
    with pytest.raises(RuntimeError):                                  # spheres without a chain
        bare.validate(x, 1, DT, spheres=sph)
    with pytest.raises(ValueError):                                    # no cost program at all
        bare.validate(x, 1, DT, grid_term=0)
    with pytest.raises(ValueError):
        bare.validate(x, 1, DT, grid_term=-2)
    out = torch.empty(3, 4, **TA(dtype))
    wh = torch.empty(3, 4, device=DEV, dtype=torch.int32)
    lib, ctx, st = bare.lib, bare._ctx, L.stream_ptr()
    null = None
    assert lib.sgpmp_validate(ctx, null, 3, 1, DT, null, 0, -1, null, null, null, L.ptr(out), L.ptr(wh), st) == L.EINVAL
    assert lib.sgpmp_validate(ctx, L.ptr(x), 3, 1, DT, null, 0, -1, null, null, null, null, L.ptr(wh), st) == L.EINVAL
    assert lib.sgpmp_validate(ctx, L.ptr(x), 3, 1, DT, null, 0, -1, null, null, null, L.ptr(out), null, st) == L.EINVAL
    assert "sgpmp_validate" in L.last_error()
    assert lib.sgpmp_interpolate(ctx, null, 3, 1, DT, L.ptr(out), st) == L.EINVAL
    assert lib.sgpmp_interpolate(ctx, L.ptr(x), 3, 1, DT, null, st) == L.EINVAL
    assert lib.sgpmp_validate(ctx, null, 0, 1, DT, null, 0, -1, null, null, null, null, null, st) == L.OK      # batch 0
    assert lib.sgpmp_interpolate(ctx, null, 0, 1, DT, null, st) == L.OK
    v, w = bare.validate(x[:0].contiguous(), 1, DT)
    assert v.shape == (0, 4) and w.shape == (0, 4)
    # nothing given: every column absent
    v, w = bare.validate(x, 2, DT)
    assert torch.all(v[:, :2] == float("inf")) and torch.all(v[:, 2:] == float("-inf")) and torch.all(w == -1)
    # a chain but no spheres: the self-clearance alone; a GP term is not a grid term
    from stoch_gpmp_amd.costs.cost_functions import CostGPTrajectory
    arm = make_engine(7, T, dtype, chain=PANDA_CHAIN,
                      costs=CostGPTrajectory(7, T, None, DT, dict(sigma_gp=1.), TA(dtype)).descriptors())
    with pytest.raises(ValueError):
        arm.validate(x, 1, DT, grid_term=0)
    with pytest.raises(ValueError):
        arm.validate(x, 1, DT, grid_term=1)
    v, w = arm.validate(x, 2, DT, v_limits=[V_LIM] * 7)
    assert torch.all(v[:, 0] == float("inf")) and torch.all(w[:, 0] == -1)
    assert bool(torch.isfinite(v[:, 1:3]).all()) and torch.all(w[:, 1:3] >= 0)
    assert torch.all(v[:, 3] == float("-inf")) and torch.all(w[:, 3] == -1)


# ------------------------------------------------------------------------------------------- 8. planner
def test_planner_picks_the_cheapest_valid_particle_per_goal():
    from stoch_gpmp_amd.robots.panda import PANDA_Q_LIMITS, PANDA_V_LIMITS
    from stoch_gpmp_amd.workloads import hip_panda_planner
    ta = TA(torch.float32)
    c, T, nppg, S, G, k = SC.PANDA, 16, 4, 8, 2, 4
    goals = torch.tensor([c["goal_q"] + [0.] * 7, [0.3, 0.1, -0.2, -1.8, 0.2, 2.4, 0.5] + [0.] * 7], **ta)
    pl = hip_panda_planner(c, T, nppg, S, ta, seed=3, goals=goals)
    obs = {"obstacle_spheres": torch.as_tensor(SC.panda_spheres(5, 0)).to(**ta)}
    pl.optimize(opt_iters=3, **obs)
    means = pl.particle_means
    val = pl.validate_trajectories(n_sub=k, q_limits=PANDA_Q_LIMITS, v_limits=PANDA_V_LIMITS, **obs)
    assert val.values.shape == (G * nppg, 4) and bool(torch.isfinite(val.values[:, :3]).all())
    assert torch.all(val.occupancy == float("-inf"))                  # no grid in this cost list: does not constrain
    assert torch.equal(val.valid, (val.clearance > 0) & (val.self_clearance > 0) & (val.limit_excess <= 0))
    # a buffer at the median clearance and no limits: some particles pass, some do not
    buf = float(val.clearance.median())
    val = pl.validate_trajectories(n_sub=k, buffer=buf, **obs)
    assert torch.equal(val.valid, (val.clearance > buf) & (val.self_clearance > 0))
    assert 0 < int(val.valid.sum()) < G * nppg
    dense = pl.interpolate_trajectories(n_sub=k)
    assert dense.shape == (G * nppg, (T - 1) * (k + 1) + 1, 14) and torch.equal(dense[:, ::k + 1], means)
    best = pl.best_trajectories(n_sub=k, buffer=buf, **obs)
    sph = obs["obstacle_spheres"].reshape(-1, 4).contiguous()
    for g in range(G):
        costs = pl._engine.cost_eval(means[g * nppg:(g + 1) * nppg].contiguous(), batch_offset=g * nppg * S, spheres=sph)
        ok = val.valid[g * nppg:(g + 1) * nppg]
        p = int(best.index[g])
        if not bool(ok.any()):
            assert p == -1 and bool(torch.isnan(best.trajectories[g]).all())
            continue
        want = int(torch.where(ok, costs, torch.full_like(costs, float("inf"))).argmin()) + g * nppg
        assert p == want and float(best.cost[g]) == float(costs[p - g * nppg])
        assert torch.equal(best.trajectories[g], dense[p])
    assert int((best.index >= 0).sum()) >= 1
    none = pl.best_trajectories(n_sub=k, buffer=float(val.clearance.max()) + 1., **obs)
    assert none.index.tolist() == [-1] * G and bool(torch.isinf(none.cost).all())
