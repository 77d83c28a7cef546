"""Test-local dense oracle of GPMP's continuous-time factors (include/sgpmp.h: sgpmp_gpmp_set_dense) -- TEST INFRASTRUCTURE ONLY.

Extra (A, b, K) systems appended to the list `oracle.gpmp_equiv.panda_systems_fn` returns and solved by `OracleGPMP(..., "inverse")`,
the way tests/test_gpu_planner.py::test_gpmp_with_end_effector_goal_matches_oracle appends its system.  Every row comes from
autograd: the errors are functions of a torch Hermite interpolation of the particle means (and, for the collision rows, of
oracle.fk and the oracle.ref_equiv fields), and A = -d error / d means.  Nothing here knows the closed form of a row.
"""
import numpy as np
import torch

from oracle import gpmp_equiv as GP
from oracle import ref_equiv as R
from oracle.fk import fk_all_links
from tests import scenarios as SC


def hermite_fine(means, n_sub, dt):
    """Differentiable cubic Hermite (= constant-velocity GP) interpolation, means [B,T,2n] -> fine states [B,T_f,2n];
    fine index f = i (n_sub + 1) + m lies at s = m / (n_sub + 1) of interval i, the last state is the last waypoint."""
    B, T, d = means.shape
    n, k1 = d // 2, n_sub + 1
    a, b = means[:, :-1], means[:, 1:]
    per_m = []
    for m in range(k1):
        s = m / k1
        h00, h10, h01, h11 = 2 * s**3 - 3 * s**2 + 1, s**3 - 2 * s**2 + s, -2 * s**3 + 3 * s**2, s**3 - s**2
        g00, g10, g01, g11 = 6 * s**2 - 6 * s, 3 * s**2 - 4 * s + 1, -6 * s**2 + 6 * s, 3 * s**2 - 2 * s
        q = h00 * a[..., :n] + h10 * dt * a[..., n:] + h01 * b[..., :n] + h11 * dt * b[..., n:]
        v = g00 / dt * a[..., :n] + g10 * a[..., n:] + g01 / dt * b[..., :n] + g11 * b[..., n:]
        per_m.append(torch.cat([q, v], -1))
    fine = torch.stack(per_m, 2).reshape(B, (T - 1) * k1, d)
    return torch.cat([fine, means[:, -1:]], 1)


def autograd_rows(means, n_sub, dt, err_fn, per_dof=False):
    """err_fn(fine [B,T_f,d]) -> errors [B,T_f,R], the R errors of a fine state functions of that state alone.
    -> (A [B,T_f,R,T d] = -d error / d means, errors), by backward passes: the errors of one sub-step m and row r over the
    intervals of one parity have disjoint supports (x_i, x_{i+1}), so one pass yields all their rows.  per_dof: row r is a
    function of degree of freedom r % n alone (the limit rows) -- the n rows of a kind then share a pass as well."""
    B, T, d = means.shape
    k1 = n_sub + 1
    x = means.detach().clone().requires_grad_(True)
    err = err_fn(hermite_fine(x, n_sub, dt))
    Tf, Rn = err.shape[1], err.shape[2]
    A = torch.zeros(B, Tf, Rn, T * d, dtype=means.dtype)
    f_all = np.arange(Tf)
    iv = np.minimum(f_all // k1, T - 2)
    mm = f_all - iv * k1
    for m in range(k1 + 1):
        for parity in (0, 1):
            sel = [int(f) for f in f_all[(mm == m) & (iv % 2 == parity)]]
            if not sel:
                continue
            n = d // 2
            for rows in ([list(range(r0, r0 + n)) for r0 in range(0, Rn, n)] if per_dof else [[r] for r in range(Rn)]):
                g, = torch.autograd.grad(err[:, sel][:, :, rows].sum(), x, retain_graph=True)
                for f in sel:
                    i = int(iv[f])
                    for r in rows:
                        cols = [w * d + c for w in (i, i + 1) for c in ((r % n, n + r % n) if per_dof else range(d))]
                        A[:, f, r, cols] = -g.reshape(B, T * d)[:, cols]
    return A, err.detach()


def _system(A, b, K_scalar):
    """Rows [B,m,N], errors [B,m] and one precision -> (A, b [B,m,1], K [B,m,m])."""
    B, m = b.shape
    return A, b.unsqueeze(-1), K_scalar * torch.eye(m, dtype=A.dtype).repeat(B, 1, 1)


def collision_system(means, n, n_sub, dt, weight, field_fn, sigma, FK=fk_all_links):
    """One SPHERES / SELF term on the INSERTED states: error = field(q_f), precision = weight / sigma^2."""
    B, T, d = means.shape

    def err_fn(fine):
        Tf = fine.shape[1]
        frames = FK(fine.reshape(-1, d)[:, :n]).reshape(B, Tf, -1, 4, 4)
        return field_fn(frames).reshape(B, Tf, 1)
    A, err = autograd_rows(means, n_sub, dt, err_fn)
    ins = [f for f in range(err.shape[1]) if f % (n_sub + 1) != 0]
    return _system(A[:, ins, 0], err[:, ins, 0], weight / sigma ** 2)


def limit_system(means, n, n_sub, dt, q_lo=None, q_hi=None, v_max=None, sigma_limit=None):
    """The limit rows of ALL fine states: per degree of freedom max(0, q_lo - q), max(0, q - q_hi), max(0, |q'| - v_max) of the
    limits that are given, precision 1 / sigma_limit^2."""
    B, T, d = means.shape
    dt_ = means.dtype

    def err_fn(fine):
        q, v = fine[..., :n], fine[..., n:]
        rows = []
        if q_lo is not None:
            rows.append(torch.clamp(torch.as_tensor(q_lo, dtype=dt_) - q, min=0.))
        if q_hi is not None:
            rows.append(torch.clamp(q - torch.as_tensor(q_hi, dtype=dt_), min=0.))
        if v_max is not None:
            rows.append(torch.clamp(v.abs() - torch.as_tensor(v_max, dtype=dt_), min=0.))
        return torch.cat(rows, -1)
    A, err = autograd_rows(means, n_sub, dt, err_fn, per_dof=True)
    Tf, Rn = err.shape[1], err.shape[2]
    return _system(A.reshape(B, Tf * Rn, T * d), err.reshape(B, Tf * Rn), 1. / sigma_limit ** 2)


def dense_systems(means, n, n_sub, dt, weight=0., fields=(), q_lo=None, q_hi=None, v_max=None, sigma_limit=None,
                  FK=fk_all_links):
    """The systems the setting adds: `fields` = [(field_fn(frames) -> [...], sigma)] for the collision rows (weight > 0 and
    n_sub > 0), then the limit rows."""
    out = []
    if weight > 0. and n_sub > 0:
        out += [collision_system(means, n, n_sub, dt, weight, fn, sigma, FK) for fn, sigma in fields]
    if q_lo is not None or q_hi is not None or v_max is not None:
        out.append(limit_system(means, n, n_sub, dt, q_lo, q_hi, v_max, sigma_limit))
    return out


def panda_fields(c, obstacle_spheres, sphere_field="rbf", clamp_sdf=False):
    """The collision terms of the Panda cost list of tests/scenarios.py as (field_fn, sigma)."""
    return [(lambda fr: R.field_self(fr, margin=c["self_margin"]), c["sigma_self"]),
            (lambda fr: R.field_spheres(fr, obstacle_spheres, field_type=sphere_field, clamp_sdf=clamp_sdf), c["sigma_coll"])]


def panda_dense_systems_fn(c, T, nppg, goals, n_sub, weight=0., q_lo=None, q_hi=None, v_max=None, sigma_limit=None,
                           sphere_field="rbf", clamp_sdf=False, collision=True, limits=True):
    """oracle.gpmp_equiv.panda_systems_fn's list with the continuous-time systems appended; `collision` / `limits` = False leave
    that part out (what the sensitivity conditions compare against)."""
    n = c["n_dof"]
    if sphere_field == "rbf":
        base = GP.panda_systems_fn(c, T, nppg, goals, fk_all_links, sphere_field)
    else:
        def base(means, obstacle_spheres=None):
            start = torch.tensor(c["start_q"] + [0.] * n, dtype=means.dtype)
            return [GP.linear_system_gp(means, start, n, c["dt"], c["cost_sigma_start"], c["cost_sigma_gp"]),
                    GP.linear_system_goal_prior(means, goals, nppg, n, c["sigma_goal_prior"]),
                    R.collision_linear_system(means, n, fk_all_links, lambda fr: R.field_self(fr, margin=c["self_margin"]),
                                              c["sigma_self"]),
                    R.collision_linear_system(means, n, fk_all_links,
                                              lambda fr: R.field_spheres(fr, obstacle_spheres, field_type=sphere_field,
                                                                         clamp_sdf=clamp_sdf), c["sigma_coll"])]

    def fn(means, obstacle_spheres=None):
        lim = dict(q_lo=q_lo, q_hi=q_hi, v_max=v_max, sigma_limit=sigma_limit) if limits else {}
        return base(means, obstacle_spheres=obstacle_spheres) + dense_systems(
            means, n, n_sub, c["dt"], weight if collision else 0.,
            panda_fields(c, obstacle_spheres, sphere_field, clamp_sdf), **lim)
    return fn


def field_dense_diag(systems):
    """sum over the particles of diag(A^T K A) of the systems past the GP and goal-prior ones (the list's first two): what
    sgpmp_gpmp_linearize's diag_sum carries with the option on.  -> [T d]"""
    A, b, K = _stack(systems[2:])
    return torch.diagonal(A.transpose(1, 2) @ K @ A, dim1=1, dim2=2).sum(0)


def _stack(systems):
    As, bs, Ks = zip(*systems)
    A = torch.cat(As, dim=1)
    K = torch.zeros(A.shape[0], A.shape[1], A.shape[1], dtype=A.dtype)
    o = 0
    for Ki in Ks:
        K[:, o:o + Ki.shape[1], o:o + Ki.shape[1]] = Ki
        o += Ki.shape[1]
    return A, torch.cat(bs, dim=1), K


def g7_setting(g):
    """The inputs that make the tests bite (fixture g7_gpmp.npz, lm/means0): weight 1e3, sigma_limit 1e-4, q_lo / q_hi the
    per-joint 10 % / 90 % quantiles of the fixture's positions, v_max the 80 % quantile of |velocity|."""
    m = torch.from_numpy(g["lm/means0"])
    n = m.shape[-1] // 2
    q, v = m[..., :n].reshape(-1, n), m[..., n:].reshape(-1, n).abs()
    return dict(weight=1e3, sigma_limit=1e-4, q_lo=torch.quantile(q, 0.1, dim=0), q_hi=torch.quantile(q, 0.9, dim=0),
                v_max=torch.quantile(v, 0.8, dim=0))


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


PANDA = SC.PANDA


# ---------------------------------------------------------------------------------- shared, computed once
_CACHE = {}


def g7_first_step(g, tag, n_sub, delta, trust, collision=True, limits=True, sphere_field="rbf", clamp_sdf=False, **only):
    """(d_theta, costs) of the oracle's FIRST step on fixture g7 under g7_setting (`only`: replaces the limit part, e.g.
    q_lo=..., for the parts-alone cases), cached: the sensitivity conditions and the parity tests share them."""
    key = (tag, n_sub, delta, trust, collision, limits, sphere_field, clamp_sdf, tuple(sorted(only)))
    if key not in _CACHE:
        o = g7_oracle(g, tag, n_sub, delta, trust, collision, limits, sphere_field, clamp_sdf, **only)
        _CACHE[key] = o.step(obstacle_spheres=torch.from_numpy(g["spheres"]))
    return _CACHE[key]


def g7_oracle(g, tag, n_sub, delta, trust, collision=True, limits=True, sphere_field="rbf", clamp_sdf=False, **only):
    T, nppg = [int(v) for v in g["dims"]]
    s = g7_setting(g)
    lim = {k: s[k] for k in ("q_lo", "q_hi", "v_max")} if not only else {k: s[k] for k in only}
    fn = panda_dense_systems_fn(PANDA, T, nppg, torch.from_numpy(g["goals"]), n_sub, weight=s["weight"],
                                sigma_limit=s["sigma_limit"], sphere_field=sphere_field, clamp_sdf=clamp_sdf,
                                collision=collision, limits=limits, **lim)
    return GP.OracleGPMP(torch.from_numpy(g[f"{tag}/means0"]), fn, 0.5, delta, trust, "inverse")
