"""Host-side arithmetic of the dense (GP-interpolated) trajectories: index bookkeeping and the interpolation weights that
`sgpmp_interpolate` / `sgpmp_validate` / `sgpmp_dense_cost` / `sgpmp_dense_cost_grad` (csrc/traj_dense.hip) apply on the GPU, and the
rows `sgpmp_gpmp_set_dense` adds to GPMP's linear system (csrc/gpmp_dense.hip).  numpy only, no GPU, no library.

Between two support states x_i = (q_i, v_i) and x_{i+1}, `dt` apart, the posterior mean of the constant-velocity GP prior is

    x(tau) = Lambda(tau) x_i + Psi(tau) x_{i+1},  Psi = Q(tau) Phi(dt - tau)^T Q(dt)^-1,  Lambda = Phi(tau) - Psi Phi(dt)

(the GPMP "GP interpolation").  For this prior Q_c cancels and so does the prior mean: per degree of freedom the weights are
the cubic Hermite basis on (q, v), which is what `hermite_weights` returns.  The reference has no counterpart.
"""
import numpy as np


def fine_length(T, n_sub):
    """Number of fine states of a T-waypoint trajectory with n_sub states inserted per interval."""
    T, n_sub = int(T), int(n_sub)
    if T < 2 or n_sub < 0:
        raise ValueError("fine_length: T >= 2 and n_sub >= 0")
    return (T - 1) * (n_sub + 1) + 1


def fine_times(T, n_sub, dt):
    """Time of every fine state [T_f]: fine index f = i (n_sub + 1) + m lies at (i + m / (n_sub + 1)) dt."""
    f = np.arange(fine_length(T, n_sub), dtype=np.float64)
    return f * (float(dt) / (n_sub + 1))


def hermite_weights(n_sub, dt):
    """(Lambda, Psi), each [n_sub + 1, 2, 2]: the 2 x 2 blocks, per degree of freedom on (q, v), of the interpolation weights
    at s = m / (n_sub + 1), m = 0 .. n_sub, of an interval of length dt; x(s) = Lambda[m] x_i + Psi[m] x_{i+1}.
    m = 0 is the support state itself: Lambda[0] = I, Psi[0] = 0."""
    n_sub, dt = int(n_sub), float(dt)
    if n_sub < 0 or not dt > 0.:
        raise ValueError("hermite_weights: n_sub >= 0 and dt > 0")
    s = np.arange(n_sub + 1, dtype=np.float64) / (n_sub + 1)
    s2, s3 = s * s, s * s * s
    h00, h10, h01, h11 = 2 * s3 - 3 * s2 + 1, s3 - 2 * s2 + s, -2 * s3 + 3 * s2, s3 - s2
    g00, g10, g11 = 6 * s2 - 6 * s, 3 * s2 - 4 * s + 1, 3 * s2 - 2 * s
    lam = np.empty((n_sub + 1, 2, 2))
    psi = np.empty((n_sub + 1, 2, 2))
    lam[:, 0, 0], lam[:, 0, 1], lam[:, 1, 0], lam[:, 1, 1] = h00, h10 * dt, g00 / dt, g10
    psi[:, 0, 0], psi[:, 0, 1], psi[:, 1, 0], psi[:, 1, 1] = h01, h11 * dt, -g00 / dt, g11
    return lam, psi


def interpolate(trajs, n_sub, dt):
    """The same interpolation on the host, in the dtype of `trajs` [..., T, 2n] -> [..., T_f, 2n] (checks, plots)."""
    x = np.asarray(trajs)
    T, n = x.shape[-2], x.shape[-1] // 2
    lam, psi = hermite_weights(n_sub, dt)
    k1 = n_sub + 1
    out = np.empty(x.shape[:-2] + (fine_length(T, n_sub), 2 * n), dtype=x.dtype)
    a, b = x[..., :-1, :], x[..., 1:, :]
    for m in range(k1):
        la, ps = lam[m], psi[m]
        q = la[0, 0] * a[..., :n] + la[0, 1] * a[..., n:] + ps[0, 0] * b[..., :n] + ps[0, 1] * b[..., n:]
        v = la[1, 0] * a[..., :n] + la[1, 1] * a[..., n:] + ps[1, 0] * b[..., :n] + ps[1, 1] * b[..., n:]
        out[..., m:-1:k1, :n], out[..., m:-1:k1, n:] = q, v
    out[..., 0:-1:k1, :] = a                      # support states are copies
    out[..., -1, :] = x[..., -1, :]
    return out


def inserted_indices(T, n_sub):
    """Fine indices of the INSERTED states (m = 1 .. n_sub of every interval), ascending: the states the collision part of
    `sgpmp_dense_cost` covers.  The support states f = i (n_sub + 1) are the cost sweep's."""
    f = np.arange(fine_length(T, n_sub), dtype=np.int64)
    return f[f % (int(n_sub) + 1) != 0]


def limit_penalty(fine, q_limits=None, v_limits=None, sigma_limit=None):
    """The limit part of `sgpmp_dense_cost` on fine states [..., T_f, 2n] -> [...], in fp64:
    1/sigma_limit^2 sum over states and dof of max(0, q_lo - q)^2 + max(0, q - q_hi)^2 + max(0, |q'| - v_max)^2.
    q_limits = (lower [n], upper [n]), either may be None; v_limits [n].  A limit that is not given contributes nothing."""
    x = np.asarray(fine, dtype=np.float64)
    n = x.shape[-1] // 2
    q, v = x[..., :n], x[..., n:]
    out = np.zeros(x.shape[:-2], dtype=np.float64)
    q_lo, q_hi = (None, None) if q_limits is None else q_limits
    if q_lo is None and q_hi is None and v_limits is None:
        return out
    if sigma_limit is None or not float(sigma_limit) > 0.:
        raise ValueError("limit_penalty: limits need sigma_limit > 0")
    if q_lo is not None:
        out += (np.maximum(np.asarray(q_lo, dtype=np.float64) - q, 0.) ** 2).sum(axis=(-2, -1))
    if q_hi is not None:
        out += (np.maximum(q - np.asarray(q_hi, dtype=np.float64), 0.) ** 2).sum(axis=(-2, -1))
    if v_limits is not None:
        out += (np.maximum(np.abs(v) - np.asarray(v_limits, dtype=np.float64), 0.) ** 2).sum(axis=(-2, -1))
    return out / float(sigma_limit) ** 2


def hermite_pullback(g_fine, T, n_sub, dt):
    """The transpose of `interpolate`: a gradient with respect to the fine states [..., T_f, 2n] -> the gradient with respect to
    the support states [..., T, 2n], in fp64.  Fine state m of interval i hands Lambda[m]^T g to x_i and Psi[m]^T g to x_{i+1}
    (m = 0 and the last state: the identity) -- what `sgpmp_dense_cost_grad` does per lane."""
    g = np.asarray(g_fine, dtype=np.float64)
    T, n_sub = int(T), int(n_sub)
    n = g.shape[-1] // 2
    if g.shape[-2] != fine_length(T, n_sub):
        raise ValueError(f"hermite_pullback: {g.shape[-2]} fine states, T = {T} and n_sub = {n_sub} give {fine_length(T, n_sub)}")
    lam, psi = hermite_weights(n_sub, dt)
    k1 = n_sub + 1
    out = np.zeros(g.shape[:-2] + (T, 2 * n), dtype=np.float64)
    out[..., -1, :] = g[..., -1, :]
    out[..., :-1, :] = g[..., 0:-1:k1, :]
    for m in range(1, k1):
        gq, gv = g[..., m:-1:k1, :n], g[..., m:-1:k1, n:]
        la, ps = lam[m], psi[m]
        out[..., :-1, :n] += la[0, 0] * gq + la[1, 0] * gv
        out[..., :-1, n:] += la[0, 1] * gq + la[1, 1] * gv
        out[..., 1:, :n] += ps[0, 0] * gq + ps[1, 0] * gv
        out[..., 1:, n:] += ps[0, 1] * gq + ps[1, 1] * gv
    return out


def limit_penalty_grad(fine, q_limits=None, v_limits=None, sigma_limit=None):
    """d `limit_penalty` / d fine states, [..., T_f, 2n] in fp64: 2/sigma_limit^2 x the signed excess, zero where no limit is
    exceeded (the penalty is C^1).  A limit that is not given contributes nothing."""
    x = np.asarray(fine, dtype=np.float64)
    n = x.shape[-1] // 2
    q, v = x[..., :n], x[..., n:]
    out = np.zeros(x.shape, dtype=np.float64)
    q_lo, q_hi = (None, None) if q_limits is None else q_limits
    if q_lo is None and q_hi is None and v_limits is None:
        return out
    if sigma_limit is None or not float(sigma_limit) > 0.:
        raise ValueError("limit_penalty_grad: limits need sigma_limit > 0")
    if q_lo is not None:
        out[..., :n] -= np.maximum(np.asarray(q_lo, dtype=np.float64) - q, 0.)
    if q_hi is not None:
        out[..., :n] += np.maximum(q - np.asarray(q_hi, dtype=np.float64), 0.)
    if v_limits is not None:
        out[..., n:] += np.sign(v) * np.maximum(np.abs(v) - np.asarray(v_limits, dtype=np.float64), 0.)
    return out * (2. / float(sigma_limit) ** 2)


def gn_rows(trajs, n_sub, dt, q_limits=None, v_limits=None):
    """The scalar rows the continuous-time factors add to GPMP's linear system (`sgpmp_gpmp_set_dense`; convention of the
    reference: A row = -d error / d x, b = error), as their nonzero coefficients, in fp64.  Fine state f of trajs [..., T, 2n]
    lies in interval i = `interval[f]` at sub-step `m[f]`; every row at f touches x_i and x_{i+1} only (the last state is
    written as m = n_sub + 1 of interval T - 2: Lambda = 0, Psi = I).  Returns a dict with
      'interval', 'm'  [T_f] int64;
      'collision'      [T_f, 4]: a collision row of a field with gradient g = d field / d q_f has the entries
                       -collision[f] (x) g on (q_i, v_i, q_{i+1}, v_{i+1}) -- row 0 of (Lambda[m], Psi[m]); b = the field;
      'q_lo', 'q_hi', 'v_max' (the limits that are given): (A [..., T_f, n, 4], b [..., T_f, n]), the row of degree of freedom j
                       at state f: its entries on dof j of (q_i, v_i, q_{i+1}, v_{i+1}) and its error max(0, q_lo - q),
                       max(0, q - q_hi), max(0, |q'| - v_max); an inactive row is a zero row.
    q_limits = (lower [n], upper [n]), either may be None; v_limits [n]."""
    x = np.asarray(trajs, dtype=np.float64)
    T, n = x.shape[-2], x.shape[-1] // 2
    n_sub = int(n_sub)
    k1 = n_sub + 1
    lam, psi = hermite_weights(n_sub, dt)
    P4 = np.concatenate([np.stack([lam[:, 0, 0], lam[:, 0, 1], psi[:, 0, 0], psi[:, 0, 1]], axis=1), [[0., 0., 1., 0.]]])
    V4 = np.concatenate([np.stack([lam[:, 1, 0], lam[:, 1, 1], psi[:, 1, 0], psi[:, 1, 1]], axis=1), [[0., 0., 0., 1.]]])
    f = np.arange(fine_length(T, n_sub), dtype=np.int64)
    interval = np.minimum(f // k1, T - 2)
    m = f - interval * k1
    out = {'interval': interval, 'm': m, 'collision': P4[m]}
    fine = interpolate(x, n_sub, dt)
    q, v = fine[..., :n], fine[..., n:]
    cp, cv = P4[m][:, None, :], V4[m][:, None, :]                   # [T_f, 1, 4]
    q_lo, q_hi = (None, None) if q_limits is None else q_limits
    if q_lo is not None:
        e = np.maximum(np.asarray(q_lo, dtype=np.float64) - q, 0.)
        out['q_lo'] = ((e > 0.)[..., None] * cp, e)
    if q_hi is not None:
        e = np.maximum(q - np.asarray(q_hi, dtype=np.float64), 0.)
        out['q_hi'] = ((e > 0.)[..., None] * -cp, e)
    if v_limits is not None:
        e = np.maximum(np.abs(v) - np.asarray(v_limits, dtype=np.float64), 0.)
        out['v_max'] = (-((e > 0.) * np.sign(v))[..., None] * cv, e)
    return out
