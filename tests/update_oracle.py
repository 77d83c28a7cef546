"""Test-side references of the update kernel (K4), the importance-sampling weights (K5) and the per-goal mean statistics,
each straight from its definition in torch fp64 on the CPU, and the inputs the tests feed both sides.  CPU only; shares no
code with the kernels.

K4:  w = softmax(-c / tau),  g = sum_s w_s (x_s - mu),  mu' = mu + step g,  and the scale A = sum_s w_s |x_s - mu|.
K5:  the one vector a with  tau x^T Sigma^-1 mu = (A_sq x)^T a  for every x, from the DENSE precision (oracle.ref_equiv):
     a = tau A_sq^-T (Sigma^-1 mu),  A_sq x = (x_0, e_0(x), .., e_{T-2}(x)) -- not the kernel's factored form.
"""
import zlib

import numpy as np
import torch

from oracle import ref_equiv as R

TAU, STEP = 0.7, 0.25
HUGE_ROW = 1e30                        # what the sample rows WITHOUT weight hold in the k_hot cases (finite; times an exact 0)

# ------------------------------------------------------------------------------------------------------------- K4
UPDATE_SHAPES = [  # n, T, P, S
    (1, 3, 1, 1),        # M = 6: two elements per thread, a single sample (weight exactly 1, g = x - mu)
    (3, 5, 3, 9),        # M = 30: two elements per thread
    (7, 37, 2, 5),       # M = 518: two elements per thread, second pass of the element loop with three live threads
    (2, 6, 3, 9),        # the shape test_update_with_fp32_costs_tensor has
    (8, 64, 2, 7),       # M = 1024 = 256 * 4 exactly
    (7, 74, 2, 6),       # M = 1036: four elements per thread, second pass
    (2, 4, 130, 4),      # P = 2 * 64 + 2: the statistics shards wrap
] + [(2, 4, 2, S) for S in (63, 64, 65, 255, 256, 257)]          # ballot-group and thread-stride boundaries

# name -> (dtype of samples / means / outputs, dtype of the costs tensor)
UPDATE_DTYPES = {
    "f64": (torch.float64, torch.float64),
    "f32_costs64": (torch.float32, torch.float64),
    "f32_costs32": (torch.float32, torch.float32),
}


def update_regimes(S):
    """The cost regimes of a shape with S samples: (name, k, positions).  k_hot with k in {1, 3, 4, 5, 7, 8} where S has
    that many rows; for S >= 65 also the positions {0, 63, 64, S-1} and {62, 63, 64, 65, S-1} (those that exist, once each:
    at S = 65 the sets are {0, 63, 64} and {62, 63, 64})."""
    out = [("spread", S, None), ("tie", S, None), ("one_hot", 1, None)]
    for k in (1, 3, 4, 5, 7, 8):
        if k <= S:
            out.append((f"k_hot{k}", k, None))
    if S >= 65:
        for tag, pos in (("a", (0, 63, 64, S - 1)), ("b", (62, 63, 64, 65, S - 1))):
            pos = tuple(sorted({q for q in pos if q < S}))
            out.append((f"k_hot{len(pos)}_straddle_{tag}", len(pos), pos))
    return out


def hot_positions(S, k, p):
    """k distinct rows of particle p, spread over [0, S) and moved on with p."""
    return [(p * 7 + (i * S) // k) % S for i in range(k)]


def update_case(shape, dtype_name, regime):
    """-> dict(costs [P,S], samples [P,S,T,d], means [P,T,d]) CPU tensors in the dtypes the device is given, tau, step and
    `expect`: the number of rows per particle that must carry weight."""
    n, T, P, S = shape
    name, k, positions = regime
    real, cost_t = UPDATE_DTYPES[dtype_name]
    g = torch.Generator().manual_seed(zlib.crc32(repr((shape, name)).encode()))
    d = 2 * n
    means = torch.randn(P, T, d, generator=g, dtype=torch.float64)
    samples = means.unsqueeze(1) + 0.1 * torch.randn(P, S, T, d, generator=g, dtype=torch.float64)
    u = torch.rand(P, S, generator=g, dtype=torch.float64)
    if name == "spread":
        costs = 4. * u
    elif name == "tie":
        costs = torch.full((P, S), 1e12, dtype=torch.float64)
    elif name == "one_hot":                        # a spread of 1e6 tau in equal steps (>= 3900 tau apart at S = 257), shuffled
        lin = torch.linspace(0., 1e6 * TAU, S, dtype=torch.float64) if S > 1 else torch.zeros(1, dtype=torch.float64)
        costs = torch.stack([lin[torch.randperm(S, generator=g)] for _ in range(P)])
    else:
        costs = u * TAU + 1e6 * TAU                # rows without weight: 1e6 tau above the hot ones ...
        for p in range(P):
            hot = list(positions) if positions is not None else hot_positions(S, k, p)
            assert len(set(hot)) == k
            costs[p, hot] = u[p, hot] * TAU        # ... which lie within tau of each other
            cold = torch.ones(S, dtype=torch.bool)
            cold[hot] = False
            samples[p, cold] = HUGE_ROW
    return dict(costs=costs.to(cost_t).contiguous(), samples=samples.to(real).contiguous(), means=means.to(real).contiguous(),
                tau=TAU, step=STEP, expect=k, real=real)


def update_reference(costs, samples, means, tau, step):
    """Plain torch fp64 from the exact inputs the device is given (fp32 cast up) -> w [P,S], g, mu', A [P,T,d]."""
    c, x, mu = costs.double().cpu(), samples.double().cpu(), means.double().cpu()
    P, S = c.shape
    w = torch.softmax(-c / tau, dim=1)
    dx = x - mu.unsqueeze(1)
    ww = w.view(P, S, 1, 1)
    g = (ww * dx).sum(1)
    A = (ww * dx.abs()).sum(1)
    return w, g, mu + step * g, A


def stats_reference(costs):
    """(sum_{p,s} c, sum_p min_s c, P) and the count per shard j: the number of p with p & 63 == j."""
    c = costs.double().cpu()
    P = c.shape[0]
    return float(c.sum()), float(c.min(1)[0].sum()), P, np.bincount(np.arange(P) & 63, minlength=64)


# ------------------------------------------------------------------------------------------------------------- K5
def _qc_inv(n):
    """The full SPD Q_c^-1 of test_dense_sampler_with_full_Qc_matches_oracle."""
    g = torch.Generator().manual_seed(3)
    A = torch.randn(n, n, generator=g, dtype=torch.float64)
    return A @ A.t() + n * torch.eye(n, dtype=torch.float64)


ISW_CASES = [  # n, T, dt, sigma_start, sigma_gp (None: a full Q_c^-1), sigma_goal (None: no goal)
    (1, 2, 0.3, 0.5, 1.5, 2.0),
    (2, 3, 0.02, 1e-3, 3.0, 1e-3),
    (7, 18, 0.05, 1e-4, 0.8, 0.1),          # (T + 1) d = 266: two blocks per particle
    (8, 4, 0.1, 0.1, 0.5, None),
    (2, 64, 0.02, 1e-3, 20.0, 1e-3),
    (3, 10, 0.1, 0.05, None, 0.2),
    (7, 24, 0.1, 0.05, None, 0.2),
]
ISW_CONSUMER_CASES = [ISW_CASES[1], ISW_CASES[2], ISW_CASES[5]]


def isw_case_id(case):
    n, T, dt, ss, sg, sgoal = case
    return f"n{n}-T{T}-{'Qc' if sg is None else 'iso'}-{'goal' if sgoal is not None else 'nogoal'}"


def isw_prior(case):
    """-> (Q_c^-1 or None, K_s, Q^-1, K_g or None, dense Sigma^-1 [M,M]) in fp64."""
    n, T, dt, ss, sg, sgoal = case
    d = 2 * n
    qc = _qc_inv(n) if sg is None else None
    K_s = R.unary_K(d, ss, torch.float64)
    Q_inv = R.q_inv_matrix(n, dt, sg, torch.float64, Q_c_inv=qc)
    K_g = None if sgoal is None else R.unary_K(d, sgoal, torch.float64)
    return qc, K_s, Q_inv, K_g, R.dense_prior_precision(T, n, dt, K_s, Q_inv, K_g, torch.float64)


def isw_means(case, P, dtype):
    n, T = case[0], case[1]
    g = torch.Generator().manual_seed(zlib.crc32(repr((case, P)).encode()))
    return torch.randn(P, T, 2 * n, generator=g, dtype=torch.float64).to(dtype).contiguous()


def isw_reference(case, means, temperature, Sigma_inv=None):
    """a = tau A_sq^-T (Sigma^-1 mu) per particle, [P, T+1, d] with block T all zeros (means: cast up)."""
    n, T, dt = case[0], case[1], case[2]
    d, M = 2 * n, case[1] * 2 * n
    if Sigma_inv is None:
        Sigma_inv = isw_prior(case)[4]
    A_sq = torch.eye(M, dtype=torch.float64)
    phi = R.phi_matrix(n, dt, torch.float64)
    for i in range(T - 1):
        A_sq[(i + 1) * d:(i + 2) * d, i * d:(i + 1) * d] = -phi
    mu = means.double().cpu().reshape(-1, M)
    rhs = Sigma_inv @ mu.t()                                                  # [M, P]
    a = temperature * torch.linalg.solve_triangular(A_sq.t().contiguous(), rhs, upper=True)
    out = torch.zeros(mu.shape[0], T + 1, d, dtype=torch.float64)
    out[:, :T] = a.t().reshape(-1, T, d)
    return out


def isw_elementwise_longdouble(case, means, temperature):
    """The kernel's factored form (is_weight_elem), restated in np.longdouble: per block t the start factor or
    Q^-1 e_{t-1}(mu), plus the goal factor K_g mu_{T-1} carried back through (Phi^T)^(T-1-t)."""
    n, T, dt = case[0], case[1], case[2]
    d = 2 * n
    _, K_s, Q_inv, K_g, _ = isw_prior(case)
    LD = np.longdouble
    mu = means.double().cpu().numpy().astype(LD).reshape(-1, T, d)
    Q, ks, dtl = Q_inv.numpy().astype(LD), LD(float(K_s[0, 0])), LD(dt)
    out = np.zeros((mu.shape[0], T + 1, d), dtype=LD)
    out[:, 0] = ks * mu[:, 0]
    e = mu[:, 1:].copy()
    e[..., :n] -= mu[:, :-1, :n] + dtl * mu[:, :-1, n:]
    e[..., n:] -= mu[:, :-1, n:]
    out[:, 1:T] = e @ Q.T
    if K_g is not None:
        kg, last = LD(float(K_g[0, 0])), mu[:, T - 1]
        for t in range(T):
            k = LD(T - 1 - t)
            out[:, t, :n] += kg * last[:, :n]
            out[:, t, n:] += kg * (k * dtl * last[:, :n] + last[:, n:])
    return LD(temperature) * out


def is_term_reference(Sigma_inv, x, means, temperature):
    """tau x^T Sigma^-1 mu: x [P,S,T,d], means [P,T,d] -> [P,S]."""
    P, S = x.shape[0], x.shape[1]
    xs, mu = x.double().cpu().reshape(P, S, -1), means.double().cpu().reshape(P, -1)
    return temperature * torch.einsum("psi,ij,pj->ps", xs, Sigma_inv, mu)


# ------------------------------------------------------------------------------------------------- mode statistics
MODE_STATS_ELEMENTS = [(1, 3), (2, 16), (7, 9), (8, 4)]        # M = 6, 64 (count alone in a second block), 126, 64
# (G, particles per goal, global particles, shards as (offset, particles))
MODE_STATS_LAYOUTS = [(1, P, P, [(0, P)]) for P in (1, 15, 16, 17, 63, 64, 65, 129)] + [
    (3, 17, 51, [(0, 51)]),
    (3, 17, 51, [(0, 17), (17, 20), (37, 14)]),                # the second boundary cuts the last goal
    (2, 5, 13, [(0, 13)]),                                     # the last goal takes eight
]


def mode_stats_means(n, T, P, dtype):
    g = torch.Generator().manual_seed(zlib.crc32(repr((n, T, P)).encode()))
    return (torch.randn(P, T, 2 * n, generator=g, dtype=torch.float64) * 2. + 0.5).to(dtype).contiguous()


def mode_stats_reference(means, G, nppg, offset=0):
    """means: this shard's [P,T,d] (global particles offset ..) -> (out [G, M+1, 2] fp64 as sgpmp_mode_stats lays it out,
    bound [G, M+1, 2]: sum |v| and sum v^2 per element, what the rounding of the sums is measured on)."""
    mu = means.double().cpu().reshape(means.shape[0], -1)
    P, M = mu.shape
    out = torch.zeros(G, M + 1, 2, dtype=torch.float64)
    scale = torch.zeros(G, M + 1, 2, dtype=torch.float64)
    for g in range(G):
        lo = g * nppg
        hi = None if g == G - 1 else lo + nppg
        a = max(lo - offset, 0)
        b = P if hi is None else min(hi - offset, P)
        if b <= a:
            continue
        v = mu[a:b]
        out[g, :M, 0], out[g, :M, 1] = v.sum(0), (v * v).sum(0)
        scale[g, :M, 0], scale[g, :M, 1] = v.abs().sum(0), (v * v).sum(0)
        out[g, M, 0] = b - a
    return out, scale
