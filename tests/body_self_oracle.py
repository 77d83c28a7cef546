"""Test-side oracle of the body's self-collision term (SGPMP_COST_BODY_SELF), straight from the definition in include/sgpmp.h, in
torch fp64: sphere centres from oracle/fk.py's link frames, the hinge on (margin + r_i + r_j) - |p_i - p_j| over the counted pairs,
gradients from autograd through the FK.  The two points where autograd would answer NaN are defined as the header defines them:
D = 0 gives the value margin + r_i + r_j and a zero gradient, h = 0 gives a zero gradient.  Shares no code with
stoch_gpmp_amd/body_self.py, robots/body.py or the kernels."""
import numpy as np
import torch

from oracle import ref_equiv as R
from oracle.fk import fk_all_links
from tests.body_sdf_oracle import body_tensors, frames_points
from tests.voxel_sdf_oracle import ARM_C, CHAINS


def pairs_of(rows):
    """rows (one integer per sphere; bit j of rows[i]: pair (i, j), only j > i read) -> (i [N], j [N]) long tensors in summation
    order: i ascending, then j ascending."""
    out = []
    for i, row in enumerate(rows):
        bits = int(row) >> (i + 1)
        j = i + 1
        while bits:
            if bits & 1:
                out.append((i, j))
            bits >>= 1
            j += 1
    assert out and all(j < len(rows) for _, j in out)
    return torch.tensor([p[0] for p in out]).long(), torch.tensor([p[1] for p in out]).long()


def pair_distance(frames, body, rows):
    """-> (D [..., N], finite [..., N]): D = |p_i - p_j| with a zero (sub)gradient at D = 0; `finite` is False where a coordinate of
    either centre is not finite."""
    pts = frames_points(frames, body)
    i, j = pairs_of(rows)
    d = pts[..., i, :] - pts[..., j, :]
    ss = (d * d).sum(-1)
    pos = ss > 0
    D = torch.where(pos, torch.sqrt(torch.where(pos, ss, torch.ones_like(ss))), torch.zeros_like(ss))
    return D, torch.isfinite(pts[..., i, :]).all(-1) & torch.isfinite(pts[..., j, :]).all(-1)


def frames_clearance(frames, body, rows):
    """-> s [..., N] = D - r_i - r_j (NaN where a centre is not finite)."""
    _, _, r = body_tensors(body)
    i, j = pairs_of(rows)
    D, ok = pair_distance(frames, body, rows)
    return torch.where(ok, D - r[i] - r[j], torch.full_like(D, float("nan")))


def frames_field(frames, body, rows, margin):
    """-> f [...] = sum over the counted pairs of the hinge (NaN where any counted centre is not finite)."""
    _, _, r = body_tensors(body)
    i, j = pairs_of(rows)
    D, ok = pair_distance(frames, body, rows)
    e = (margin + r[i] + r[j]) - D
    h = torch.where(e > 0, e, torch.zeros_like(e))
    f = h.sum(-1)
    return torch.where(ok.all(-1), f, torch.full_like(f, float("nan")))


def config_field_and_grad(q, chain, body, rows, margin):
    """q [B, n] numpy -> (f [B], df/dq [B, n], min s [B], its gradient [B, n], s [B, N], D [B, N]), gradients from autograd; a
    configuration with a non-finite counted centre has NaN everywhere."""
    x = torch.tensor(np.asarray(q, dtype=np.float64), requires_grad=True)
    frames = fk_all_links(x, chain)
    _, _, r = body_tensors(body)
    i, j = pairs_of(rows)
    D, ok = pair_distance(frames, body, rows)
    ok = ok.all(-1)
    e = (margin + r[i] + r[j]) - D
    f = torch.where(e > 0, e, torch.zeros_like(e)).sum(-1)
    s = D - r[i] - r[j]
    smin = s.min(-1)[0]
    good = torch.nonzero(ok).flatten()
    g, = torch.autograd.grad(f[good].sum(), x, retain_graph=True)
    gs, = torch.autograd.grad(smin[good].sum(), x)
    bad = (~ok).numpy()
    f, smin, s, D = f.detach().numpy().copy(), smin.detach().numpy().copy(), s.detach().numpy().copy(), D.detach().numpy().copy()
    g, gs = g.numpy().copy(), gs.numpy().copy()
    for arr in (f, smin, s, g, gs):
        arr[bad] = np.nan
    return f, g, smin, gs, s, D


def conditions(s, D, margin):
    """What the GPU tests assert about their random inputs: (min over everything of |margin - s_ij|, min of D_ij) -- the distance of
    every counted pair from the hinge's kink and from the D = 0 singularity."""
    return float(np.abs(margin - s).min()), float(D.min())


def argmin_gap(s):
    """s [B, N] -> the gap between the smallest and the second smallest clearance [B] (inf for N = 1)."""
    if s.shape[1] < 2:
        return np.full(s.shape[0], np.inf)
    part = np.sort(s, axis=1)
    return part[:, 1] - part[:, 0]


def sweep_term(trajs, n, chain, body, rows, margin, sigma):
    """trajs [B, T, 2n] torch fp64 -> the term of a cost list [B]: 1 / sigma^2 * sum over t = 1 .. T-1 of f(q_t)."""
    B, T = trajs.shape[0], trajs.shape[1]
    if T < 2:
        return torch.zeros(B, dtype=torch.float64)
    q = trajs[:, 1:, :n].reshape(-1, n)
    f = frames_field(fk_all_links(q, chain), body, rows, margin).reshape(B, T - 1)
    return f.sum(-1) / sigma ** 2


def gpmp_systems_fn(body, rows, margin, chain=None, n_sub=0, weight=1., field=True, c=None):
    """systems_fn of oracle.gpmp_equiv.OracleGPMP: GP + goal prior (+ the term's rows at the waypoints 1 .. T-1: error f, A = -df/dq
    by autograd through FK, precision 1 / sigma^2; + with n_sub > 0 its rows on the inserted states, precision weight / sigma^2)."""
    from oracle import gpmp_equiv as GP
    from tests import gpmp_dense_oracle as DO
    c = ARM_C if c is None else c
    chain = CHAINS["panda"][0] if chain is None else chain
    n = c["n_dof"]
    start = torch.tensor(c["start_q"] + [0.] * n, dtype=torch.float64)
    goals = torch.tensor([c["goal_q"] + [0.] * n], dtype=torch.float64)
    fk = lambda q: fk_all_links(q, chain)                                               # noqa: E731
    fn_field = lambda fr: frames_field(fr, body, rows, margin)                          # noqa: E731

    def fn(m, **obs):
        out = [GP.linear_system_gp(m, start, n, c["dt"], c["cost_sigma_start"], c["cost_sigma_gp"]),
               GP.linear_system_goal_prior(m, goals, m.shape[0], n, c["sigma_goal_prior"])]
        if field:
            out.append(R.collision_linear_system(m, n, fk, fn_field, c["sigma_coll"]))
            if n_sub > 0 and weight > 0.:
                out.append(DO.collision_system(m, n, n_sub, c["dt"], weight, fn_field, c["sigma_coll"], FK=fk))
        return out
    return fn


# ------------------------------------------------------------------------------------------------ the cases of the tests
SPACING, RADIUS = 0.12, 0.06        # the along_links body of tests/test_gpu_body_sdf.py
SEED = 11                           # of the configurations; tests/test_cpu_body_self.py holds the cases below to the conditions
BIG_SEED = 2                        # of the 64-sphere body


def rows_by_gap(links, gap, ignore=()):
    """The rows that count every pair whose link indices differ by at least `gap` (links non-decreasing), without the link pairs
    (a, b), a < b, listed in `ignore`."""
    rows = []
    for i, li in enumerate(links):
        row = 0
        for j in range(i + 1, len(links)):
            if links[j] - li >= gap and (li, links[j]) not in ignore:
                row += 2 ** j
        rows.append(row)
    return rows


# the Panda's link pairs (gap >= 2) whose spheres of an along_links body keep a constant distance: links that share an origin
# (joints with a zero offset) and the wrist and hand, links 5 to 10, which are rigid or turn about a common point
PANDA_CONSTANT = [(0, 2), (1, 3), (2, 4), (4, 6)] + [(a, b) for a in range(5, 11) for b in range(a + 2, 11)]


def cases(which):
    """name -> (BodySpheres, rows, margin) on chain `which`: two spheres; along_links under the gap-2 rule; the largest table with
    every cross-link pair counted; a pair with only fixed joints between its links (exactly zero gradient); link 0 against the
    last link."""
    from stoch_gpmp_amd.robots.body import BodySpheres
    chain = CHAINS[which][0]
    L = len(chain) + 1
    fixed = [k for k, joint in enumerate(chain) if joint[1] == "fixed"][0]
    rng = np.random.default_rng(BIG_SEED)
    along = BodySpheres.along_links(chain, SPACING, RADIUS)
    big = BodySpheres(rng.integers(0, L, 64), rng.uniform(-0.1, 0.1, (64, 3)), rng.uniform(0., 0.02, 64))
    return {"M=2": (BodySpheres([1, L - 2], [(0.03, -0.02, 0.04), (0.01, 0.05, -0.02)], [0.05, 0.08]), [2, 0], 0.3),
            "along_links": (along, rows_by_gap(along.links, 2), 0.15),
            "M=64": (big, rows_by_gap(big.links, 1), 0.0285),
            "behind a fixed joint": (BodySpheres([fixed, L - 1], [(0., 0.03, 0.02), (0.02, 0., 0.01)], [0.06, 0.04]), [2, 0], 0.3),
            "link 0 against the last": (BodySpheres([0, L - 1], [(0.1, 0., 0.2), (0., 0.01, 0.02)], [0.1, 0.07]), [2, 0], 0.3)}
