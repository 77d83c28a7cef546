"""The references tests/test_gpu_update.py holds the update, IS-weight and mode-statistics kernels to (tests/update_oracle.py),
checked on their own: every update case is the case it claims to be (the number of rows that carry weight, a non-zero scale,
finite sums beside the 1e30 rows), the dense-precision IS weights agree with the factored form restated in extended
precision, and the per-goal sums agree with a loop over particles."""
import math

import numpy as np
import pytest
import torch

from tests import update_oracle as U


def update_ids():
    return [f"n{n}-T{T}-P{P}-S{S}" for n, T, P, S in U.UPDATE_SHAPES]


@pytest.mark.parametrize("dtype_name", list(U.UPDATE_DTYPES))
@pytest.mark.parametrize("shape", U.UPDATE_SHAPES, ids=update_ids())
def test_update_cases_are_what_they_claim(shape, dtype_name):
    n, T, P, S = shape
    regimes = U.update_regimes(S)
    names = [r[0] for r in regimes]
    assert len(set(names)) == len(names)
    assert {"spread", "tie", "one_hot", "k_hot1"} <= set(names)
    for k in (3, 4, 5, 7, 8):
        assert (f"k_hot{k}" in names) == (k <= S)
    assert any("straddle" in nm for nm in names) == (S >= 65)
    for regime in regimes:
        name, k, positions = regime
        case = U.update_case(shape, dtype_name, regime)
        real, cost_t = U.UPDATE_DTYPES[dtype_name]
        assert case["samples"].dtype == real and case["means"].dtype == real and case["costs"].dtype == cost_t
        assert case["samples"].shape == (P, S, T, 2 * n)
        for v in case["costs"], case["samples"], case["means"]:
            assert bool(torch.isfinite(v).all()), name
        w, g, mu_new, A = U.update_reference(case["costs"], case["samples"], case["means"], case["tau"], case["step"])
        nnz = (w != 0).sum(1)
        want = {"spread": S, "tie": S, "one_hot": 1}.get(name, k)
        assert case["expect"] == want
        assert nnz.tolist() == [want] * P, (name, nnz.tolist())
        assert float(A.max()) > 0, name
        assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(mu_new).all()) and float(A.max()) < 10., name
        assert float((w.sum(1) - 1).abs().max()) < 1e-14
        if name == "tie":
            assert bool((w == 1. / S).all())
        if name.startswith("k_hot"):
            hot = w != 0
            cold_rows = case["samples"].double()[~hot]
            assert bool((cold_rows == float(torch.tensor(U.HUGE_ROW, dtype=torch.float64).to(real))).all())
            c = case["costs"].double()
            for p in range(P):
                assert float(c[p][hot[p]].max() - c[p][hot[p]].min()) <= case["tau"]
                if k < S:
                    assert float(c[p][~hot[p]].min() - c[p][hot[p]].max()) >= 0.99e6 * case["tau"]
                if positions is not None:
                    assert tuple(torch.nonzero(hot[p]).flatten().tolist()) == positions
        if S == 1:
            assert bool((w == 1).all()) and torch.equal(g, case["samples"].double()[:, 0] - case["means"].double())


def test_straddling_positions_cross_a_ballot_group():
    for S in (65, 255, 256, 257):
        sets = [r[2] for r in U.update_regimes(S) if r[2] is not None]
        assert len(sets) == 2
        for pos in sets:
            assert min(pos) < 64 <= max(pos) and 63 in pos and 64 in pos and S - 1 in pos


def test_stats_reference_counts_particles_per_shard():
    c = torch.arange(130 * 4, dtype=torch.float64).reshape(130, 4)
    tot, mins, P, per_shard = U.stats_reference(c)
    assert tot == float(sum(range(520))) and mins == float(sum(range(0, 520, 4))) and P == 130
    assert per_shard.tolist() == [3, 3] + [2] * 62 and per_shard.sum() == 130


@pytest.mark.parametrize("case", U.ISW_CASES, ids=[U.isw_case_id(c) for c in U.ISW_CASES])
def test_dense_is_weights_agree_with_the_factored_form_in_extended_precision(case):
    n, T = case[0], case[1]
    Sigma_inv = U.isw_prior(case)[4]
    assert Sigma_inv.shape == (T * 2 * n, T * 2 * n)
    for dtype in (torch.float64, torch.float32):
        for P in (1, 3):
            means = U.isw_means(case, P, dtype)
            for tau in (1., 3.):
                ref = U.isw_reference(case, means, tau, Sigma_inv)
                fac = U.isw_elementwise_longdouble(case, means, tau)
                assert ref.shape == (P, T + 1, 2 * n) and bool((ref[:, T] == 0).all()) and bool((fac[:, T] == 0).all())
                for p in range(P):
                    scale = float(ref[p].abs().max())
                    err = float(np.abs(fac[p] - ref[p].numpy().astype(np.longdouble)).max())
                    assert scale > 0 and err <= 1e-14 * scale, (P, tau, err / scale)


def test_dense_is_weights_agree_with_the_factored_form_at_T128():
    case = (2, 128, 0.02, 1e-3, 3., 1e-3)
    means = U.isw_means(case, 2, torch.float64)
    ref, fac = U.isw_reference(case, means, 3.), U.isw_elementwise_longdouble(case, means, 3.)
    for p in range(2):
        assert float(np.abs(fac[p] - ref[p].numpy().astype(np.longdouble)).max()) <= 1e-14 * float(ref[p].abs().max())


@pytest.mark.parametrize("case", U.ISW_CONSUMER_CASES, ids=[U.isw_case_id(c) for c in U.ISW_CONSUMER_CASES])
def test_is_weights_reference_is_the_vector_the_sweep_consumes(case):
    """(A_sq x)^T a = tau x^T Sigma^-1 mu for random x: the identity the consumer test checks on the device."""
    n, T, dt = case[0], case[1], case[2]
    P, S, tau = 3, 3, 3.
    Sigma_inv = U.isw_prior(case)[4]
    means = U.isw_means(case, P, torch.float64)
    a = U.isw_reference(case, means, tau, Sigma_inv)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(P, S, T, 2 * n, generator=g, dtype=torch.float64)
    e = torch.cat([x[..., 1:, :n] - x[..., :-1, :n] - dt * x[..., :-1, n:], x[..., 1:, n:] - x[..., :-1, n:]], dim=-1)
    Ax = torch.cat([x[..., :1, :], e, x[..., -1:, :]], dim=-2)                 # [P,S,T+1,d]
    got = (Ax * a.unsqueeze(1)).sum((-1, -2))
    want = U.is_term_reference(Sigma_inv, x, means, tau)
    assert float(((got - want).abs() / want.abs()).max()) < 1e-11


def test_mode_stats_reference_against_a_loop_over_particles():
    for G, nppg, Pg, shards in U.MODE_STATS_LAYOUTS:
        assert sum(p for _, p in shards) == Pg and [o for o, _ in shards] == [sum(p for _, p in shards[:i]) for i in range(len(shards))]
        n, T = 1, 3
        means = U.mode_stats_means(n, T, Pg, torch.float64)
        total = torch.zeros(G, T * 2 * n + 1, 2, dtype=torch.float64)
        for off, P in shards:
            total += U.mode_stats_reference(means[off:off + P], G, nppg, off)[0]
        loop = torch.zeros_like(total)
        for p in range(Pg):
            g = min(G - 1, p // nppg)
            v = means[p].reshape(-1)
            loop[g, :-1, 0] += v
            loop[g, :-1, 1] += v * v
            loop[g, -1, 0] += 1
        assert torch.allclose(total, loop, rtol=1e-13, atol=0)
        assert total[:, -1, 0].sum() == Pg and math.isclose(float(total[..., :-1, 0].sum()), float(means.sum()), rel_tol=1e-12)
    G, nppg, Pg, _ = U.MODE_STATS_LAYOUTS[-1]
    assert U.mode_stats_reference(U.mode_stats_means(1, 3, Pg, torch.float64), G, nppg)[0][:, -1, 0].tolist() == [5., 8.]
