"""Host side of the dense (GP-interpolated) trajectories: stoch_gpmp_amd/dense.py against dense GP conditioning in numpy, the
fine-index bookkeeping, and the Panda's limits as data.  No GPU, no library."""
import numpy as np
import pytest

from stoch_gpmp_amd import dense


def gp_interpolation_weights(n, dt, tau, Qc):
    """Lambda(tau), Psi(tau) [2n,2n] of the constant-velocity GP by their definition (state order (q, v))."""
    I, Z = np.eye(n), np.zeros((n, n))

    def Phi(t):
        return np.block([[I, t * I], [Z, I]])

    def Q(t):
        return np.block([[t ** 3 / 3 * Qc, t ** 2 / 2 * Qc], [t ** 2 / 2 * Qc, t * Qc]])
    Psi = np.linalg.solve(Q(dt).T, (Q(tau) @ Phi(dt - tau).T).T).T
    return Phi(tau) - Psi @ Phi(dt), Psi


@pytest.mark.parametrize("dt", [0.02, 0.05])
@pytest.mark.parametrize("k", [0, 1, 3, 31])
def test_hermite_weights_are_the_gp_interpolation_for_any_Qc(dt, k):
    n = 2
    rng = np.random.default_rng(7 + k)
    A = rng.normal(size=(n, n))
    Qc = A @ A.T + n * np.eye(n)                       # random, non-isotropic, SPD: it must cancel
    lam, psi = dense.hermite_weights(k, dt)
    assert lam.shape == psi.shape == (k + 1, 2, 2)
    np.testing.assert_array_equal(lam[0], np.eye(2))
    np.testing.assert_array_equal(psi[0], np.zeros((2, 2)))
    for m in range(k + 1):
        Lam, Psi = gp_interpolation_weights(n, dt, m / (k + 1) * dt, Qc)
        np.testing.assert_allclose(np.kron(lam[m], np.eye(n)), Lam, rtol=0, atol=1e-12)
        np.testing.assert_allclose(np.kron(psi[m], np.eye(n)), Psi, rtol=0, atol=1e-12)


def test_fine_length_and_times():
    assert dense.fine_length(2, 0) == 2
    assert dense.fine_length(64, 4) == 316
    assert dense.fine_length(66, 31) == 65 * 32 + 1
    t = dense.fine_times(8, 3, 0.05)
    assert t.shape == (29,)
    np.testing.assert_allclose(t[::4], np.arange(8) * 0.05, rtol=0, atol=1e-15)      # support waypoints keep their times
    np.testing.assert_allclose(np.diff(t), 0.0125, rtol=1e-12)
    np.testing.assert_array_equal(dense.fine_times(5, 0, 0.1), np.arange(5) * 0.1)
    with pytest.raises(ValueError):
        dense.fine_length(1, 0)
    with pytest.raises(ValueError):
        dense.fine_length(4, -1)
    with pytest.raises(ValueError):
        dense.hermite_weights(1, 0.)


def test_host_interpolation_keeps_support_states_and_reproduces_cubics():
    rng = np.random.default_rng(3)
    x = rng.normal(size=(3, 6, 4))
    for k in (0, 1, 3):
        out = dense.interpolate(x, k, 0.05)
        assert out.shape == (3, dense.fine_length(6, k), 4)
        np.testing.assert_array_equal(out[:, ::k + 1], x)
    # a cubic in t with its own derivative as velocity is reproduced exactly by the Hermite interpolant
    T, k, dt = 5, 3, 0.1
    c = rng.normal(size=(4, 2))
    poly = lambda t: c[0] + c[1] * t[:, None] + c[2] * t[:, None] ** 2 + c[3] * t[:, None] ** 3          # noqa: E731
    dpoly = lambda t: c[1] + 2 * c[2] * t[:, None] + 3 * c[3] * t[:, None] ** 2                          # noqa: E731
    ts, tf = np.arange(T) * dt, dense.fine_times(T, k, dt)
    out = dense.interpolate(np.concatenate([poly(ts), dpoly(ts)], axis=1), k, dt)
    np.testing.assert_allclose(out, np.concatenate([poly(tf), dpoly(tf)], axis=1), rtol=0, atol=1e-13)


def test_panda_limits_contain_the_workload():
    from stoch_gpmp_amd.robots.panda import PANDA_Q_LIMITS, PANDA_V_LIMITS
    from stoch_gpmp_amd.robots.panda_chain import PANDA_Q_LOWER, PANDA_Q_UPPER
    from stoch_gpmp_amd.workloads import PANDA
    lo, hi = (np.asarray(v) for v in PANDA_Q_LIMITS)
    assert lo.shape == hi.shape == (7,) and len(PANDA_V_LIMITS) == 7
    assert list(lo) == PANDA_Q_LOWER and list(hi) == PANDA_Q_UPPER
    assert np.all(lo < hi) and np.all(np.asarray(PANDA_V_LIMITS) > 0)
    for q in (PANDA["start_q"], PANDA["goal_q"]):
        assert np.all(lo <= np.asarray(q)) and np.all(np.asarray(q) <= hi)
