"""Host side of the continuous-time cost gradient (sgpmp_dense_cost_grad): the numpy helpers of stoch_gpmp_amd/dense.py that restate
the kernel's Hermite adjoint and limit derivative, and what the built library and the binding declare.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from stoch_gpmp_amd import dense

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.37


def dense_matrix(T, n_sub, n, dt):
    """W [T_f 2n, T 2n] with interpolate(x).ravel() = W x.ravel(), column by column from the unit vectors."""
    cols = []
    for j in range(T * 2 * n):
        e = np.zeros(T * 2 * n)
        e[j] = 1.
        cols.append(dense.interpolate(e.reshape(T, 2 * n), n_sub, dt).ravel())
    return np.stack(cols, axis=1)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("n_sub", [0, 1, 4, 31])
@pytest.mark.parametrize("T", [2, 5])
def test_hermite_pullback_is_the_transpose_of_interpolate(T, n_sub, n):
    rng = np.random.default_rng(100 * T + 10 * n_sub + n)
    Tf = dense.fine_length(T, n_sub)
    W = dense_matrix(T, n_sub, n, DT)
    g = rng.standard_normal((3, Tf, 2 * n))
    got = dense.hermite_pullback(g, T, n_sub, DT)
    assert got.shape == (3, T, 2 * n) and got.dtype == np.float64
    ref = (g.reshape(3, -1) @ W).reshape(3, T, 2 * n)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    x = rng.standard_normal((3, T, 2 * n))
    lhs = (dense.interpolate(x, n_sub, DT) * g).sum()
    rhs = (x * got).sum()
    scale = np.abs(dense.interpolate(x, n_sub, DT) * g).sum()
    assert abs(lhs - rhs) <= 1e-12 * scale
    with pytest.raises(ValueError):
        dense.hermite_pullback(g[:, :-1] if Tf > 1 else g, T + 1, n_sub, DT)


def torch_limit_penalty(x, q_lo, q_hi, v_max, sigma):
    n = x.shape[-1] // 2
    q, v = x[..., :n], x[..., n:]
    out = torch.zeros(x.shape[:-2], dtype=torch.float64)
    if q_lo is not None:
        out = out + torch.clamp(torch.as_tensor(q_lo, dtype=torch.float64) - q, min=0.).square().sum((-2, -1))
    if q_hi is not None:
        out = out + torch.clamp(q - torch.as_tensor(q_hi, dtype=torch.float64), min=0.).square().sum((-2, -1))
    if v_max is not None:
        out = out + torch.clamp(v.abs() - torch.as_tensor(v_max, dtype=torch.float64), min=0.).square().sum((-2, -1))
    return out / sigma ** 2


LO, HI, VM = [-0.5, -0.2, -0.9], [0.4, 0.6, 0.3], [0.7, 0.2, 1.1]


@pytest.mark.parametrize("which", ["all", "lower", "upper", "velocity"])
def test_limit_penalty_grad_matches_autograd(which):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(4, 9, 6, generator=g, dtype=torch.float64)
    q_lo = LO if which in ("all", "lower") else None
    q_hi = HI if which in ("all", "upper") else None
    v_max = VM if which in ("all", "velocity") else None
    sigma = 0.3
    xt = x.clone().requires_grad_()
    J = torch_limit_penalty(xt, q_lo, q_hi, v_max, sigma)
    assert np.abs(J.detach().numpy() - dense.limit_penalty(x.numpy(), (q_lo, q_hi), v_max, sigma)).max() <= 1e-12 * float(J.detach().max())
    ref, = torch.autograd.grad(J.sum(), xt)
    got = dense.limit_penalty_grad(x.numpy(), (q_lo, q_hi), v_max, sigma)
    assert got.shape == x.shape and got.dtype == np.float64
    assert float(ref.abs().max()) > 0
    assert np.abs(got - ref.numpy()).max() <= 1e-12 * float(ref.abs().max())
    # zero exactly where nothing is exceeded
    n = 3
    q, v = x[..., :n].numpy(), x[..., n:].numpy()
    inside_q = np.ones_like(q, dtype=bool)
    if q_lo is not None:
        inside_q &= q >= np.asarray(q_lo)
    if q_hi is not None:
        inside_q &= q <= np.asarray(q_hi)
    inside_v = np.ones_like(v, dtype=bool) if v_max is None else np.abs(v) <= np.asarray(v_max)
    assert inside_q.any() and not inside_q.all() or which == "velocity"
    assert np.all(got[..., :n][inside_q] == 0) and np.all(got[..., n:][inside_v] == 0)
    if which == "lower":
        assert np.all(got[..., :n] <= 0) and np.all(got[..., n:] == 0)
    if which == "upper":
        assert np.all(got[..., :n] >= 0) and np.all(got[..., n:] == 0)
    if which == "velocity":
        assert np.all(got[..., :n] == 0) and np.all(got[..., n:] * v >= 0)


def test_missing_limits_give_zeros():
    x = np.random.default_rng(0).standard_normal((2, 5, 4))
    assert np.all(dense.limit_penalty_grad(x) == 0)
    assert np.all(dense.limit_penalty_grad(x, (None, None), None, None) == 0)
    assert dense.limit_penalty_grad(x).shape == x.shape
    with pytest.raises(ValueError):
        dense.limit_penalty_grad(x, ([0.] * 2, None), None, None)


def test_library_exports_the_entry_point_and_the_header_documents_it():
    from stoch_gpmp_amd import _lib as L
    lib = L.load()
    assert hasattr(lib, "sgpmp_dense_cost_grad")
    res, args = L.SIGNATURES["sgpmp_dense_cost_grad"]
    assert len(args) == 18                                  # sgpmp_dense_cost's 16 + support + grad
    assert len(L.SIGNATURES["sgpmp_dense_cost"][1]) == 16
    assert lib.sgpmp_dense_cost_grad.argtypes == args
    header = open(os.path.join(ROOT, "include", "sgpmp.h")).read()
    assert re.search(r"#define\s+SGPMP_ABI_VERSION\s+6\b", header) and L.ABI_VERSION == 6 and lib.sgpmp_abi_version() == 6
    decl = re.search(r"int sgpmp_dense_cost_grad\((.*?)\);", header, re.S)
    assert decl is not None
    for word in ("support", "accumulate", "grad", "costs64", "sigma_limit"):
        assert word in decl.group(1)
    doc = header[:decl.start()].rsplit("/*", 1)[1]
    for word in ("SGPMP_EINVAL", "occupancy", "GRID", "NaN", "arg-max", "LDS"):
        assert word in doc, word


def test_engine_and_planner_expose_the_call():
    import inspect
    from stoch_gpmp_amd.engine import Engine
    from stoch_gpmp_amd.planner import GPMP, StochGPMP
    sig = inspect.signature(Engine.dense_cost_grad)
    assert list(sig.parameters)[1:] == ["trajs", "n_sub", "dt", "spheres", "weight", "q_limits", "v_limits", "sigma_limit",
                                        "support", "grad", "accumulate"]
    assert sig.parameters["support"].default is False and sig.parameters["accumulate"].default is False
    sig = inspect.signature(StochGPMP.continuous_cost)
    assert list(sig.parameters)[1:8] == ["trajs", "n_sub", "weight", "q_limits", "v_limits", "sigma_limit", "support"]
    assert sig.parameters["support"].default is True
    assert GPMP.continuous_cost is StochGPMP.continuous_cost
