"""CPU checks of GPMP's continuous-time factors (include/sgpmp.h: sgpmp_gpmp_set_dense): the declarations, the numpy twin of the
rows (dense.gn_rows) against autograd rows of the test-local oracle, the band structure of the oracle's normal matrix, and the
conditions under which the GPU parity tests bite."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from stoch_gpmp_amd import _lib, dense
from tests import gpmp_dense_oracle as DO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [("lm", 5.0, False), ("tr", 1e-2, True)]


def test_header_declares_the_entry_points_under_abi_6():
    src = open(os.path.join(ROOT, "include", "sgpmp.h")).read()
    assert re.search(r"#define SGPMP_ABI_VERSION 6\b", src) and _lib.ABI_VERSION == 6
    m = re.search(r"int sgpmp_gpmp_set_dense\(([^;]*)\);", src)
    assert m, "sgpmp_gpmp_set_dense is not declared"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert args == ["sgpmp_ctx* ctx", "int n_sub", "double dt", "double weight", "const double* q_lo", "const double* q_hi",
                    "const double* v_max", "double sigma_limit"]
    assert re.search(r"const char\* sgpmp_last_gpmp_kernel\(void\);", src)
    assert re.search(r"^int sgpmp_last_gpmp_ppw\(void\);", src, flags=re.M)
    res, argt = _lib.SIGNATURES["sgpmp_gpmp_set_dense"]
    assert len(argt) == len(args) and _lib.SIGNATURES["sgpmp_last_gpmp_kernel"][1] == []
    import ctypes
    assert _lib.SIGNATURES["sgpmp_last_gpmp_ppw"] == (ctypes.c_int, [])
    # an older build of ABI 6 may lack it and still load (_lib.ADDED_UNDER_THIS_ABI); the library of this tree has it
    assert _lib.ADDED_UNDER_THIS_ABI == {"sgpmp_last_gpmp_ppw"} and _lib.load().sgpmp_last_gpmp_ppw() == 0
    # linearize and solve keep their signatures
    assert len(_lib.SIGNATURES["sgpmp_gpmp_linearize"][1]) == 6 and len(_lib.SIGNATURES["sgpmp_gpmp_solve"][1]) == 8


def test_engine_and_planner_signatures():
    from stoch_gpmp_amd.engine import Engine
    from stoch_gpmp_amd.gpmp import GPMP
    from stoch_gpmp_amd.planner import StochGPMP
    p = inspect.signature(Engine.gpmp_set_dense).parameters
    assert list(p) == ["self", "n_sub", "dt", "weight", "q_limits", "v_limits", "sigma_limit"]
    assert hasattr(Engine, "last_gpmp_kernel") and list(inspect.signature(Engine.last_gpmp_ppw).parameters) == ["self"]
    assert list(inspect.signature(GPMP.set_dense_cost).parameters) == list(inspect.signature(StochGPMP.set_dense_cost).parameters)
    assert GPMP.set_dense_cost is not StochGPMP.set_dense_cost and "NotImplementedError" not in inspect.getsource(GPMP.set_dense_cost)


@pytest.mark.parametrize("n_sub", [0, 1, 3])
def test_gn_rows_match_autograd_rows(golden, n_sub):
    """dense.gn_rows (closed form) against rows the oracle gets from autograd through its own interpolation, to 1e-12: the limit
    rows of every kind with both active and inactive rows present (and both signs of q' among the active velocity rows), and a
    collision row through a field that is linear in q_f (gradient = a known vector)."""
    g = golden("g7_gpmp.npz")
    means = torch.from_numpy(g["lm/means0"])
    B, T, d = means.shape
    n, dt = d // 2, DO.PANDA["dt"]
    s = DO.g7_setting(g)
    rows = dense.gn_rows(means.numpy(), n_sub, dt, q_limits=(s["q_lo"].numpy(), s["q_hi"].numpy()), v_limits=s["v_max"].numpy())
    Tf = dense.fine_length(T, n_sub)
    iv = rows["interval"]
    fine = dense.interpolate(means.numpy(), n_sub, dt)
    for kind in ("q_lo", "q_hi", "v_max"):
        A_o, b_o, _ = DO.limit_system(means, n, n_sub, dt, sigma_limit=1.0, **{kind: s[kind]})
        A4, e = rows[kind]
        A = np.zeros((B, Tf, n, T * d))
        for f in range(Tf):
            for j in range(n):
                for c, col in enumerate((iv[f] * d + j, iv[f] * d + n + j, (iv[f] + 1) * d + j, (iv[f] + 1) * d + n + j)):
                    A[:, f, j, col] = A4[:, f, j, c]
        assert np.abs(A.reshape(B, Tf * n, T * d) - A_o.numpy()).max() < 1e-12
        assert np.abs(e.reshape(B, Tf * n) - b_o[..., 0].numpy()).max() < 1e-12
        active = e > 0.
        assert active.any() and (~active).any(), kind
        if kind == "v_max":
            v = fine[..., n:]
            assert (v[active] > 0).any() and (v[active] < 0).any()
    w = torch.linspace(0.3, -1.1, n, dtype=torch.float64)
    A_o, err = DO.autograd_rows(means, n_sub, dt, lambda fine_t: (fine_t[..., :n] * w).sum(-1, keepdim=True))
    A = np.zeros((B, Tf, T * d))
    for f in range(Tf):
        c4 = rows["collision"][f]
        A[:, f, iv[f] * d:iv[f] * d + n] += -c4[0] * w.numpy()
        A[:, f, iv[f] * d + n:iv[f] * d + d] += -c4[1] * w.numpy()
        A[:, f, (iv[f] + 1) * d:(iv[f] + 1) * d + n] += -c4[2] * w.numpy()
        A[:, f, (iv[f] + 1) * d + n:(iv[f] + 2) * d] += -c4[3] * w.numpy()
    assert np.abs(A - A_o[:, :, 0].numpy()).max() < 1e-12


def test_oracle_normal_matrix_is_block_tridiagonal(golden):
    """Every new row touches x_i and x_{i+1} only: outside the block-tridiagonal band the oracle's A^T K A is exactly zero."""
    from oracle import gpmp_equiv as GP
    g = golden("g7_gpmp.npz")
    o = DO.g7_oracle(g, "lm", 3, 5.0, False)
    A, b, K = GP.composite_linear_system(o.particle_means, o.systems_fn(o.particle_means, obstacle_spheres=torch.from_numpy(g["spheres"])))
    N = A.transpose(1, 2) @ K @ A
    T, d = o.particle_means.shape[1:]
    blk = torch.arange(T * d) // d
    off = (blk[:, None] - blk[None, :]).abs() > 1
    assert off.any() and float(N[:, off].abs().max()) == 0.
    sub = (blk[:, None] - blk[None, :]) == 1
    base = DO.g7_oracle(g, "lm", 3, 5.0, False, collision=False, limits=False)
    A0, _, K0 = GP.composite_linear_system(base.particle_means, base.systems_fn(base.particle_means, obstacle_spheres=torch.from_numpy(g["spheres"])))
    N0 = A0.transpose(1, 2) @ K0 @ A0
    assert float((N - N0)[:, sub].abs().max()) > 0.          # the sub-diagonal block is no longer the constant -Q^-1 Phi


@pytest.mark.parametrize("tag,delta,trust", MODES)
def test_inputs_make_the_parity_tests_bite(golden, tag, delta, trust):
    """With weight 1e3, sigma_limit 1e-4 and the quantile limits, each part alone moves the oracle's d_theta by at least 0.05
    (relative L2); 5 .. 25 % of the limit rows are active."""
    g = golden("g7_gpmp.npz")
    full, _ = DO.g7_first_step(g, tag, 3, delta, trust)
    no_coll, _ = DO.g7_first_step(g, tag, 3, delta, trust, collision=False)
    no_lim, _ = DO.g7_first_step(g, tag, 3, delta, trust, limits=False)
    assert DO.rel_l2(no_coll, full) >= 0.05 and DO.rel_l2(no_lim, full) >= 0.05
    s = DO.g7_setting(g)
    means = torch.from_numpy(g[f"{tag}/means0"])
    _, b, _ = DO.limit_system(means, 7, 3, DO.PANDA["dt"], s["q_lo"], s["q_hi"], s["v_max"], s["sigma_limit"])
    frac = float((b > 0).double().mean())
    assert 0.05 / 3 < frac < 0.25, frac


def test_gpmp_solve_layout_over_every_admissible_shape(tmp_path):
    """csrc/sgpmp_internal.h gpmp_solve_layout -- the function launch_gpmp_solve takes its particles per wave and dynamic LDS from --
    itself, through tests/host_asan/gpmp_layout.cpp (host-only, -fsanitize=address,undefined): over all traj_len in [2, 128] and
    0 .. 4 field terms, two or four particles per wave, the request with the kernel's 512 B of static LDS inside a workgroup's
    160 KiB, four exactly while 4 x 8 T (32 + 9 F) <= 150 KiB; and the rows tests/test_gpu_gpmp_solve.py runs on the GPU."""
    import shutil
    import subprocess
    if not os.path.exists("/opt/rocm/bin/hipcc") or not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang")
    d = os.path.join(ROOT, "tests", "host_asan")
    b = str(tmp_path / "build")
    r = subprocess.run(["make", "-C", d, f"B={b}", os.path.join(b, "gpmp_layout")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith(("SGPMP_", "STUB_", "HOST_ASAN"))}
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    p = subprocess.run([os.path.join(b, "gpmp_layout")], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "GPMP_LAYOUT_OK" in p.stdout, (p.stdout[-1000:], p.stderr[-4000:])
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    shutil.rmtree(b, ignore_errors=True)
    lines = p.stdout.split("\n")
    assert lines[0] == "LIMITS 128 4"
    rows = {}
    for ln in lines[1:]:
        v = ln.split()
        if len(v) == 5:
            rows[(int(v[0]), int(v[1]))] = tuple(int(x) for x in v[2:])
    assert sorted(rows) == [(T, F) for T in range(2, 129) for F in range(5)]
    for (T, F), (ppw, per, lds) in rows.items():
        assert per == 8 * T * (32 + 9 * F) and lds == ppw * per, (T, F)
        assert ppw in (2, 4) and ppw * per + 512 <= 160 * 1024, (T, F, ppw)
        assert (ppw == 4) == (4 * per <= 150 * 1024), (T, F, ppw)
    # planar (one field), Panda (two fields), no field: (ppw, request)
    want = {(49, 1): (4, 64288), (50, 1): (4, 65600), (117, 1): (4, 153504), (118, 1): (2, 77408), (128, 1): (2, 83968),
            (40, 2): (4, 64000), (41, 2): (4, 65600), (96, 2): (4, 153600), (97, 2): (2, 77600),
            (64, 0): (4, 65536), (65, 0): (4, 66560), (128, 4): (2, 139264)}
    for k, (ppw, lds) in want.items():
        assert (rows[k][0], rows[k][2]) == (ppw, lds), (k, rows[k])
