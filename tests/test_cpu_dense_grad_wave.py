"""The text of dense_cost_grad_kernel (csrc/traj_dense.hip) run on the CPU: cut out of the source, compiled for the host under
AddressSanitizer + UBSan as a 64-thread lock-step twin of one wave (tests/host_wave/wave.cpp) and held to autograd through the
oracle -- the same restatement tests/test_gpu_dense_grad.py holds the device to, on dense.interpolate's fine states.  No GPU.

What it covers without a device: the Hermite adjoint with its shuffle and the carry across passes of 64 lanes (T = 65, 66), both
storage instantiations (chain length compiled in / generic), interpolated link points, the sdf arg-max rule, the limit derivative,
accumulate, the NaN rule, and every LDS index (the column is a bounded array under ASan).  Bound: the GPU tests' own, rtol 1e-9
(fp64) / 3e-4 (fp32) with atol = rtol x max |ref| of the trajectory."""
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle.fk import PANDA_CHAIN, _origin
from stoch_gpmp_amd import dense

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
RTOL = {torch.float64: 1e-9, torch.float32: 3e-4}


def cut(src, a, b):
    i = src.index(a)
    return src[i:src.index(b, i)]


@pytest.fixture(scope="module")
def wave(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++")
    d = tmp_path_factory.mktemp("host_wave")
    src = open(os.path.join(ROOT, "stoch_gpmp_amd", "csrc", "traj_dense.hip")).read()
    parts = [cut(src, "template <typename real>\nstruct HermiteK {", "// " + "-" * 82 + " sgpmp_interpolate"),
             cut(src, "template <typename real>\nstruct DenseCostK {", "// (HIP passes at most 4 KiB of kernel arguments)"),
             cut(src, "// this lane's columns, stride 64:", "// SGPMP_OK, or the code of a refusal")]
    text = "\n".join(parts)
    decl = "    extern __shared__ __align__(16) unsigned char lds_raw[];\n"
    assert text.count(decl) == 1 and "dense_cost_grad_kernel(" in text
    (d / "kernel_funcs.inc").write_text(text.replace(decl, ""))
    exe = str(d / "wave")
    r = subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-pthread", "-Wno-unused-value", "-Wno-unknown-pragmas", "-I", str(d),
                        os.path.join(ROOT, "tests", "host_wave", "wave.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(dtype, njf, n, chain, T, k, dt, support, accumulate, weight, spec, sph, limits, x, g0):
        B = x.shape[0]
        lines = [f"{int(dtype == torch.float64)} {njf} {n} {len(chain)} {T} {k} {dt!r} {int(support)} {int(accumulate)} {weight!r} {B}"]
        q = 0
        for _, kind, rpy, xyz in chain:
            H = _origin(rpy, xyz, torch.float64)
            rev = int(kind == "revolute")
            lines.append(" ".join(repr(float(v)) for v in H[:3, :3].flatten()) + " " + " ".join(repr(float(v)) for v in H[:3, 3])
                         + f" {rev} {q if rev else 0}")
            q += rev
        lines.append(str(len(spec)))
        for t in spec:
            ni = t.get("num_interpolate", 0)
            al = [float(a) for a in torch.linspace(0, 1, ni + 2)[1:ni + 1].double()] + [0.] * (8 - ni)
            if t["kind"] == "self":
                kind, flags, K2 = 5, 0, -1. / (2 * t["margin"] ** 2)
            else:
                kind, flags, K2 = 4, {"rbf": 0, "sdf": 1}[t["field_type"]] | (16 if t.get("clamp") else 0), 0.
            lines.append(f"{kind} {flags} {1. / t['sigma'] ** 2!r} {K2!r} {len(chain) + 1 + 2 * ni} {ni} 5 7 " + " ".join(repr(a) for a in al))
        lines.append(str(0 if sph is None else sph.shape[0]))
        lines += [] if sph is None else [" ".join(repr(float(v)) for v in s) for s in sph]
        if limits is None:
            lines.append("0 0 1.0")
        else:
            (qlo, qhi), vm, sig = limits
            lines.append(f"{int(qlo is not None or qhi is not None)} {int(vm is not None)} {sig!r}")
            if qlo is not None or qhi is not None:
                lines += [f"{(qlo[i] if qlo is not None else -1e300)!r} {(qhi[i] if qhi is not None else 1e300)!r}" for i in range(n)]
            if vm is not None:
                lines.append(" ".join(repr(float(v)) for v in vm))
        lines.append(" ".join(repr(float(v)) for v in x.double().flatten()))
        lines.append(" ".join(repr(float(v)) for v in g0.double().flatten()))
        case = d / "case.txt"
        case.write_text("\n".join(lines) + "\n")
        res = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=600)
        assert res.returncode == 0 and not res.stderr.strip(), res.stderr[-3000:]          # (a sanitizer report fails the case)
        out = np.array([float(v) for v in res.stdout.split()])
        return torch.from_numpy(out[:B]), torch.from_numpy(out[B:].reshape(B, T, 2 * n))
    return run


def compare(val, grad, ref, gref, dtype, what):
    B = gref.shape[0]
    rtol = RTOL[dtype]
    top = gref.abs().reshape(B, -1).max(1)[0].reshape(B, 1, 1)
    bound = rtol * gref.abs() + rtol * top
    err = (grad - gref).abs()
    print(f"    {what}: worst gradient error / bound = {float((err / bound.clamp(min=1e-300)).max()):.3e}, "
          f"value rel err {float(((val - ref).abs() / ref.abs().clamp(min=1e-300)).max()):.3e}")
    assert bool(torch.isfinite(grad).all()) and bool((err <= bound).all()), what
    assert bool(((val - ref).abs() <= rtol * ref.abs()).all()), what


def panda_case(wave, dtype, T, k, support, njf=10, B=2, spec=None, limits="default", accumulate=False, seed=None):
    import tests.test_gpu_dense_grad as G
    from tests.test_gpu_dense_cost import DT, Q_LIM, SIGMA_LIM, V_LIM, arm_inputs, panda_terms, spheres
    spec = panda_terms()[0] if spec is None else spec
    limits = ((Q_LIM[0], Q_LIM[1]), V_LIM, SIGMA_LIM) if limits == "default" else limits
    sph = spheres().double()
    x = arm_inputs(T, dtype, B=B, seed=seed)
    g0 = torch.zeros(B, T, 14, dtype=dtype)
    if accumulate:
        g0 = (1e4 * torch.randn(B, T, 14, generator=torch.Generator().manual_seed(5), dtype=torch.float64)).to(dtype)
    val, grad = wave(dtype, njf, 7, PANDA_CHAIN, T, k, DT, support, accumulate, 0.7, spec, sph.numpy(), limits, x, g0)
    fine = torch.from_numpy(dense.interpolate(x.numpy(), k, DT))
    ref, _, gref, _ = G.oracle(fine, T, k, spec, sph=sph, weight=0.7, limits=limits, support=support)
    return val, grad, ref, gref + g0.double()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("T,k,support", [(2, 0, True), (6, 3, False), (64, 1, True), (65, 1, True), (66, 3, True)])
def test_kernel_text_matches_autograd_on_the_host(wave, dtype, T, k, support):
    val, grad, ref, gref = panda_case(wave, dtype, T, k, support)
    assert float(gref.abs().max()) > 0
    compare(val, grad, ref, gref, dtype, f"panda T={T} n_sub={k} support={int(support)}")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_generic_storage_interpolated_points_and_accumulate(wave, dtype):
    from tests.test_gpu_dense_cost import panda_terms
    import tests.test_gpu_dense_grad as G
    val, grad, ref, gref = panda_case(wave, dtype, 6, 3, True, njf=0)
    compare(val, grad, ref, gref, dtype, "generic storage")
    spec = panda_terms("sdf", num_interpolate=2, with_self=False)[0]
    val, grad, ref, gref = panda_case(wave, dtype, 6, 3, True, njf=0, B=5, spec=spec, limits=None, seed=G.SDF_SEED[("sdf", 2)])
    compare(val, grad, ref, gref, dtype, "sdf, 2 interpolated points")
    spec = [dict(kind="self", sigma=0.01, margin=0.08, num_interpolate=3)]
    val, grad, ref, gref = panda_case(wave, dtype, 6, 3, True, njf=0, spec=spec, limits=None)
    compare(val, grad, ref, gref, dtype, "self, 3 interpolated points")
    val, grad, ref, gref = panda_case(wave, dtype, 66, 1, True, accumulate=True)
    compare(val, grad, ref, gref, dtype, "accumulate, T=66")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("T,at", [(8, (1, 0, 3)), (66, (2, 65, 9)), (66, (0, 30, 0))])
def test_one_nan_poisons_its_trajectory_only_on_the_host(wave, dtype, T, at):
    from tests.test_gpu_dense_cost import DT, Q_LIM, SIGMA_LIM, V_LIM, arm_inputs, panda_terms, spheres
    x = arm_inputs(T, dtype, B=3)
    x[at] = float("nan")
    g0 = torch.ones(3, T, 14, dtype=dtype)
    val, grad = wave(dtype, 10, 7, PANDA_CHAIN, T, 1, DT, True, True, 0.7, panda_terms()[0], spheres().double().numpy(),
                     ((Q_LIM[0], Q_LIM[1]), V_LIM, SIGMA_LIM), x, g0)
    keep = [b for b in range(3) if b != at[0]]
    assert bool(torch.isnan(val[at[0]])) and bool(torch.isnan(grad[at[0]]).all())
    assert bool(torch.isfinite(val[keep]).all()) and bool(torch.isfinite(grad[keep]).all())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_limits_alone_without_a_chain_on_the_host(wave, dtype):
    from tests.test_gpu_dense_cost import planar_inputs
    T, k, dt = 66, 3, 0.02
    x = planar_inputs(T, dtype, 3, B=2)
    for limits in ((([-5., -4.], None), None, 0.5), ((None, [5., 4.]), None, 0.5), ((None, None), [10., 12.], 0.5)):
        val, grad = wave(dtype, 0, 2, [], T, k, dt, False, False, 0., [], None, limits, x, torch.zeros(2, T, 4, dtype=dtype))
        f = dense.interpolate(x.numpy(), k, dt).astype(np.float64)
        ref = torch.from_numpy(dense.limit_penalty(f, *limits))
        gref = torch.from_numpy(dense.hermite_pullback(dense.limit_penalty_grad(f, *limits), T, k, dt))
        assert float(ref.min()) > 0
        compare(val, grad, ref, gref, dtype, f"planar limits {limits[:2]}")
