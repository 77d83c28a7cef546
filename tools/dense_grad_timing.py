"""Timing of the continuous-time cost gradient (sgpmp_dense_cost_grad, csrc/traj_dense.hip) on the MI355X, to record -- no rate is
promised: nobody had measured this kernel.

Per dtype (fp32, fp64), Panda chain, T = 64, self + 5 rbf spheres, 131 072 trajectories (BASELINE configs[2]'s samples),
n_sub = 1 and 4, all in one process:
  * sgpmp_dense_cost_grad, support = 0 (the same fine states as sgpmp_dense_cost: the inserted ones) and support = 1;
  * beside it sgpmp_dense_cost of the same batch on its generic path (option force_generic_fk: the same forward kinematics through
    LDS, the yardstick the ratio is stated against) and on its built-in path;
  * per call and per evaluated fine state, and the ratio gradient / generic value.
Times are HIP events around back-to-back calls after warm-up (tools/dense_validate_timing.py: timed), 5 windows, median and spread;
clocks as the box runs them (nothing pinned).
--resources-only (needs no GPU) appends VGPRs, AGPRs, scratch, static LDS and waves per SIMD of every instantiation, from the
compiler's -Rpass-analysis=kernel-resource-usage remarks on traj_dense.hip, with the launch's dynamic LDS beside them.

usage: python tools/dense_grad_timing.py [--out profiles/r09/dense_grad.txt] [--batch 131072] [--resources-only]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dense_cost_timing import panda_descriptors  # noqa: E402
from dense_validate_timing import timed  # noqa: E402


def resource_lines():
    src = os.path.join(ROOT, "stoch_gpmp_amd", "csrc", "traj_dense.hip")
    with tempfile.TemporaryDirectory() as tmp:
        err = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only",
                              "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "traj_dense.co")],
                             check=True, capture_output=True, text=True).stderr
    out = ["kernel resources (-Rpass-analysis=kernel-resource-usage, gfx950): VGPRs, AGPRs, scratch bytes / lane, waves per SIMD by "
           "registers; dynamic LDS of the launch for the Panda (11 links): 11 x 3 x 64 doubles of forces + 21 x 3 x 64 reals of points and axes"]
    get = lambda key, blk: int(re.search(r"%s: (\d+)" % re.escape(key), blk).group(1))     # noqa: E731
    for blk in err.split("Function Name: ")[1:]:
        m = re.match(r"_Z\d+dense_cost_grad_kernelI([fd])Li(\d+)ELi(n?\d+)E", blk)
        if not m:
            continue
        real, nj = ("float", 4) if m.group(1) == "f" else ("double", 8), m.group(3)
        path = {"n1": "no FK", "0": "generic"}.get(nj, f"{nj} joints")
        lds = 0 if nj == "n1" else 11 * 3 * 64 * 8 + 21 * 3 * 64 * real[1]
        scratch = get("ScratchSize [bytes/lane]", blk)
        out.append(f"  dense_cost_grad_kernel<{real[0]}, n = {m.group(2)}, {path}>: {get('VGPRs', blk)} VGPRs, {get('AGPRs', blk)} AGPRs, "
                   f"scratch {scratch}{' (SPILLS)' if scratch else ''}, {get('Occupancy [waves/SIMD]', blk)} waves / SIMD by registers, "
                   f"static LDS {get('LDS Size [bytes/block]', blk)}, dynamic LDS {lds}"
                   + (f" = {160 * 1024 // lds} one-wave workgroups per CU by LDS" if lds else ""))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "dense_grad.txt"))
    ap.add_argument("--batch", type=int, default=131072)
    ap.add_argument("--resources-only", action="store_true", help="append the compiler's figures to --out; needs no GPU")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.resources_only:
        with open(args.out, "a") as f:
            f.write("\n".join(resource_lines()) + "\n")
        return
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    from stoch_gpmp_amd.engine import Engine
    from stoch_gpmp_amd.robots.panda_chain import PANDA_CHAIN
    from stoch_gpmp_amd.workloads import PANDA, panda_spheres
    dev = torch.device("cuda:0")
    lines = [f"continuous-time cost gradient: {torch.cuda.get_device_name(0)}, Panda chain (11 links), T = 64, self + 5 rbf spheres, no "
             "limits; ms per call, median [min .. max] of 5 event-timed windows, one process, clocks as the box runs them (no clock "
             "pinned); fp32 and fp64 as tagged"]
    say = lambda s: (lines.append(s), print(s, flush=True))                        # noqa: E731
    T, n, dt, B = 64, 7, PANDA["dt"], args.batch
    for dtype in (torch.float32, torch.float64):
        ta = {"device": dev, "dtype": dtype}
        tag = "fp32" if dtype == torch.float32 else "fp64"

        def engine(generic=False):
            eng = Engine(n, T, 0, 1, tensor_args=ta)
            eng.set_fk(PANDA_CHAIN, codegen=False)
            if generic:
                eng.set_option("force_generic_fk", 1)
            eng.set_costs(panda_descriptors(T, ta))
            return eng
        fast, slow = engine(), engine(generic=True)
        sph = torch.as_tensor(panda_spheres(5, 0)).to(**ta).reshape(-1, 4).contiguous()
        g = torch.Generator().manual_seed(1)
        q0, q1 = torch.tensor(PANDA["start_q"]), torch.tensor(PANDA["goal_q"])
        w = torch.linspace(0., 1., T).reshape(1, T, 1)
        q = q0 + (q1 - q0) * w + 0.15 * torch.randn(B, T, n, generator=g)
        v = (q1 - q0) / ((T - 1) * dt) + 0.5 * torch.randn(B, T, n, generator=g)
        x = torch.cat([q, v], dim=-1).to(**ta).contiguous()
        costs, grad = torch.empty(B, **ta), torch.empty(B, T, 2 * n, **ta)
        for k in (1, 4):
            ins = B * (T - 1) * k
            ms_gen = timed(lambda: slow.dense_cost(x, k, dt, spheres=sph, out=costs), torch)
            say(f"{tag} B={B} n_sub={k}  sgpmp_dense_cost generic ({slow.last_dense_kernel()}): {ms_gen[0]:.4f} [{ms_gen[1]:.4f} .. "
                f"{ms_gen[2]:.4f}] ms = {ms_gen[0] / ins * 1e9:.1f} ps per inserted state")
            ms_cg = timed(lambda: fast.dense_cost(x, k, dt, spheres=sph, out=costs), torch)
            say(f"{tag} B={B} n_sub={k}  sgpmp_dense_cost built-in ({fast.last_dense_kernel()}): {ms_cg[0]:.4f} [{ms_cg[1]:.4f} .. "
                f"{ms_cg[2]:.4f}] ms = {ms_cg[0] / ins * 1e9:.1f} ps per inserted state")
            for eng, path in ((fast, "chain length compiled in"), (slow, "generic")):
                for support in (False, True):
                    states = ins + (B * (T - 1) if support else 0)
                    ms = timed(lambda: eng.dense_cost_grad(x, k, dt, spheres=sph, support=support, grad=grad), torch)
                    say(f"{tag} B={B} n_sub={k}  sgpmp_dense_cost_grad support={int(support)} {path} ({eng.last_dense_kernel()}): "
                        f"{ms[0]:.4f} [{ms[1]:.4f} .. {ms[2]:.4f}] ms = {ms[0] / states * 1e9:.1f} ps per evaluated state"
                        + (f" = {ms[0] / ms_gen[0]:.2f} x the generic value kernel, {ms[0] / ms_cg[0]:.2f} x the built-in one"
                           if not support else ""))
        del x, costs, grad
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
