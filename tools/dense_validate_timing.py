"""Timing of the dense trajectory check (sgpmp_validate, csrc/traj_dense.hip) on the MI355X, to record -- no rate is promised.

Per dtype (fp32, fp64), Panda chain, T = 64, 5 spheres, joint + velocity limits:
  * sgpmp_validate at n_sub = 0 and 4 on 1024 trajectories (a population of means) and on 131 072 (BASELINE configs[2]'s samples);
  * beside it sgpmp_cost_eval of the SAME batch in the same run -- the yardstick: the same forward-kinematics count per
    waypoint, so validate at n_sub = k is expected at roughly (k + 1) x;
  * the unfused composition (interpolate -> sgpmp_fk -> sgpmp_link_distances x 2 -> amin) at the largest batch whose
    frames and distance tables fit in free memory;
  * the kernels' VGPR count and private-segment (scratch) size, read from the gfx950 code object's metadata.
Times are HIP events around `reps` back-to-back calls (reps sized so that a window lasts >= 0.3 s where the call allows), after
3 warm-up calls per shape; 5 windows, median and spread reported.

usage: python tools/dense_validate_timing.py [--out profiles/r07/dense_validate.txt] [--no-resources]
"""
import argparse
import math
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LLVM = "/opt/rocm/lib/llvm/bin"


def kernel_resources():
    """[(kernel, vgprs, agprs, sgprs, scratch bytes, lds bytes)] of traj_dense.hip's code object (compiled here for gfx950)."""
    src = os.path.join(ROOT, "stoch_gpmp_amd", "csrc", "traj_dense.hip")
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "traj_dense.co")
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only",
                        "--no-gpu-bundle-output", "-c", src, "-o", obj], check=True, stderr=subprocess.DEVNULL)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", obj], check=True, capture_output=True,
                               text=True).stdout
    rows = []
    for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        blk = ".agpr_count:" + blk
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))     # noqa: E731
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.match(r"_Z\d+(\w+?_kernel)I([fd])Li(\d+)EE", name)          # <real, N> of the two kernel templates
        if m:
            name = f"{m.group(1)}<{'float' if m.group(2) == 'f' else 'double'}, {m.group(3)}>"
        rows.append((name, get("vgpr_count"), get("agpr_count"), get("sgpr_count"),
                     get("private_segment_fixed_size"), get("group_segment_fixed_size")))
    return rows


def timed(fn, torch, min_window_s=0.3, windows=5, max_reps=2000):
    """median / min / max milliseconds per call of fn() over `windows` event-timed windows"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    one = max(a.elapsed_time(b) * 1e-3, 1e-6)
    reps = int(min(max_reps, max(3, math.ceil(min_window_s / one))))
    per = []
    for _ in range(windows):
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) / reps)
    per.sort()
    return per[len(per) // 2], per[0], per[-1], reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "dense_validate.txt"))
    ap.add_argument("--no-resources", action="store_true")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    from stoch_gpmp_amd.robots.panda import PANDA_Q_LIMITS, PANDA_V_LIMITS
    from stoch_gpmp_amd.workloads import PANDA, hip_panda_cost, panda_spheres
    dev = torch.device("cuda:0")
    lines = [f"dense trajectory check: {torch.cuda.get_device_name(0)}, Panda chain (11 links), T = 64, 5 spheres, "
             "q and v limits; ms per call, median [min .. max] of 5 event-timed windows"]
    say = lambda s: (lines.append(s), print(s, flush=True))                        # noqa: E731
    T, n, dt = 64, 7, PANDA["dt"]
    for dtype in (torch.float32, torch.float64):
        ta = {"device": dev, "dtype": dtype}
        tag = "fp32" if dtype == torch.float32 else "fp64"
        cost = hip_panda_cost(PANDA, T, 1024, 128, ta)
        eng = cost._engine(dtype, dev)
        sph = torch.as_tensor(panda_spheres(5, 0)).to(**ta).reshape(-1, 4).contiguous()
        g = torch.Generator().manual_seed(1)
        q0, q1 = torch.tensor(PANDA["start_q"]), torch.tensor(PANDA["goal_q"])
        w = torch.linspace(0., 1., T).reshape(1, T, 1)
        for B in (1024, 131072):
            q = q0 + (q1 - q0) * w + 0.15 * torch.randn(B, T, n, generator=g)
            v = (q1 - q0) / ((T - 1) * dt) + 0.5 * torch.randn(B, T, n, generator=g)
            x = torch.cat([q, v], dim=-1).to(**ta).contiguous()
            costs = torch.empty(B, **ta)
            ms_c = timed(lambda: eng.cost_eval(x, spheres=sph, out=costs), torch)
            say(f"{tag} B={B:6d}  sgpmp_cost_eval ({eng.last_cost_kernel()}): {ms_c[0]:.4f} [{ms_c[1]:.4f} .. {ms_c[2]:.4f}] "
                f"({ms_c[3]} calls per window)")
            for k in (0, 4):
                ms = timed(lambda: eng.validate(x, k, dt, spheres=sph, q_limits=PANDA_Q_LIMITS, v_limits=PANDA_V_LIMITS), torch)
                fk = B * ((T - 1) * (k + 1) + 1)
                say(f"{tag} B={B:6d}  sgpmp_validate n_sub={k}: {ms[0]:.4f} [{ms[1]:.4f} .. {ms[2]:.4f}] ({ms[3]} calls per window)"
                    f" = {ms[0] / ms_c[0]:.2f} x cost_eval; {fk / ms[0] * 1e-6:.1f} G fine states / s")
        # the unfused composition, k = 4, at the largest batch that fits
        k, L, O, esz = 4, 11, sph.shape[0], 4 if dtype == torch.float32 else 8
        Tf = (T - 1) * (k + 1) + 1
        per_traj = Tf * (2 * n + L * 16 + L * O + 2 * L * L + 2) * esz      # dense states, frames, two tables (+ the masked copy)
        free = torch.cuda.mem_get_info()[0]
        Bc = 131072
        while Bc > 1 and per_traj * Bc * 1.3 > free:
            Bc //= 2
        xc = x[:Bc].contiguous()
        mask = torch.ones(L, L, dtype=torch.bool, device=dev).tril(-2)

        def composed():
            fine = eng.interpolate(xc, k, dt)
            frames = eng.fk(fine[..., :n].reshape(-1, n).contiguous())
            d_obs = eng.link_distances(frames, sph, mode=0).reshape(Bc, -1).amin(dim=1)
            d_self = eng.link_distances(frames, None, mode=0).reshape(Bc, Tf, L, L)
            d_self = torch.where(mask, d_self, torch.full_like(d_self[:1, :1], float("inf"))).reshape(Bc, -1).amin(dim=1)
            return d_obs, d_self
        ms_u = timed(composed, torch, max_reps=20)
        ms_f = timed(lambda: eng.validate(xc, k, dt, spheres=sph), torch)
        say(f"{tag} B={Bc:6d}  unfused interpolate -> fk -> link_distances x 2 -> amin, n_sub=4: {ms_u[0]:.3f} "
            f"[{ms_u[1]:.3f} .. {ms_u[2]:.3f}]; frames alone {Bc * Tf * L * 16 * esz / 1e9:.2f} GB "
            f"(free memory {free / 1e9:.0f} GB); sgpmp_validate of the same batch and columns: {ms_f[0]:.4f} "
            f"= {ms_u[0] / ms_f[0]:.1f} x faster")
        del x, xc, costs
        torch.cuda.empty_cache()
    if not args.no_resources:
        say("kernel resources (gfx950 code object metadata): vgprs, agprs, sgprs, private segment bytes / lane, static LDS bytes")
        for name, vg, ag, sg, scratch, lds in kernel_resources():
            if re.search(r"<(float|double), (2|7)>", name):
                say(f"  {name.split('(')[0]}: {vg} vgprs, {ag} agprs, {sg} sgprs, private segment {scratch}"
                    f"{' (SPILLS)' if scratch else ' (no spill)'}, static LDS {lds}"
                    f"{' (+ dynamic: links x 3 x 64 reals)' if name.startswith('validate') else ''}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
