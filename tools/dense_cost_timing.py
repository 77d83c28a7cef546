"""Timing of the continuous-time cost (sgpmp_dense_cost, csrc/traj_dense.hip) on the MI355X, to record -- no rate is promised.

Per dtype (fp32, fp64), Panda chain, T = 64, 5 spheres (rbf) + self term, joint and velocity limits, 131 072 trajectories
(BASELINE configs[2]'s samples), n_sub = 1 and 4:
  * sgpmp_dense_cost on the built-in chain code and on the generic path (option force_generic_fk), per call and per inserted state;
  * beside it sgpmp_cost_eval of the same batch, per waypoint -- the same fields on the same chain code: the per-state work the
    built-in path should be close to -- and the ratio of the two;
  * the unfused composition: sgpmp_interpolate, then sgpmp_cost_eval of the fine trajectories on a T_f-long context, minus the
    support part (sgpmp_cost_eval of the T support waypoints);
  * sgpmp_validate of the same batch (the generic path's sibling: the same forward kinematics per fine state);
  * ms per step() at BASELINE configs 2 and 3 with the option off (unchanged) and with n_sub = 4;
  * the kernels' VGPR count and private-segment (scratch) size, read from the gfx950 code object's metadata.
Times are HIP events around back-to-back calls in one process after warm-up (tools/dense_validate_timing.py: timed), 5 windows,
median and spread.

usage: python tools/dense_cost_timing.py [--out profiles/r08/dense_cost.txt] [--no-resources] [--no-steps] [--resources-only]
"""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dense_validate_timing import kernel_resources, timed  # noqa: E402


def panda_descriptors(T, ta):
    """The collision terms of the Panda workload (self + rbf spheres) alone, as set_costs takes them: the terms sgpmp_dense_cost
    evaluates, so that sgpmp_cost_eval of this program is the like-for-like yardstick per waypoint."""
    from stoch_gpmp_amd.costs.fields import LinkDistanceField, LinkSelfDistanceField
    from stoch_gpmp_amd.workloads import PANDA as c
    return [LinkSelfDistanceField(margin=c["self_margin"]).descriptor(c["sigma_self"]),
            LinkDistanceField(field_type="rbf").descriptor(c["sigma_coll"])]


def resource_lines():
    out = ["kernel resources (gfx950 code object metadata): vgprs, agprs, sgprs, private segment bytes / lane, static LDS bytes"]
    for name, vg, ag, sg, scratch, lds in kernel_resources():
        m = re.match(r"_Z\d+dense_cost_kernelI([fd])Li(\d+)ELi(\d)E", name)
        if m and m.group(2) in ("2", "6", "7"):
            mode = {"0": "no FK", "1": "generic FK", "2": "generated chain"}[m.group(3)]
            out.append(f"  dense_cost_kernel<{'float' if m.group(1) == 'f' else 'double'}, {m.group(2)}, {mode}>: {vg} vgprs, {ag} agprs, "
                       f"{sg} sgprs, private segment {scratch}{' (SPILLS)' if scratch else ' (no spill)'}, static LDS {lds}"
                       f"{' (+ dynamic: points x 3 x 64 reals)' if m.group(3) == '1' else ''}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "dense_cost.txt"))
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--batch", type=int, default=131072)
    ap.add_argument("--resources-only", action="store_true", help="append the code object's figures to --out; needs no GPU")
    args = ap.parse_args()
    if args.resources_only:
        with open(args.out, "a") as f:
            f.write("\n".join(resource_lines()) + "\n")
        return
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    from stoch_gpmp_amd.engine import Engine
    from stoch_gpmp_amd.robots.panda import PANDA_Q_LIMITS, PANDA_V_LIMITS
    from stoch_gpmp_amd.robots.panda_chain import PANDA_CHAIN
    from stoch_gpmp_amd.workloads import PANDA, panda_spheres
    dev = torch.device("cuda:0")
    lines = [f"continuous-time cost: {torch.cuda.get_device_name(0)}, Panda chain (11 links), T = 64, self + 5 rbf spheres, "
             "q and v limits; ms per call, median [min .. max] of 5 event-timed windows, one process, clocks as the box runs them "
             "(no clock pinned); fp32 and fp64 as tagged"]
    say = lambda s: (lines.append(s), print(s, flush=True))                        # noqa: E731
    T, n, dt, B = 64, 7, PANDA["dt"], args.batch
    lim = dict(q_limits=PANDA_Q_LIMITS, v_limits=PANDA_V_LIMITS, sigma_limit=0.1)
    for dtype in (torch.float32, torch.float64):
        ta = {"device": dev, "dtype": dtype}
        tag = "fp32" if dtype == torch.float32 else "fp64"

        def engine(T_ctx, generic=False):
            eng = Engine(n, T_ctx, 0, 1, tensor_args=ta)
            eng.set_fk(PANDA_CHAIN, codegen=False)
            if generic:
                eng.set_option("force_generic_fk", 1)
            eng.set_costs(panda_descriptors(T_ctx, ta))
            return eng
        fast, slow = engine(T), engine(T, generic=True)
        sph = torch.as_tensor(panda_spheres(5, 0)).to(**ta).reshape(-1, 4).contiguous()
        g = torch.Generator().manual_seed(1)
        q0, q1 = torch.tensor(PANDA["start_q"]), torch.tensor(PANDA["goal_q"])
        w = torch.linspace(0., 1., T).reshape(1, T, 1)
        q = q0 + (q1 - q0) * w + 0.15 * torch.randn(B, T, n, generator=g)
        v = (q1 - q0) / ((T - 1) * dt) + 0.5 * torch.randn(B, T, n, generator=g)
        x = torch.cat([q, v], dim=-1).to(**ta).contiguous()
        costs = torch.empty(B, **ta)
        ms_c = timed(lambda: fast.cost_eval(x, spheres=sph, out=costs), torch)
        per_wp = ms_c[0] / (B * T) * 1e9
        say(f"{tag} B={B}  sgpmp_cost_eval, collision terms only ({fast.last_cost_kernel()}): {ms_c[0]:.4f} [{ms_c[1]:.4f} .. {ms_c[2]:.4f}] ms"
            f" = {per_wp:.1f} ps per waypoint")
        for k in (1, 4):
            ins = B * (T - 1) * k
            for eng, path in ((fast, "built-in"), (slow, "generic")):
                for what, kw in (("collision + limits", lim), ("collision only", {})):
                    ms = timed(lambda: eng.dense_cost(x, k, dt, spheres=sph, out=costs, **kw), torch)
                    per = ms[0] / ins * 1e9
                    say(f"{tag} B={B}  sgpmp_dense_cost n_sub={k} {path} ({eng.last_dense_kernel()}), {what}: {ms[0]:.4f} "
                        f"[{ms[1]:.4f} .. {ms[2]:.4f}] ms = {per:.1f} ps per inserted state = {per / per_wp:.2f} x cost_eval's "
                        f"per waypoint")
            ms_v = timed(lambda: slow.validate(x, k, dt, spheres=sph, q_limits=PANDA_Q_LIMITS, v_limits=PANDA_V_LIMITS), torch)
            say(f"{tag} B={B}  sgpmp_validate n_sub={k} (all fine states, generic FK): {ms_v[0]:.4f} [{ms_v[1]:.4f} .. {ms_v[2]:.4f}] ms")
            # the unfused composition at the parent commit: interpolate, sweep the fine trajectories, take the support part off
            Tf = (T - 1) * (k + 1) + 1
            long = engine(Tf)
            cf = torch.empty(B, **ta)

            def composed():
                fine = fast.interpolate(x, k, dt)
                long.cost_eval(fine, spheres=sph, out=cf)
                fast.cost_eval(x, spheres=sph, out=costs)
                return cf - costs
            ms_u = timed(composed, torch, max_reps=50)
            ms_d = timed(lambda: fast.dense_cost(x, k, dt, spheres=sph, out=costs), torch)
            say(f"{tag} B={B}  unfused interpolate -> cost_eval on a T_f = {Tf} context ({long.last_cost_kernel()}) - cost_eval, "
                f"n_sub={k}: {ms_u[0]:.4f} [{ms_u[1]:.4f} .. {ms_u[2]:.4f}] ms, fine states {B * Tf * 2 * n * x.element_size() / 1e9:.2f} GB; "
                f"sgpmp_dense_cost built-in, collision only: {ms_d[0]:.4f} ms = {ms_u[0] / ms_d[0]:.2f} x faster")
            del long, cf
        del x, costs
        torch.cuda.empty_cache()
    if not args.no_steps:
        import bench
        for label, spec in (("config 2 (planar 256 x 64 x 128, fp32)", dict(workload="planar", P_local=256, S=64, T=128, goals=4)),
                            ("config 3 (Panda 1024 x 128 x 64, fp32)", dict(workload="panda", P_local=1024, S=128, T=64))):
            panda = spec["workload"] == "panda"
            for setting in [None, dict(n_sub=4)] + ([dict(n_sub=4, **lim)] if panda else []):
                pl, obs, _ = bench.build_planner(torch, dtype=torch.float32, dev=dev, dense_cost=setting, **spec)
                ms = timed(lambda: pl.step(**obs), torch)
                say(f"{label}  step() with dense_cost {'off' if setting is None else 'n_sub = %d, %s' % (setting['n_sub'], 'with limits' if 'q_limits' in setting else 'no limits')}: {ms[0]:.4f} "
                    f"[{ms[1]:.4f} .. {ms[2]:.4f}] ms per step"
                    + ("" if setting is None else f" ({pl._engine.last_dense_kernel()})"))
                del pl
                torch.cuda.empty_cache()
    if not args.no_resources:
        for line in resource_lines():
            say(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
