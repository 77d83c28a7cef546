// Which launches does a particle range's step run?  Host code only: this file instantiates no kernel (the kernel sources are
// included for the limits they define -- tile sizes, LDS tables -- and nothing else).
//
// plan_step is the ONE place that knows the conditions: api.hip asks it once per launch sequence, launch_fused_step
// (cost_sweep.hip) enqueues what it says, and tests/host_asan/plan_table.cpp holds it to a table of shapes on the CPU.
#include <cstring>

#include "chain_code_generated.h"
#include "rng.h"
#include "sgpmp_internal.h"
#include "update_common.h"
#include "cost_device.h"
#include "cost_host.h"
#include "cost_sweep_kernel.inc"
#include "cost_sweep_dual.inc"
#include "fused_step.inc"
#include "fused_planar.inc"
#include "fused_planar_seg.inc"

// Shape of the lane-per-sample launch (fused_planar_seg.inc): waypoints per wave, 0 when (S, T, n) does not fit.
// Never a function of the particle count.
static int planar_seg_len(int n, int T, int S, const SgpmpToggles& tg) {
    if (tg.no_planar_seg || S % 64 != 0) return 0;
    const int L = T <= 128 ? 8 : 16;
    if (T % L != 0 || T / L > 16 || (L == 16 && n != 2)) return 0;
    return L;
}

static size_t planar_seg_lds(int n, int T, int L) {
    const int G = T / L;
    return (size_t)G * 64 * (16 * n + 8) + (size_t)G * 64 * 20 * sizeof(float) + (size_t)G * 16;
}

// the program as named fields, with what every one-launch step asks of them
template <typename real>
static bool flat_fits(const CostProgram& prog, const PriorDev& prior, int S, FlatProg<real>& F) {
    if (!make_flat<real>(prog, F)) return false;
    if (F.has_goal && F.goal.rows_per_goal % S != 0) return false;      // (a particle has one goal)
    if (F.has_gp && (real)prior.dt != F.gp.dt) return false;             // IS term and GP factors share Phi
    return true;
}

int fused_full_variant(const StepPlan& plan, const CostProgram& prog, const SgpmpToggles& tg) {
    if (tg.fused_generic || plan.family != STEP_CHAIN || plan.ragged || plan.small || plan.regen_recipe != 0) return 0;
    // exactly the four terms, one of each kind (an end-effector term is a fifth; the grid term never reaches a chain plan)
    if (prog.n_terms != 4 || prog.n_ee != 0) return 0;
    bool gp = false, goal = false, self = false, sph = false;
    for (int i = 0; i < prog.n_terms; ++i) {
        const CostTerm& t = prog.terms[i];
        if (t.n_interp > 0) return 0;
        if (t.kind == SGPMP_COST_GP && !gp) gp = (t.flags & SGPMP_FLAG_GP_START) != 0;
        else if (t.kind == SGPMP_COST_GOAL_PRIOR && !goal) goal = true;
        else if (t.kind == SGPMP_COST_SELF && !self) self = true;
        else if (t.kind == SGPMP_COST_SPHERES && !sph) sph = true;
        else return 0;
    }
    if (!(gp && goal && self && sph)) return 0;
    return plan.partials ? 2 : 1;
}

StepPlan plan_step(const StepShape& shape, const StepWants& wants, const PriorDev& prior, const CostProgram& prog,
                   const ChainDev& chain, const SgpmpToggles& tg) {
    using CCp = ChainCode_panda;
    const int dtype = shape.dtype, n = shape.n, T = shape.T, S = shape.S, P = shape.P;
    StepPlan none;
    std::memset(&none, 0, sizeof(none));
    none.shape = shape; none.max_iters = none.iters = 1; none.kernel = "";
    // one item per wave measured fastest at config 3 (4096 workgroups 0.216 ms/iteration, 2048: 0.219,
    // 1024: 0.227): the per-workgroup set-up is small and the hardware dispatcher balances better than
    // a grid-stride loop; the loop stays for batches beyond 2^20 items and for the k3_blocks switch
    none.block_cap = tg.k3_blocks > 0 ? tg.k3_blocks : 1LL << 18;
    StepPlan p = none;
    if (wants.eps || tg.no_fused_step || tg.no_flat_program || !prior.isotropic) return none;
    if ((dtype != SGPMP_F32 && dtype != SGPMP_F64) || T < 2 || P < 1 || S < 1) return none;
    if ((long long)P * S + (long long)shape.offset * S >= (1LL << 31)) return none;       // row indices are 32-bit
    bool interp = false;
    for (int i = 0; i < prog.n_terms; ++i) interp = interp || prog.terms[i].n_interp > 0;
    if (dtype == SGPMP_F64) {
        // fp64 contexts: sampler + sweep as fused_step_f64_kernel (cost_sweep_kernel.inc: GEN) -- one wave per trajectory, lane =
        // waypoint, the recurrence as a scan over the lanes; FLAT programs on the positions themselves (n = 2, 3) or on the chain
        // code built with the library
        FlatProg<double> F;
        if (!prior.scan64 || interp || !flat_fits<double>(prog, prior, S, F)) return none;
        if (!prog.needs_fk) {
            if (F.has_self || F.has_sph || (n != 2 && n != 3)) return none;
        } else if (tg.no_chain_codegen || tg.force_generic_fk || !chain.plan.fast || chain.plan.codegen_id != 1 || n != CCp::N || F.has_grid) {
            return none;
        }
        p.family = STEP_F64;
        p.mixed = tg.f64_fields_f32 && prog.needs_fk && shape.n_spheres <= SGPMP_SPH_LDS;
        p.kernel = p.mixed ? "fused_step_f64_mixed_kernel" : "fused_step_f64_kernel";
    } else {
        // (S: the chain-code launch masks the rows of a particle's last group of 8 -- round 4; the planar launches want whole groups)
        // (T: the chain-code launch masks the columns and cost lanes past T in the last chunk of 16 -- T even: 16-byte rows)
        FlatProg<float> F;
        if (T % 2 != 0 || !flat_fits<float>(prog, prior, S, F) || (F.has_goal && F.goal.dim0 > SGPMP_FUSED_GOALS)) return none;
        p.ragged = S % SGPMP_FUSED_SPW != 0 || T % SGPMP_FUSED_TC != 0;
        // what a store-free step that REGENERATES rows in update_kernel needs, beyond a recipe: that regenerating pays.
        // update_kernel's regeneration is a dependent chain of ~6.5 us per particle (T = 64) that a small step cannot hide, while what
        // the launch saves grows with the bytes it does not write.  Measured break-even on MI355X (tools/store_free_sizes.py,
        // profiles/r05/store_free_sizes.txt: Panda, S = 64 .. 512, T = 32 and 64, P = 16 .. 2048): 176 MB of samples per step at
        // T = 64, ~88 MB at T = 32 -- i.e. 2.75 MB per waypoint; below it a store-free step ran 4 .. 20 % SLOWER than a storing one,
        // so the step stores (same results either way: the choice is a function of the shape).
        auto regen = [&](int recipe) {
            const long long waypoint_bytes = (long long)shape.particles_total * S * 2 * n * (long long)sizeof(float);
            const long long min_bytes = tg.store_free_min_bytes > 0 ? tg.store_free_min_bytes : SGPMP_STORE_FREE_BREAK_EVEN;
            return wants.no_samples && waypoint_bytes >= min_bytes && update_regen_rows(dtype, n, T, S, recipe) > 0 ? recipe : 0;
        };
        if (!prog.needs_fk && prog.n_ee == 0) {
            // no link fields: GP / goal prior / occupancy grid on the positions themselves
            if (p.ragged || F.has_self || F.has_sph || (n != 2 && n != 3) || T > SGPMP_PLANAR_TMAX) return none;
            // lane = sample, wave = time segment (fused_planar_seg.inc: 1024-thread workgroups, one per particle and 64 samples) where
            // the shape allows -- picked from (S, T, n) alone -- and the grid fits; else 8 samples per wave through an LDS tile
            p.L = planar_seg_len(n, T, S, tg);
            p.seg_table = p.L == 8 ? 3 : 4;
            const bool seg = p.L != 0 && (long long)P * S / 64 <= (1LL << 20);
            p.family = seg ? STEP_PLANAR_SEG : STEP_PLANAR_TILE;
            p.kernel = seg ? "fused_planar_seg_kernel" : "fused_planar_kernel";
            if (seg) {
                p.seg_lds = (unsigned)planar_seg_lds(n, T, p.L);
                // Store-free step of a problem whose particles have exactly one workgroup's 64 samples: the UPDATE runs inside the
                // launch (seg_update) -- no sample store, no update_kernel, no regeneration: one launch per iteration
                const size_t tail_lds = (size_t)T * 2 * n * sizeof(float);
                p.update_in_launch = wants.no_samples && wants.update_in_launch_ok && S == 64 && !tg.no_planar_tail &&
                                     tail_lds + p.seg_lds <= 160 * 1024;
                if (p.update_in_launch) p.seg_lds += (unsigned)tail_lds;
                // ... and ONE launch can run several of them (PERSIST): instantiated for n = 2 with segments of 8 waypoints -- BASELINE
                // configs[1]'s shape: 110 vector registers.  Segments of 16 and n = 3 hold 32 / 48 waypoint values per lane: their
                // single-step launches use 118 / 114 of the 128 registers a 1024-thread workgroup's waves can have, and the loop's few
                // carried values pushed 21 / 19 registers into scratch (tools/audit_asm_loads.py refuses scratch in these kernels) --
                // those shapes keep one launch per iteration.  A launch runs persist_max_iters iterations at most -- 2048: ~25 ms at
                // BASELINE configs[1], far below anything a driver would call a hang.
                if (p.update_in_launch && !tg.no_persist_planar && n == 2 && p.L == 8)
                    p.max_iters = tg.persist_max_iters >= 2 ? (int)(tg.persist_max_iters < 0x7fffffff ? tg.persist_max_iters : 0x7fffffff) : 2048;
                // (regenerating rows: built, bit-identical, and measured slower store-free at config 2 -- its update kernel is not hidden
                // under another chain's launch, and regenerating a row costs it more than the launch saves: opt-in)
                if (!p.update_in_launch && tg.planar_store_free) p.regen_recipe = regen(2);
            }
        } else {
            if (tg.no_dual_sweep || tg.no_chain_codegen || tg.force_generic_fk || !chain.plan.fast || F.has_grid) return none;
            if (chain.plan.codegen_id == 1) { if (n != CCp::N) return none; }               // the chain built with the library
            else if (chain.plan.codegen_id != 2 || !chain.rtc || n > 7) return none;         // ... or compiled at run time (sgpmp_set_fk_codegen)
            if (shape.n_spheres > SGPMP_FUSED_SPH || interp) return none;
            p.field_type = F.has_sph ? (F.sph.flags & 15) : SGPMP_FIELD_RBF;
            // a SMALL step -- fewer items than SIMDs: every wave of the one-wave-per-item launch would sit alone on its SIMD for as long
            // as one item takes one wave (~20 us) -- goes out with one WORKGROUP per item instead, its four waves on the item's chunks
            // side by side (fused_step.inc: LAT; same samples and costs, bit for bit).  Up to two workgroups per CU for shapes on the
            // launch's 8 x 16 grid (253 registers, 57 KB of LDS: two per SIMD set), one for the others (the masked instantiation needs
            // 262 registers): beyond, a second round of workgroups costs what the other launch does in one (tools/small_step_sizes.py).
            // (judged on the WHOLE problem -- all ranks' particles, both halves of a two-chain step -- so that a shard takes the launch
            // its unsharded run takes)
            const long long small_items = tg.small_step_items > 0 ? tg.small_step_items : p.ragged ? 256 : 512;
            const long long items_global = (long long)(shape.particles_global > 0 ? shape.particles_global : P) * ((S + SGPMP_FUSED_SPW - 1) / SGPMP_FUSED_SPW);
            p.small = !tg.no_small_step && items_global <= small_items && (T + SGPMP_FUSED_TC - 1) / SGPMP_FUSED_TC <= 16;
            p.family = STEP_CHAIN;
            p.kernel = p.small ? "fused_step_small_kernel" : "fused_step_kernel";
            if (chain.plan.codegen_id == 2) {           // this chain's kernels are compiled at run time (chain_rtc.hip), on first use
                p.rtc_fn = rtc_kernel((RtcChain*)chain.rtc, p.field_type, false, p.ragged, p.small);
                if (!p.rtc_fn) return none;
                p.family = STEP_CHAIN_RTC;
                p.kernel = p.small ? "fused_step_small_kernel (run-time chain code)" : "fused_step_kernel (run-time chain code)";
            }
            // costs complete inside the launch (ee_goal_kernel reads the rows): softmax partials for the dense-weight regime of the
            // update, and the store-free form
            if (prog.n_ee == 0) {
                p.partials = !tg.no_dense_partials && (T * 2 * n) % 4 == 0;
                p.regen_recipe = regen(1);
            }
            p.full = fused_full_variant(p, prog, tg);
        }
    }
    // The step's end-effector goal term goes INTO update_kernel (update_common.h: EeFold) when it is the only one and the kernel's
    // scratch has room: one launch less per iteration (the term is a few hundred flops per trajectory; as a launch of its own it
    // cost 6 us of the reference's Panda example's 24); else ee_goal_kernel in front of update_kernel
    if (prog.n_ee > 0)
        p.ee = !tg.no_ee_fold && prog.n_ee == 1 && update_ee_fold_fits(dtype, n, T, S) ? STEP_EE_FOLD : STEP_EE_LAUNCH;
    if (wants.iters > 1 && wants.iters <= p.max_iters) p.iters = wants.iters;
    return p;
}
