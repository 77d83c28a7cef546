// The arguments of plan_step (csrc/step_plan.hip) for a case given as a row of small integers: shapes, a cost program, a chain,
// one development switch.  TEST INFRASTRUCTURE (plan_table.cpp; tests/test_cpu_host.py).
#pragma once
#include <cstdint>
#include <cstring>

#include "sgpmp_internal.h"

struct PlanCase {
    int dtype, n, T, S, P, offset, n_spheres, particles_total, particles_global;
    int prog, chain, toggle;      // ProgKind, ChainKind, index into kPlanToggles
    long long min_bytes;          // SgpmpToggles::store_free_min_bytes
    int eps, no_samples, update_ok, iters;   // StepWants
};

enum ProgKind {
    PROG_PLANAR,        // GP + goal prior
    PROG_PLANAR_GRID,   // + occupancy grid
    PROG_PANDA,         // GP + goal prior + self-distance + spheres (rbf)
    PROG_PANDA_SDF,     // ... spheres as sdf
    PROG_PANDA_EE,      // PANDA + one end-effector goal term
    PROG_PANDA_EE2,     // PANDA + two
    PROG_PANDA_INTERP,  // PANDA with interpolated points (num_interpolate > 0)
    PROG_TWO_GP,        // a second term of one kind
    PROG_CHAIN_GRID,    // PANDA + a grid term
    PROG_GP_DT,         // PLANAR whose GP factor has another dt than the prior
    PROG_EE_ONLY,       // PLANAR + one end-effector goal term (no link field)
    PROG_GOALS15,       // PANDA with more goals than the fused launch stages
    PROG_GOAL_ROWS,     // PLANAR whose goals do not change at particle boundaries
    PROG_COUNT
};
enum ChainKind {
    CHAIN_NONE,         // codegen_id 0
    CHAIN_PANDA,        // 1: the chain code built with the library
    CHAIN_RTC,          // 2: compiled at run time, kernels available
    CHAIN_RTC_NOKERNEL, // 2: ... the run-time function is null
    CHAIN_RTC_NULL,     // 2 without an RtcChain
    CHAIN_SLOW,         // 1, not revolute-first
    CHAIN_COUNT
};
// one switch per case; the last entry is not a switch: a prior that is not isotropic
static const struct { const char* name; int SgpmpToggles::*flag; long long SgpmpToggles::*num; long long value; } kPlanToggles[] = {
    {"-", nullptr, nullptr, 0},
    {"no_fused_step", &SgpmpToggles::no_fused_step, nullptr, 1}, {"no_flat_program", &SgpmpToggles::no_flat_program, nullptr, 1},
    {"no_chain_codegen", &SgpmpToggles::no_chain_codegen, nullptr, 1}, {"force_generic_fk", &SgpmpToggles::force_generic_fk, nullptr, 1},
    {"no_dual_sweep", &SgpmpToggles::no_dual_sweep, nullptr, 1}, {"no_planar_seg", &SgpmpToggles::no_planar_seg, nullptr, 1},
    {"no_planar_tail", &SgpmpToggles::no_planar_tail, nullptr, 1}, {"planar_store_free", &SgpmpToggles::planar_store_free, nullptr, 1},
    {"no_persist_planar", &SgpmpToggles::no_persist_planar, nullptr, 1}, {"no_small_step", &SgpmpToggles::no_small_step, nullptr, 1},
    {"no_dense_partials", &SgpmpToggles::no_dense_partials, nullptr, 1}, {"no_ee_fold", &SgpmpToggles::no_ee_fold, nullptr, 1},
    {"f64_fields_f32", &SgpmpToggles::f64_fields_f32, nullptr, 1}, {"persist_max_iters=7", nullptr, &SgpmpToggles::persist_max_iters, 7},
    {"small_step_items=64", nullptr, &SgpmpToggles::small_step_items, 64}, {"k3_blocks=100", nullptr, &SgpmpToggles::k3_blocks, 100},
    {"prior not isotropic", nullptr, nullptr, 0},
};
static const int kPlanToggleCount = (int)(sizeof(kPlanToggles) / sizeof(kPlanToggles[0]));

struct PlanArgs {
    StepShape shape; StepWants wants; PriorDev prior; CostProgram prog; ChainDev chain; SgpmpToggles tg;
    int rtc_available;            // what ChainDev::rtc points to: the stand-in rtc_kernel reads it
};

static inline void plan_case_args(const PlanCase& k, PlanArgs& a) {
    static double table[64];      // every device table the plan only passes on
    std::memset(&a, 0, sizeof(a));
    a.shape = {k.dtype, k.n, k.T, k.S, k.n_spheres, k.P, k.offset, k.particles_total, k.particles_global};
    a.wants = {k.eps != 0, k.no_samples != 0, k.update_ok != 0, k.iters};
    a.prior.isotropic = k.toggle != kPlanToggleCount - 1; a.prior.valid = 1; a.prior.dt = 0.05; a.prior.kg = -1.;
    a.prior.iso64 = a.prior.scan64 = a.prior.Qinv = table;
    a.prior.iso32 = a.prior.iso32p = a.prior.slabpre = (float*)table;
    const auto& t = kPlanToggles[k.toggle];
    if (t.flag) a.tg.*(t.flag) = (int)t.value;
    if (t.num) a.tg.*(t.num) = t.value;
    a.tg.store_free_min_bytes = k.min_bytes;
    auto add = [&](int kind, int flags = 0) -> CostTerm& {
        CostTerm& c = a.prog.terms[a.prog.n_terms++];
        c.kind = kind; c.flags = flags; c.K = 1.; c.dt = 0.05; c.dev_data = table;
        if (kind == SGPMP_COST_EE_GOAL) a.prog.n_ee += 1;
        if (kind == SGPMP_COST_SELF || kind == SGPMP_COST_SPHERES) a.prog.needs_fk = 1;
        return c;
    };
    const bool panda = (k.prog >= PROG_PANDA && k.prog <= PROG_PANDA_INTERP) || k.prog == PROG_CHAIN_GRID || k.prog == PROG_GOALS15;
    add(SGPMP_COST_GP, SGPMP_FLAG_GP_START).dt = k.prog == PROG_GP_DT ? 0.1 : 0.05;
    CostTerm& goal = add(SGPMP_COST_GOAL_PRIOR);
    goal.dim0 = k.prog == PROG_GOALS15 ? 15 : 1; goal.dim1 = 2 * k.n;
    goal.rows_per_goal = (long long)k.S * k.particles_global + (k.prog == PROG_GOAL_ROWS ? 1 : 0);
    if (k.prog == PROG_TWO_GP) add(SGPMP_COST_GP);
    if (k.prog == PROG_PLANAR_GRID || k.prog == PROG_CHAIN_GRID) { CostTerm& g = add(SGPMP_COST_GRID); g.dim0 = g.dim1 = 200; g.inv_cell = 10.; }
    if (panda) {
        add(SGPMP_COST_SELF);
        CostTerm& s = add(SGPMP_COST_SPHERES, k.prog == PROG_PANDA_SDF ? (SGPMP_FIELD_SDF | SGPMP_FLAG_SDF_CLAMP) : SGPMP_FIELD_RBF);
        if (k.prog == PROG_PANDA_INTERP) { s.n_interp = 2; s.interp_lo = 5; s.interp_hi = 7; }
    }
    if (k.prog == PROG_PANDA_EE || k.prog == PROG_PANDA_EE2 || k.prog == PROG_EE_ONLY) add(SGPMP_COST_EE_GOAL);
    if (k.prog == PROG_PANDA_EE2) add(SGPMP_COST_EE_GOAL);
    a.chain.n_joints = k.n; a.chain.n_links = k.n + 1;
    a.chain.plan.fast = k.chain != CHAIN_SLOW;
    a.chain.plan.codegen_id = k.chain == CHAIN_NONE ? 0 : (k.chain == CHAIN_PANDA || k.chain == CHAIN_SLOW) ? 1 : 2;
    a.rtc_available = k.chain == CHAIN_RTC;
    a.chain.rtc = (k.chain == CHAIN_RTC || k.chain == CHAIN_RTC_NOKERNEL) ? &a.rtc_available : nullptr;
}
// the stand-in for chain_rtc.hip's lookup: a handle that names the variant asked for, or null
static inline hipFunction_t plan_case_rtc_kernel(RtcChain* c, int ft, bool sweep, bool rag, bool small) {
    if (!c || !*(const int*)c) return nullptr;
    return (hipFunction_t)(uintptr_t)(0x1000 + ft * 8 + (sweep ? 4 : 0) + (rag ? 2 : 0) + (small ? 1 : 0));
}
