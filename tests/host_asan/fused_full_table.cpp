// Which instantiation of fused_step_kernel a step launches (csrc/step_plan.hip: fused_full_variant, the real object), walked on the
// CPU under AddressSanitizer + UBSan: the rule itself over every combination of launch mode and program, and plan_step's plans
// for the cases of plan_cases.h.  0: the generic kernel; 1 / 2: the four-term program compiled in, without / with the softmax
// partials armed.  Exit code 0 and FUSED_FULL_OK = pass.  TEST INFRASTRUCTURE (tests/test_cpu_fused_full.py).
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "plan_cases.h"

int update_regen_rows(int, int, int, int, int recipe) { return recipe == 1 ? 4 : 0; }
bool update_ee_fold_fits(int, int, int, int) { return true; }
hipFunction_t rtc_kernel(RtcChain* c, int ft, bool sweep, bool rag, bool small) { return plan_case_rtc_kernel(c, ft, sweep, rag, small); }

static int g_bad = 0, g_n = 0;
static void expect(int got, int want, const char* what, int i = 0) {
    g_n += 1;
    if (got != want) { g_bad += 1; std::fprintf(stderr, "%s [%d]: variant %d, expected %d\n", what, i, got, want); }
}

// a program from a list of (kind, flags)
struct TermSpec { int kind, flags, n_interp; };
static CostProgram program(std::initializer_list<TermSpec> terms) {
    static double table[64];
    CostProgram p;
    std::memset(&p, 0, sizeof(p));
    for (const TermSpec& t : terms) {
        CostTerm& c = p.terms[p.n_terms++];
        c.kind = t.kind; c.flags = t.flags; c.n_interp = t.n_interp; c.K = 1.; c.dt = 0.05; c.dev_data = table;
        if (t.kind == SGPMP_COST_EE_GOAL) p.n_ee += 1;
        if (t.kind == SGPMP_COST_SELF || t.kind == SGPMP_COST_SPHERES) p.needs_fk = 1;
    }
    return p;
}

int main() {
    const TermSpec GP = {SGPMP_COST_GP, SGPMP_FLAG_GP_START, 0}, GP_NOSTART = {SGPMP_COST_GP, 0, 0}, GOAL = {SGPMP_COST_GOAL_PRIOR, 0, 0},
                   SELF = {SGPMP_COST_SELF, 0, 0}, SPH = {SGPMP_COST_SPHERES, SGPMP_FIELD_RBF, 0},
                   SPH_SDF = {SGPMP_COST_SPHERES, SGPMP_FIELD_SDF | SGPMP_FLAG_SDF_CLAMP, 0}, SPH_INTERP = {SGPMP_COST_SPHERES, SGPMP_FIELD_RBF, 2},
                   EE = {SGPMP_COST_EE_GOAL, 0, 0}, GRID = {SGPMP_COST_GRID, 0, 0};
    // ---- the rule: every launch mode x every program
    const struct { CostProgram prog; bool four; } progs[] = {
        {program({GP, GOAL, SELF, SPH}), true}, {program({SPH_SDF, SELF, GOAL, GP}), true},          // (any order)
        {program({GP, GOAL, SELF, SPH, EE}), false}, {program({GP, GOAL, SELF, EE}), false}, {program({GP, GOAL, SELF}), false},
        {program({GP, GOAL, SPH}), false}, {program({GP, SELF, SPH}), false}, {program({GOAL, SELF, SPH}), false},
        {program({GP_NOSTART, GOAL, SELF, SPH}), false}, {program({GP, GOAL, SELF, SPH_INTERP}), false},
        {program({GP, GP, SELF, SPH}), false}, {program({GP, GOAL, SELF, SELF}), false}, {program({GP, GOAL, GRID, SPH}), false},
        {program({GP, GOAL, SELF, SPH, GRID}), false}, {program({}), false},
    };
    int pi = 0;
    for (const auto& pr : progs) {
        for (int m = 0; m < 6 * 2 * 2 * 2 * 3 * 2; ++m) {
            int k = m;
            StepPlan p;
            std::memset(&p, 0, sizeof(p));
            p.family = k % 6; k /= 6;
            p.ragged = k % 2; k /= 2;
            p.small = k % 2; k /= 2;
            p.partials = k % 2; k /= 2;
            p.regen_recipe = k % 3; k /= 3;
            SgpmpToggles tg;
            std::memset(&tg, 0, sizeof(tg));
            tg.fused_generic = k % 2;
            const bool full = pr.four && p.family == STEP_CHAIN && !p.ragged && !p.small && p.regen_recipe == 0 && !tg.fused_generic;
            expect(fused_full_variant(p, pr.prog, tg), full ? (p.partials ? 2 : 1) : 0, "rule", pi * 1000 + m);
        }
        pi += 1;
    }
    // ---- plan_step's plans
    const int F32 = SGPMP_F32, F64 = SGPMP_F64;
    int none = 0, nodense = 0, nosmall = 0;
    for (int i = 0; i < kPlanToggleCount; ++i) {
        if (!std::strcmp(kPlanToggles[i].name, "no_dense_partials")) nodense = i;
        if (!std::strcmp(kPlanToggles[i].name, "no_small_step")) nosmall = i;
    }
    //                   dtype n  T   S    P  off sph total global prog            chain        toggle min_bytes eps no_samples update_ok iters
    const struct { PlanCase k; int want; const char* what; } cases[] = {
        {{F32, 7, 64, 128, 512, 0, 5, 1024, 1024, PROG_PANDA, CHAIN_PANDA, none, 0, 0, 0, 1, 1}, 2, "headline half, storing"},
        {{F32, 7, 64, 128, 1024, 0, 5, 1024, 1024, PROG_PANDA, CHAIN_PANDA, nodense, 0, 0, 0, 1, 1}, 1, "no partials"},
        {{F32, 7, 64, 128, 1024, 0, 5, 1024, 1024, PROG_PANDA_SDF, CHAIN_PANDA, none, 0, 0, 0, 1, 1}, 2, "sdf"},
        {{F32, 7, 64, 128, 1024, 0, 5, 1024, 1024, PROG_PANDA, CHAIN_PANDA, none, 1, 0, 1, 1, 1}, 0, "store-free step"},
        {{F32, 7, 64, 128, 1024, 0, 5, 1024, 1024, PROG_PANDA, CHAIN_PANDA, none, 0, 0, 1, 1, 1}, 0, "store-free step above the break-even"},
        {{F32, 7, 32, 16, 4, 0, 5, 4, 4, PROG_PANDA, CHAIN_PANDA, none, 0, 0, 1, 1, 1}, 0, "small step, store-free refused"},
        {{F32, 7, 32, 16, 4, 0, 5, 4, 4, PROG_PANDA, CHAIN_PANDA, nosmall, 0, 0, 1, 1, 1}, 2, "few items as one wave each; too small to go store-free"},
        {{F32, 7, 32, 16, 4, 0, 5, 4, 4, PROG_PANDA, CHAIN_PANDA, none, 0, 0, 0, 1, 1}, 0, "small-step launch"},
        {{F32, 7, 64, 12, 1024, 0, 5, 1024, 1024, PROG_PANDA, CHAIN_PANDA, none, 0, 0, 0, 1, 1}, 0, "S off the grid"},
        {{F32, 7, 24, 128, 1024, 0, 5, 1024, 1024, PROG_PANDA, CHAIN_PANDA, none, 0, 0, 0, 1, 1}, 0, "T off the grid"},
        {{F32, 7, 64, 24, 1024, 0, 5, 1024, 1024, PROG_PANDA, CHAIN_PANDA, none, 0, 0, 0, 1, 1}, 2, "three groups per particle"},
        {{F32, 7, 64, 128, 1024, 0, 5, 1024, 1024, PROG_PANDA_EE, CHAIN_PANDA, none, 0, 0, 0, 1, 1}, 0, "end-effector term"},
        {{F32, 7, 64, 128, 1024, 0, 5, 1024, 1024, PROG_PANDA_EE2, CHAIN_PANDA, none, 0, 0, 0, 1, 1}, 0, "two end-effector terms"},
        {{F32, 7, 64, 128, 1024, 0, 5, 1024, 1024, PROG_PANDA_INTERP, CHAIN_PANDA, none, 0, 0, 0, 1, 1}, 0, "interpolated points"},
        {{F32, 7, 64, 128, 1024, 0, 5, 1024, 1024, PROG_CHAIN_GRID, CHAIN_PANDA, none, 0, 0, 0, 1, 1}, 0, "grid term"},
        {{F32, 7, 64, 128, 1024, 0, 5, 1024, 1024, PROG_GOALS15, CHAIN_PANDA, none, 0, 0, 0, 1, 1}, 0, "more goals than the launch stages"},
        {{F32, 7, 64, 128, 1024, 0, 5, 1024, 1024, PROG_PANDA, CHAIN_RTC, none, 0, 0, 0, 1, 1}, 0, "chain code compiled at run time"},
        {{F32, 7, 64, 128, 1024, 0, 5, 1024, 1024, PROG_PANDA, CHAIN_NONE, none, 0, 0, 0, 1, 1}, 0, "no chain code"},
        {{F32, 7, 64, 128, 1024, 0, 5, 1024, 1024, PROG_PANDA, CHAIN_PANDA, none, 0, 1, 0, 1, 1}, 0, "the caller's noise"},
        {{F64, 7, 64, 128, 1024, 0, 5, 1024, 1024, PROG_PANDA, CHAIN_PANDA, none, 0, 0, 0, 1, 1}, 0, "fp64"},
        {{F32, 2, 64, 64, 1024, 0, 0, 1024, 1024, PROG_PLANAR, CHAIN_NONE, none, 0, 0, 0, 1, 1}, 0, "planar"},
    };
    int ci = 0;
    for (const auto& c : cases) {
        PlanArgs a;
        plan_case_args(c.k, a);
        expect(plan_step(a.shape, a.wants, a.prior, a.prog, a.chain, a.tg).full, c.want, c.what, ci);
        a.tg.fused_generic = 1;
        expect(plan_step(a.shape, a.wants, a.prior, a.prog, a.chain, a.tg).full, 0, "fused_generic", ci);
        ci += 1;
    }
    // ... and the two programs plan_cases.h has no name for, on the headline's shape
    {
        PlanArgs a;
        plan_case_args(cases[0].k, a);
        a.prog.terms[0].flags = 0;                                        // the GP term without its start prior
        expect(plan_step(a.shape, a.wants, a.prior, a.prog, a.chain, a.tg).full, 0, "GP term without start prior");
        plan_case_args(cases[0].k, a);
        a.prog.n_terms = 3;                                               // no sphere term
        const StepPlan p = plan_step(a.shape, a.wants, a.prior, a.prog, a.chain, a.tg);
        expect(p.family, STEP_CHAIN, "three terms: still the chain-code launch");
        expect(p.full, 0, "missing sphere term");
    }
    std::printf("%d checks, %d wrong\n", g_n, g_bad);
    if (g_bad == 0 && g_n > 4000) std::printf("FUSED_FULL_OK\n");
    return g_bad != 0;
}
