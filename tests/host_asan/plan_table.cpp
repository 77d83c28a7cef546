// The step's ONE decision (csrc/step_plan.hip: plan_step, the real object) held to a table of shapes and programs on the CPU,
// under AddressSanitizer + UBSan.  plan_table_rows.inc: a case (plan_cases.h), what update_kernel's scratch answers for its shape
// (update_regen_rows for recipes 1 and 2, update_ee_fold_fits -- update.hip is not part of this program), and the plan expected.
// The rows were recorded once from the predicates and the launcher plan_step replaced (fused_step_eligible, planar_seg_step,
// planar_tail_step, planar_persist_step, fused_step_regen_recipe, launch_fused_step's out-parameters), at the commit before:
// BASELINE configs 1-5, the reference's example sizes, the edges of every condition, every switch.
// Exit code 0 and PLAN_TABLE_OK = pass.  TEST INFRASTRUCTURE (tests/test_cpu_host.py).
#include <cstdio>
#include <cstring>

#include "plan_cases.h"

struct PlanRow {
    PlanCase k;
    int regen_rows1, regen_rows2, ee_fits;
    int family, ragged, small, mixed, field_type, L, partials, regen_recipe, update_in_launch, max_iters, iters, ee;
    const char* kernel;
};
static const PlanRow kRows[] = {
#include "plan_table_rows.inc"
};

static const PlanRow* g_row;
int update_regen_rows(int, int, int, int, int recipe) { return recipe == 1 ? g_row->regen_rows1 : recipe == 2 ? g_row->regen_rows2 : 0; }
bool update_ee_fold_fits(int, int, int, int) { return g_row->ee_fits != 0; }
hipFunction_t rtc_kernel(RtcChain* c, int ft, bool sweep, bool rag, bool small) { return plan_case_rtc_kernel(c, ft, sweep, rag, small); }

int main() {
    int bad = 0, n = 0;
    for (const PlanRow& r : kRows) {
        g_row = &r;
        PlanArgs a;
        plan_case_args(r.k, a);
        const StepPlan p = plan_step(a.shape, a.wants, a.prior, a.prog, a.chain, a.tg);
        const bool chain = p.family == STEP_CHAIN || p.family == STEP_CHAIN_RTC;
        const int got[] = {p.family, chain && p.ragged, p.small, p.mixed, chain ? p.field_type : 0, p.L, p.partials, p.regen_recipe, p.update_in_launch,
                           p.max_iters, p.iters, p.family != STEP_NONE ? p.ee : 0};
        const int want[] = {r.family, r.ragged, r.small, r.mixed, r.field_type, r.L, r.partials, r.regen_recipe, r.update_in_launch, r.max_iters, r.iters, r.ee};
        // a run-time chain's plan carries the kernel of exactly its variant
        const bool fn_ok = (p.family == STEP_CHAIN_RTC) == (p.rtc_fn != nullptr) &&
                           (!p.rtc_fn || p.rtc_fn == plan_case_rtc_kernel((RtcChain*)a.chain.rtc, p.field_type, false, p.ragged, p.small));
        n += 1;
        if (std::memcmp(got, want, sizeof(got)) != 0 || std::strcmp(p.kernel, r.kernel) != 0 || !fn_ok || std::memcmp(&p.shape, &a.shape, sizeof(StepShape)) != 0) {
            bad += 1;
            std::fprintf(stderr, "row %d (dtype %d n %d T %d S %d P %d+%d spheres %d total %d global %d prog %d chain %d switch '%s' min_bytes %lld wants %d%d%d x%d):\n  got ",
                         n, r.k.dtype, r.k.n, r.k.T, r.k.S, r.k.offset, r.k.P, r.k.n_spheres, r.k.particles_total, r.k.particles_global, r.k.prog, r.k.chain,
                         kPlanToggles[r.k.toggle].name, r.k.min_bytes, r.k.eps, r.k.no_samples, r.k.update_ok, r.k.iters);
            for (int v : got) std::fprintf(stderr, " %d", v);
            std::fprintf(stderr, " '%s'%s\n  want", p.kernel, fn_ok ? "" : " (run-time kernel handle wrong)");
            for (int v : want) std::fprintf(stderr, " %d", v);
            std::fprintf(stderr, " '%s'\n", r.kernel);
        }
    }
    std::printf("%d rows, %d wrong\n", n, bad);
    if (bad == 0 && n > 400) std::printf("PLAN_TABLE_OK\n");
    return bad != 0;
}
