// Stand-ins for the kernel launchers of libsgpmp.so (the launch_* functions defined beside the kernels in the .hip files) for
// the host-side sanitizer run: each TOUCHES exactly the byte ranges the real kernel reads and writes -- on malloc-backed
// "device" memory (stub_hip.cpp) -- so AddressSanitizer checks every pointer and size the host layer hands to a launch.
// TEST INFRASTRUCTURE (tests/test_cpu_host.py); no arithmetic of the product lives here.
#include <cstdlib>
#include <cstring>

#include "sgpmp_internal.h"

static size_t esz(int dtype) { return dtype == SGPMP_F64 ? 8 : 4; }
static void rd(const void* p, size_t n) {                 // read every byte (a checksum the optimiser cannot drop)
    if (!p || !n) return;
    volatile unsigned char acc = 0;
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; i += 61) acc = acc ^ b[i];
    acc = acc ^ b[n - 1];
}
static void wr(void* p, size_t n, int v = 0) { if (p && n) std::memset(p, v, n); }
static bool env1(const char* k) { const char* e = getenv(k); return e && *e == '1'; }

hipError_t launch_prior_factor(int n, int T, double, double, double, const double* qc, int, PriorDev out, hipStream_t) {
    const size_t d = 2 * n;
    rd(qc, sizeof(double) * n * n);
    wr(out.blocks, sizeof(double) * 4 * d * d); wr(out.G, sizeof(double) * T * d * d); wr(out.H, sizeof(double) * T * d * d);
    wr(out.iso64, sizeof(double) * T * 8); wr(out.iso32, sizeof(float) * T * 8); wr(out.Qinv, sizeof(double) * d * d);
    wr(out.G32, sizeof(float) * T * d * d); wr(out.H32, sizeof(float) * T * d * d);
    *out.status = env1("STUB_NOT_PD") ? 1 : 0;
    return hipSuccess;
}
hipError_t launch_prior_factor_blocks(int n, int T, int m, const double* D, const double* E, PriorDev out, hipStream_t) {
    const size_t d = 2 * n, dd = d * d;
    rd(D, sizeof(double) * m * T * dd); rd(E, sizeof(double) * m * (T - 1) * dd);
    wr(out.G, sizeof(double) * m * T * dd); wr(out.H, sizeof(double) * m * T * dd);
    wr(out.G32, sizeof(float) * m * T * dd); wr(out.H32, sizeof(float) * m * T * dd);
    *out.status = 0;
    return hipSuccess;
}
hipError_t launch_prior_quadform(int dtype, int n, int T, long long rows, int m, const void* x, const void* means, const PriorDev&, double* out, hipStream_t) {
    const size_t M = (size_t)T * 2 * n;
    rd(x, rows * M * esz(dtype)); rd(means, (size_t)m * M * esz(dtype)); wr(out, rows * sizeof(double));
    return hipSuccess;
}
hipError_t launch_sample(int dtype, int n, int T, const PriorDev& p, uint64_t, uint64_t, const void* means, int n_modes, int, int S,
                         const void* eps, int eps_modes, int, void* out, hipStream_t, const SgpmpToggles&, double* zero_stats) {
    const size_t M = (size_t)T * 2 * n;
    rd(p.iso32, sizeof(float) * T * 8); rd(means, (size_t)n_modes * M * esz(dtype));
    if (eps) rd(eps, (size_t)S * eps_modes * M * esz(dtype));
    wr(out, (size_t)n_modes * S * M * esz(dtype)); wr(zero_stats, sizeof(double) * SGPMP_STAT_SHARDS * 4);
    return hipSuccess;
}
hipError_t launch_noise(int dtype, int n, int T, int n_modes, int, int S, uint64_t, uint64_t, void* out, hipStream_t) {
    wr(out, (size_t)S * n_modes * T * 2 * n * esz(dtype));
    return hipSuccess;
}
hipError_t launch_cost(int dtype, int n, int T, const CostProgram&, const ChainDev* dch, const ChainDev&, const void* trajs, long long batch, long long,
                       const void* spheres, int ns, const void* isw, int rpp, double, void* costs, double* c64, hipStream_t, const SgpmpToggles&,
                       const char** picked) {
    const size_t M = (size_t)T * 2 * n;
    rd(dch, sizeof(ChainDev)); rd(trajs, batch * M * esz(dtype)); rd(spheres, (size_t)ns * 4 * esz(dtype));
    if (isw && rpp > 0) rd(isw, (size_t)(batch / rpp) * (T + 1) * 2 * n * esz(dtype));
    wr(costs, batch * esz(dtype)); wr(c64, batch * 8);
    *picked = "stub_cost";
    return hipSuccess;
}
bool update_ee_fold_fits(int, int, int, int S) { return S <= 4096; }
int update_regen_rows(int dtype, int, int T, int, int recipe) { return dtype == SGPMP_F32 && T % 2 == 0 && recipe == 1 ? 4 : 0; }
// The ONE decision (the real one: csrc/step_plan.hip, held to its table by plan_table.cpp): a chain-code-like fused step under
// STUB_FUSED=1; STUB_TAIL=1: as if a store-free step's launch updated its particles itself (fused_planar_seg.inc: seg_update);
// STUB_PERSIST=1 (with STUB_TAIL): as if that launch could run several iterations (PERSIST) -- sgpmp_optimize's chunking of a
// call is then exercised on the host
StepPlan plan_step(const StepShape& sh, const StepWants& w, const PriorDev&, const CostProgram& prog, const ChainDev&, const SgpmpToggles& tg) {
    StepPlan p = {};
    p.shape = sh; p.max_iters = p.iters = 1; p.kernel = "";
    if (!env1("STUB_FUSED") || w.eps || sh.dtype != SGPMP_F32 || tg.no_fused_step || sh.T % 16 != 0 || sh.S % 8 != 0 || sh.P < 1) return p;
    p.family = STEP_CHAIN; p.kernel = "stub_fused";
    p.partials = prog.needs_fk && !tg.no_dense_partials && (sh.T * 2 * sh.n) % 4 == 0;
    const bool nostore = w.no_samples && prog.n_ee == 0 && update_regen_rows(sh.dtype, sh.n, sh.T, sh.S, 1) > 0;
    p.update_in_launch = nostore && env1("STUB_TAIL") && w.update_in_launch_ok;
    p.regen_recipe = nostore && !p.update_in_launch ? 1 : 0;
    if (p.update_in_launch && env1("STUB_PERSIST") && !tg.no_persist_planar) p.max_iters = tg.persist_max_iters >= 2 ? (int)tg.persist_max_iters : 2048;
    if (prog.n_ee > 0) p.ee = !tg.no_ee_fold && prog.n_ee == 1 && update_ee_fold_fits(sh.dtype, sh.n, sh.T, sh.S) ? STEP_EE_FOLD : STEP_EE_LAUNCH;
    if (w.iters > 1 && w.iters <= p.max_iters) p.iters = w.iters;
    return p;
}
// every fused launch is logged for the driver: draw, iterations, particle range
static unsigned long long g_log_draw[4096];
static int g_log_iters[4096], g_log_first[4096], g_log_P[4096], g_log_n = 0;
extern "C" int stub_launch_log(int i, unsigned long long* draw, int* iters) {     // entry i of the log; returns the number of entries
    if (i >= 0 && i < g_log_n) { *draw = g_log_draw[i]; *iters = g_log_iters[i]; }
    return g_log_n;
}
extern "C" void stub_launch_log_range(int i, int* first, int* P) { *first = g_log_first[i]; *P = g_log_P[i]; }
extern "C" void stub_launch_log_clear() { g_log_n = 0; }
hipError_t launch_fused_step(const StepPlan& plan, const StepIo& io) {
    if (plan.family == STEP_NONE || !io.samples || !io.isw || (plan.iters > 1 && !plan.update_in_launch)) return hipErrorInvalidValue;
    const int n = plan.shape.n, T = plan.shape.T, S = plan.shape.S, P = plan.shape.P;
    const size_t M = (size_t)T * 2 * n;
    const FusedDenseHost& d = io.dense;
    rd(io.means, (size_t)P * M * 4); rd(io.isw, (size_t)P * (T + 1) * 2 * n * 4); rd(io.spheres, (size_t)plan.shape.n_spheres * 16);
    if (plan.regen_recipe) rd(io.prior->iso32p, sizeof(float) * T * 8);
    else if (!plan.update_in_launch) wr(io.samples, (size_t)P * S * M * 4);
    wr(io.costs, (size_t)P * S * 4); wr(io.costs64, (size_t)P * S * 8); wr(io.zero_stats, sizeof(double) * SGPMP_STAT_SHARDS * 4);
    rd(d.nnz, (size_t)P * 4);
    if (plan.partials) wr(d.part, (size_t)P * ((S + 7) / 8) * (M + 4) * 4);
    if (plan.update_in_launch) {                               // touches what update_kernel would
        rd(d.tail_done, 4); wr(d.tail_done, 4); rd(d.tail_acc, sizeof(double) * SGPMP_STAT_SHARDS * 4);
        wr(d.stats_out, sizeof(double) * SGPMP_STAT_SHARDS * 4);
        wr(const_cast<void*>(io.means), (size_t)P * M * 4); wr(d.weights, (size_t)P * S * 4); wr(d.grad, (size_t)P * M * 4);
        wr(d.means_prev, (size_t)P * M * 4); wr(const_cast<void*>(io.isw), (size_t)P * (T + 1) * 2 * n * 4); wr(d.nnz, (size_t)P * 4, 1);
    }
    if (g_log_n < 4096) { g_log_draw[g_log_n] = io.draw; g_log_iters[g_log_n] = plan.iters; g_log_first[g_log_n] = plan.shape.offset; g_log_P[g_log_n] = P; ++g_log_n; }
    return hipSuccess;
}
hipError_t launch_is_weights(int dtype, int n, int T, const PriorDev& p, const void* means, int P, double, void* out, double* zero_stats, hipStream_t) {
    rd(p.Qinv, sizeof(double) * 4 * n * n); rd(means, (size_t)P * T * 2 * n * esz(dtype));
    wr(out, (size_t)P * (T + 1) * 2 * n * esz(dtype)); wr(zero_stats, sizeof(double) * SGPMP_STAT_SHARDS * 4);
    return hipSuccess;
}
hipError_t launch_update(const UpdatePlan& plan, const UpdateIo& io) {
    if (!plan.ok) return hipErrorInvalidValue;
    const int n = plan.shape.n, T = plan.shape.T, P = plan.shape.P, S = plan.shape.S;
    if (P <= 0) return hipSuccess;
    const size_t M = (size_t)T * 2 * n, w = esz(plan.shape.dtype);
    rd(io.costs, (size_t)P * S * esz(plan.shape.costs_dtype));
    if (io.ee.term) {                                          // the end-effector goal term inside the update: chain, rows, the cost output
        rd(io.ee.d_chain, sizeof(ChainDev)); rd(io.samples, (size_t)P * S * M * w);
        if (io.ee.costs) { rd(io.ee.costs, (size_t)P * S * w); wr(io.ee.costs, (size_t)P * S * w); }
    }
    if (io.regen.recipe) {                                     // store-free step: tables instead of rows
        rd(io.regen.coef, sizeof(float) * T * 8);
        if (io.regen.recipe == 2) rd(io.regen.pre, sizeof(float) * T * 4);
    } else {
        rd(io.samples, (size_t)P * S * M * w);
    }
    wr(io.means, (size_t)P * M * w); wr(io.weights, (size_t)P * S * w); wr(io.grad, (size_t)P * M * w); wr(io.means_prev, (size_t)P * M * w);
    wr(io.means_copy, (size_t)P * M * w);
    if (io.stats) for (int i = 0; i < SGPMP_STAT_SHARDS * 4; ++i) io.stats[i] += 1.;  // accumulates, as the kernel's atomics do
    if (plan.tail) { rd(io.isw_prior->Qinv, sizeof(double) * 4 * n * n); wr(io.isw_next, (size_t)P * (T + 1) * 2 * n * w); }
    if (io.part) rd(io.part, (size_t)P * (S / 8) * (M + 4) * 4);
    if (io.nnz) { rd(io.nnz, (size_t)P * 4); wr(io.nnz, (size_t)P * 4, 1); }
    if (io.done) return hipEventRecord(io.done, nullptr);
    return hipSuccess;
}
hipError_t launch_stats_add(double* dst, const double* src, hipStream_t) {
    for (int i = 0; i < SGPMP_STAT_SHARDS * 4; ++i) dst[i] += src[i];
    return hipSuccess;
}
hipError_t launch_mode_stats(int dtype, int n, int T, int P, long long, int, int G, const void* means, double* out, hipStream_t) {
    const size_t M = (size_t)T * 2 * n;
    rd(means, (size_t)P * M * esz(dtype)); rd(out, (size_t)G * (M + 1) * 2 * 8); wr(out, (size_t)G * (M + 1) * 2 * 8);
    return hipSuccess;
}
hipError_t launch_ee_goal(int dtype, int n, int T, const CostTerm&, const ChainDev* ch, const void* trajs, long long batch, void* costs, double* c64, hipStream_t) {
    rd(ch, sizeof(ChainDev)); rd(trajs, (size_t)batch * T * 2 * n * esz(dtype)); wr(costs, batch * esz(dtype)); wr(c64, batch * 8);
    return hipSuccess;
}
hipError_t launch_ee_grad(int dtype, int n, const CostTerm&, const ChainDev*, const void*, long long, int, long long, long long, void*, void*, hipStream_t) { (void)dtype; (void)n; return hipSuccess; }
hipError_t launch_field_grad(int dtype, int n, const CostTerm&, const ChainDev*, int, const void* q, long long batch, int, const void* sph, int ns, void* value, void* grad, hipStream_t) {
    (void)q; rd(sph, (size_t)ns * 4 * esz(dtype)); wr(value, batch * esz(dtype)); wr(grad, batch * n * esz(dtype));
    return hipSuccess;
}
hipError_t launch_gpmp_diag(int, const GpmpArgs& a, double* diag, hipStream_t) { wr(diag, (size_t)a.T * 2 * a.n * 8); return hipSuccess; }
hipError_t launch_gpmp_solve(int dtype, const GpmpArgs& a, void* means, void* d_theta, void* costs, hipStream_t, bool) {
    const size_t M = (size_t)a.T * 2 * a.n;
    wr(a.scratch, (size_t)a.P * a.T * 2 * 256 * 8); wr(means, a.P * M * esz(dtype)); wr(d_theta, a.P * M * esz(dtype)); wr(costs, a.P * esz(dtype));
    *a.status = 0;
    return hipSuccess;
}
hipError_t launch_link_dist(int, const void*, long long, int, const void*, int, int, double, void*, hipStream_t) { return hipSuccess; }
hipError_t launch_fk(int dtype, int n, const ChainDev* ch, int n_links, const void* q, long long batch, void* frames, hipStream_t) {
    rd(ch, sizeof(ChainDev)); rd(q, batch * n * esz(dtype)); wr(frames, (size_t)batch * n_links * 16 * esz(dtype));
    return hipSuccess;
}
hipError_t launch_grid_lookup(int dtype, const CostTerm&, const void* xy, long long batch, void* out, hipStream_t) {
    rd(xy, batch * 2 * esz(dtype)); wr(out, batch * esz(dtype));
    return hipSuccess;
}
hipError_t launch_field_eval(int dtype, const CostTerm&, const void* frames, long long batch, int nl, const void*, int, void* out, hipStream_t) {
    rd(frames, (size_t)batch * nl * 16 * esz(dtype)); wr(out, batch * esz(dtype));
    return hipSuccess;
}
// run-time chain kernels: none in this harness (chain_rtc.hip needs hipModule*; its compile path has its own CPU test)
const char* rtc_chain_get(const char*, int, RtcChain**) { return "no run-time compiler in the sanitizer harness"; }
hipFunction_t rtc_kernel(RtcChain*, int, bool, bool, bool) { return nullptr; }
hipError_t rtc_launch(hipFunction_t, unsigned, unsigned, hipStream_t, void**, hipEvent_t) { return hipErrorNotSupported; }
const char* rtc_verify(RtcChain*, const ChainDev&, int, int* mismatch) { if (mismatch) *mismatch = 0; return "no run-time compiler in the sanitizer harness"; }
const char* rtc_error(const RtcChain*) { return ""; }
void rtc_stats(const RtcChain*, double* s, int* c, int* f) { if (s) *s = 0.; if (c) *c = 0; if (f) *f = 0; }
long long rtc_compile_check_c(const char*, int, char* err, size_t n) { if (err && n) err[0] = 0; return -1; }
