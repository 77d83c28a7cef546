// K3 -- composite cost sweep over the trajectory batch: trajs [B,T,d] -> costs [B].
//
// Replaces CostComposite.eval (costs/cost_functions.py:47-58) and everything it calls:
//   CostGP / CostGPTrajectory.eval   cost_functions.py:128-146, 202-215  (+ gp_factor.py:54-67,
//                                    unary_factor.py:21-22)
//   CostGoalPrior.eval               cost_functions.py:376-388
//   CostCollision.eval               cost_functions.py:247-261 + field_factor.py:18-40 with
//       ObstacleMap.get_collisions   envs/obst_map.py:164-182
//       LinkDistanceField            costs/fields.py:63-86   (rbf / sdf / occupancy)
//       LinkSelfDistanceField        costs/fields.py:114-124
//   the FK callable                  cost_functions.py:51-52 (URDF chain)
//   the importance-sampling term     planner.py:233-236, in the factored form
//       x^T Sigma^-1 mu = (A x)^T [blkdiag(K_s, Q^-1.., K_g) A mu],  A x = (x_0, e_0.., x_{T-1})
//
// Mapping: ONE WAVE PER TRAJECTORY, ONE LANE PER WAYPOINT (64 waypoints per pass).  A lane loads its
// own d-vector (the wave reads one contiguous 64*d*w-byte span), gets x_{t-1} from its neighbour
// lane, evaluates every per-waypoint term, and the wave reduces the 64 partial costs in fp64.
//
// Per-term constants travel in the kernel-argument segment (ProgK, by value) and per-joint constants
// are read through the constant address space, so both are scalar loads into SGPRs; read through a
// plain global pointer they become loop-invariant VECTOR loads that pin >200 VGPRs.
//
// Link fields have two paths:
//   register path (FKMODE = number of joints): revolute-first chains without interpolated points.
//     The link positions stay in registers (every loop over links is unrolled), coincident links
//     are merged and rigid link pairs folded into a constant by the host analysis (FkPlan), exp is
//     one v_exp_f32 (exp2 with log2(e) folded into the constant) and sin/cos are native in fp32.
//   generic path (FKMODE = -1): any chain / interpolated points; link positions of the lane's
//     waypoint live in LDS (structure-of-arrays, one column per lane: bank-conflict free) because
//     the loops index them dynamically.
#include <cstdlib>
#include <cstring>

#include "chain_code_generated.h"
#include "rng.h"
#include "sgpmp_internal.h"
#include "update_common.h"
#include <hip/hip_ext.h>

#include "cost_device.h"
#include "cost_host.h"

// ---- host side of the kernel-argument structs (make_termk, make_flat: cost_host.h)
template <typename real>
static ProgK<real> make_progk(const CostProgram& p) {
    ProgK<real> k;
    k.n_terms = p.n_terms; k.needs_fk = p.needs_fk;
    for (int i = 0; i < SGPMP_MAX_TERMS; ++i) k.t[i] = make_termk<real>(p.terms[i]);
    return k;
}

#include "cost_sweep_kernel.inc"
#include "cost_sweep_dual.inc"
#include "fused_step.inc"
#include "fused_planar.inc"
#include "fused_planar_seg.inc"

// K2 + K3 in one launch, as the plan says (step_plan.hip: plan_step has the conditions)
hipError_t launch_fused_step(const StepPlan& plan, const StepIo& io) {
    using CCp = ChainCode_panda;
    const StepShape& sh = plan.shape;
    const int n = sh.n, T = sh.T, S = sh.S, P = sh.P, n_spheres = sh.n_spheres;
    const PriorDev& prior = *io.prior;
    const CostProgram& h_prog = *io.prog;
    const FusedDenseHost& dense = io.dense;
    hipStream_t stream = io.stream;
    if (plan.family == STEP_NONE || !io.samples || !io.isw) return hipErrorInvalidValue;
    if (plan.iters > 1 && !plan.update_in_launch) return hipErrorInvalidValue;    // (several iterations: only where the launch updates)
    auto log2_exact = [](long long v) { int s = 0; while ((1LL << s) < v && s < 62) ++s; return (1LL << s) == v ? s : -1; };
    const long long batch = (long long)P * S, batch_offset = (long long)sh.offset * S;
    if (plan.family == STEP_F64) {
        FlatProg<double> F;
        make_flat<double>(h_prog, F);
        const ProgK<double> PK = make_progk<double>(h_prog);
        CostArgs<double> a;
        a.T = T; a.chain = nullptr; a.n_links = io.chain->n_links; a.trajs = (const double*)io.samples;
        a.batch = batch; a.batch_offset = batch_offset;
        a.spheres = (const double*)io.spheres; a.n_spheres = n_spheres;
        a.isw = (const double*)io.isw; a.rows_per_particle = S; a.is_dt = prior.dt;
        a.costs = (double*)io.costs; a.costs64 = io.costs64;
        a.rpp_shift = log2_exact(S); a.rpg_shift = F.has_goal ? log2_exact(F.goal.rows_per_goal) : -1;
        GenArgs64 g;
        g.coef = prior.iso64; g.scan = prior.scan64; g.means = (const double*)io.means; g.samples = (double*)io.samples;
        g.seed = io.seed; g.draw = io.draw; g.mode_offset = sh.offset; g.S = S; g.zero_stats = io.zero_stats;
        const size_t lds = (size_t)T * SGPMP_SCAN64_ROW * sizeof(double);
        // (few trajectories -- BASELINE configs[0] has 64 -- : one wave per workgroup, so that every wave gets a CU of its own, and
        // the lanes read their rows of the scan table straight from memory: staging 14 KB per workgroup for one or two items is a
        // string of dependent round trips a latency-bound launch cannot hide)
        const int block = a.batch <= 2048 ? 64 : 256;
        const bool scan_lds = lds <= 48 * 1024 && a.batch > 2048;
        long long blocks = (a.batch + block / 64 - 1) / (block / 64);
        const long long cap = 256LL * 32;
        if (blocks > cap) blocks = cap;
        // (+ the chain launches' store tile: a pass of 64 waypoints x d doubles per wave -- cost_sweep_kernel.inc)
        const bool store_tile = scan_lds && h_prog.needs_fk;
        const unsigned dyn = scan_lds ? (unsigned)(lds + (store_tile ? (size_t)(block / 64) * 64 * 2 * n * sizeof(double) : 0)) : 0u;
        // (SCAN_: how a big launch reads its staged scan table -- cost_sweep_kernel.inc: in one batch, or round by round)
#define F64_LAUNCH(K_, N_, FK_, SCAN_) do { if (scan_lds) hipLaunchKernelGGL((K_<N_, FK_, SCAN_>), dim3((unsigned)blocks), dim3(block), dyn, stream, a, PK, F, g); \
                                            else hipLaunchKernelGGL((K_<N_, FK_, 0>), dim3((unsigned)blocks), dim3(block), dyn, stream, a, PK, F, g); } while (0)
        if (h_prog.needs_fk && plan.mixed) F64_LAUNCH(fused_step_f64_mixed_kernel, CCp::N, 1000, 2);
        else if (h_prog.needs_fk) F64_LAUNCH(fused_step_f64_kernel, CCp::N, 1000, 1);
        else if (n == 2) F64_LAUNCH(fused_step_f64_kernel, 2, 0, 2);
        else F64_LAUNCH(fused_step_f64_kernel, 3, 0, 2);
#undef F64_LAUNCH
        return hipGetLastError();
    }
    FlatProg<float> F;
    make_flat<float>(h_prog, F);
    CostArgs<float> a;
    a.T = T; a.chain = nullptr; a.n_links = io.chain->n_links; a.trajs = (const float*)io.samples;
    a.batch = batch; a.batch_offset = batch_offset; a.spheres = (const float*)io.spheres; a.n_spheres = n_spheres;
    a.isw = (const float*)io.isw; a.rows_per_particle = S; a.is_dt = (float)prior.dt;
    a.costs = (float*)io.costs; a.costs64 = io.costs64;
    a.rpp_shift = log2_exact(S);
    a.rpg_shift = F.has_goal ? log2_exact(F.goal.rows_per_goal) : -1;
    const bool chain_code = plan.family == STEP_CHAIN || plan.family == STEP_CHAIN_RTC;
    FusedArgs fs;
    fs.coef = prior.iso32; fs.coefp = prior.iso32p; fs.means = (const float*)io.means; fs.samples = (float*)io.samples;
    fs.seed = io.seed; fs.draw = io.draw; fs.mode_offset = sh.offset; fs.S = S;
    fs.gpp = (S + SGPMP_FUSED_SPW - 1) / SGPMP_FUSED_SPW; fs.gpp_shift = log2_exact(fs.gpp);
    fs.nitems = (long long)P * fs.gpp;
    fs.zero_stats = io.zero_stats;
    fs.part = nullptr; fs.nnz_prev = dense.nnz; fs.nnz_threshold = 0u; fs.inv_temperature = 0.f;
    fs.nostore = 0; fs.store_threshold = 0u;
    std::memset(&fs.tail, 0, sizeof(fs.tail));
    if (plan.partials) {                          // softmax partials for the dense-weight regime of the update
        if (!dense.part || !dense.nnz) return hipErrorInvalidValue;
        fs.part = dense.part; fs.nnz_threshold = dense.threshold;
        fs.inv_temperature = (float)(1. / dense.temperature);
    }
    if (plan.regen_recipe != 0) {                 // store-free step: the update behind the launch regenerates rows
        if (!dense.nnz) return hipErrorInvalidValue;
        fs.nostore = 1; fs.store_threshold = dense.store_threshold;
    }
    const long long nitems = chain_code ? fs.nitems : batch / SGPMP_FUSED_SPW;
    long long blocks = (nitems + 3) / 4;
    if (blocks > plan.block_cap) blocks = plan.block_cap;
    if (plan.family == STEP_PLANAR_SEG) {
        const int L = plan.L, G = T / L;
        const long long wgs = batch / 64;
        const bool upd = plan.update_in_launch;
        fs.gpp = S / 64; fs.gpp_shift = log2_exact(fs.gpp);
        if (upd) {
            if (!dense.tail_done) return hipErrorInvalidValue;
            SegTail& t = fs.tail;
            t.done = dense.tail_done; t.acc = dense.tail_acc; t.stats_out = dense.stats_out;
            t.means = (float*)const_cast<void*>(io.means); t.weights = (float*)dense.weights; t.grad = (float*)dense.grad;
            t.means_prev = (float*)dense.means_prev; t.isw_next = (float*)const_cast<void*>(io.isw); t.nnz_out = dense.nnz;
            t.Qinv = prior.Qinv; t.ks = prior.ks; t.kg = prior.kg; t.dt = prior.dt;
            t.temperature = dense.temperature; t.step_size = dense.step_size; t.P = P;
            t.iters = plan.iters;
            if (t.iters > 1) { t.done = nullptr; t.stats_out = nullptr; }    // (several iterations in this launch: no statistics)
            fs.nostore = 1; fs.store_threshold = 0xffffffffu;
            fs.zero_stats = nullptr;                      // (the launch's last particle writes the statistics)
        }
        const float* tab = prior.slabpre + (size_t)plan.seg_table * T * 4;
        const unsigned lds = plan.seg_lds;
#define SEG_LAUNCH(NN, LL) do { if (upd) hipLaunchKernelGGL((fused_planar_seg_kernel<NN, LL, true>), dim3((unsigned)wgs), dim3(64 * G), lds, stream, a, F, fs, tab); \
                                 else hipLaunchKernelGGL((fused_planar_seg_kernel<NN, LL, false>), dim3((unsigned)wgs), dim3(64 * G), lds, stream, a, F, fs, tab); } while (0)
        if (plan.iters > 1) {
            if (n != 2 || L != 8) return hipErrorInvalidValue;     // (PERSIST is instantiated for this shape alone)
            hipLaunchKernelGGL((fused_planar_seg_kernel<2, 8, true, true>), dim3((unsigned)wgs), dim3(64 * G), lds, stream, a, F, fs, tab);
        }
        else if (n == 2) { if (L == 8) SEG_LAUNCH(2, 8); else SEG_LAUNCH(2, 16); }
        else SEG_LAUNCH(3, 8);
#undef SEG_LAUNCH
        return hipGetLastError();
    }
    if (plan.family == STEP_PLANAR_TILE) {
        if (n == 2) hipLaunchKernelGGL((fused_planar_kernel<2>), dim3((unsigned)blocks), dim3(256), 0, stream, a, F, fs);
        else hipLaunchKernelGGL((fused_planar_kernel<3>), dim3((unsigned)blocks), dim3(256), 0, stream, a, F, fs);
        return hipGetLastError();
    }
    const int ft = plan.field_type;
    const bool rag = plan.ragged, small = plan.small;
    // the launch sizes the sphere / state tables (dynamic LDS): 30.7 KB of tiles + these per workgroup, five workgroups per CU while
    // they stay under 2 KB
    const size_t dyn = fused_wave_dyn_lds(n_spheres, F.has_goal ? F.goal.dim0 : 0);
    if (plan.family == STEP_CHAIN_RTC) {           // this chain's kernels were compiled at run time (chain_rtc.hip)
        if (!plan.rtc_fn) return hipErrorInvalidValue;
        void* args[] = {&a, &F, &fs};
        return rtc_launch(plan.rtc_fn, small ? (unsigned)fs.nitems : (unsigned)blocks, (unsigned)dyn, stream, args, nullptr);
    }
#ifndef SGPMP_FUSED_EXTRA_LDS   // occupancy diagnostic: unused bytes per workgroup, e.g. 8000 -> four workgroups per CU instead of five
#define SGPMP_FUSED_EXTRA_LDS 0
#endif
    if (small) {
#define SMALL_LAUNCH(FT_, RAG_) hipLaunchKernelGGL((fused_step_small_kernel<CCp::N, CCp, FT_, RAG_>), dim3((unsigned)fs.nitems), dim3(256), (unsigned)dyn, stream, a, F, fs)
        if (ft == SGPMP_FIELD_RBF) { if (rag) SMALL_LAUNCH(SGPMP_FIELD_RBF, true); else SMALL_LAUNCH(SGPMP_FIELD_RBF, false); }
        else if (ft == SGPMP_FIELD_SDF) { if (rag) SMALL_LAUNCH(SGPMP_FIELD_SDF, true); else SMALL_LAUNCH(SGPMP_FIELD_SDF, false); }
        else { if (rag) SMALL_LAUNCH(SGPMP_FIELD_OCCUPANCY, true); else SMALL_LAUNCH(SGPMP_FIELD_OCCUPANCY, false); }
#undef SMALL_LAUNCH
        return hipGetLastError();
    }
    // S, T off the launch's grid of 8 rows x 16 waypoints: the instantiation with the masks (fused_step.inc: RAG)
#define FUSED_LAUNCH(...) hipExtLaunchKernelGGL((fused_step_kernel<CCp::N, CCp, __VA_ARGS__>), dim3((unsigned)blocks), dim3(256), (unsigned)dyn + SGPMP_FUSED_EXTRA_LDS, stream, (hipEvent_t) nullptr, (hipEvent_t) nullptr, 0u, a, F, fs)
    // the four-term program compiled in (fused_step.inc: FULL; step_plan.hip: fused_full_variant -- what the plan says must hold HERE,
    // or the launch would ignore a term or an argument it was given)
    const int full = plan.full;
    if (full != 0 && (rag || fs.nostore || (full == 1) != (fs.part == nullptr) || !F.has_gp || !(F.gp.flags & SGPMP_FLAG_GP_START) ||
                      !F.has_goal || !F.has_self || !F.has_sph || F.has_grid))
        return hipErrorInvalidValue;
#define FUSED_FIELD(FT_) do { if (full == 1) FUSED_LAUNCH(FT_, false, 1); else if (full == 2) FUSED_LAUNCH(FT_, false, 2); \
                              else if (rag) FUSED_LAUNCH(FT_, true); else FUSED_LAUNCH(FT_, false); } while (0)
    if (ft == SGPMP_FIELD_RBF) FUSED_FIELD(SGPMP_FIELD_RBF);
    else if (ft == SGPMP_FIELD_SDF) FUSED_FIELD(SGPMP_FIELD_SDF);
    else FUSED_FIELD(SGPMP_FIELD_OCCUPANCY);
#undef FUSED_FIELD
#undef FUSED_LAUNCH
    return hipGetLastError();
}

template <typename real>
static hipError_t cost_dispatch(int n, int T, const CostProgram& h_prog, const ChainDev* d_chain,
                                const ChainDev& h_chain, const real* trajs, long long batch,
                                long long batch_offset, const real* spheres, int n_spheres,
                                const real* isw, int rows_per_particle, double is_dt, real* costs,
                                double* costs64, hipStream_t stream, const SgpmpToggles& tg, const char** picked) {
    const int n_links = h_chain.n_links;
    const char* unused_name;
    if (!picked) picked = &unused_name;
    constexpr bool f64 = sizeof(real) == 8;
    if (batch + batch_offset >= (1LL << 31)) return hipErrorInvalidValue;   // row indices are 32-bit
    CostArgs<real> a;
    a.T = T; a.chain = d_chain; a.n_links = n_links; a.trajs = trajs;
    a.batch = batch; a.batch_offset = batch_offset; a.spheres = spheres; a.n_spheres = n_spheres;
    a.isw = isw; a.rows_per_particle = rows_per_particle > 0 ? rows_per_particle : 1;
    a.is_dt = (real)is_dt; a.costs = costs; a.costs64 = costs64;
    const ProgK<real> P = make_progk<real>(h_prog);
    int block = 256;
    size_t lds = 0;
    const bool fk = h_prog.needs_fk != 0;
    // register path: revolute-first chain, no interpolated points, an instantiated (n, joints) pair
    bool reg = fk && h_chain.plan.fast && !tg.force_generic_fk;
    for (int i = 0; i < h_prog.n_terms; ++i)
        if (h_prog.terms[i].n_interp > 0) reg = false;
    const int nj = n_links - 1;
    if (fk && !reg) {
        int max_pts = n_links;
        for (int i = 0; i < h_prog.n_terms; ++i)
            if (h_prog.terms[i].n_points > max_pts) max_pts = h_prog.terms[i].n_points;
        lds = (size_t)max_pts * 3 * block * sizeof(real);
        while (lds > 64 * 1024 && block > 64) { block >>= 1; lds >>= 1; }
    }
    const int wpb = block / 64;
    long long blocks = (batch + wpb - 1) / wpb;
    const long long cap = 256LL * 32;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    FlatProg<real> F;
    const bool flat = make_flat<real>(h_prog, F) && !tg.no_flat_program;
    auto log2_exact = [](long long v) { int s = 0; while ((1LL << s) < v && s < 62) ++s; return (1LL << s) == v ? s : -1; };
    a.rpp_shift = log2_exact(a.rows_per_particle);
    a.rpg_shift = (flat && F.has_goal) ? log2_exact(F.goal.rows_per_goal) : -1;
    const bool cg_static = h_chain.plan.codegen_id == 1 && n == ChainCode_panda::N;
    const bool cg_rtc = h_chain.plan.codegen_id == 2 && h_chain.rtc && sizeof(real) == 4 && n <= 7;
    if (reg && (cg_static || cg_rtc) && !tg.no_chain_codegen) {
        if constexpr (sizeof(real) == 4) {
            // two trajectories per wave on packed fp32 math (cost_sweep_dual.inc) when rows pair up
            const bool pairs_ok = (batch_offset % 2 == 0) && (!isw || a.rows_per_particle % 2 == 0) &&
                                  (!F.has_goal || F.goal.rows_per_goal % 2 == 0);
            const int ft = F.has_sph ? (F.sph.flags & 15) : SGPMP_FIELD_RBF;
            const bool sph_ok = !F.has_sph || n_spheres <= SGPMP_SPH_LDS;
            // chunked sweep (fused_step.inc, phase C alone on existing samples): 8 rows of one particle and goal
            // per wave, 16 waypoints per chunk -- fewer instructions per waypoint than the 64-lane passes below
            const bool chunk_ok = flat && !F.has_grid && sph_ok && !tg.no_dual_sweep && !tg.no_chunked_sweep &&
                                  batch % SGPMP_FUSED_SPW == 0 && batch_offset % SGPMP_FUSED_SPW == 0 &&
                                  T % SGPMP_FUSED_TC == 0 && n_spheres <= SGPMP_FUSED_SPH &&
                                  (!isw || a.rows_per_particle % SGPMP_FUSED_SPW == 0) &&
                                  (!F.has_goal || (F.goal.rows_per_goal % SGPMP_FUSED_SPW == 0 && F.goal.dim0 <= SGPMP_FUSED_GOALS)) &&
                                  (!F.has_gp || a.is_dt == F.gp.dt || !isw);
            if (chunk_ok) {
                FusedArgs fs;
                std::memset(&fs, 0, sizeof(fs));
                fs.gpp = 1; fs.gpp_shift = 0;
                long long cblocks = (batch / SGPMP_FUSED_SPW + 3) / 4;
                long long ccap = 1LL << 18;
                if (tg.k3_blocks > 0) ccap = tg.k3_blocks;
                if (cblocks > ccap) cblocks = ccap;
                const int cft = F.has_sph ? (F.sph.flags & 15) : SGPMP_FIELD_RBF;
                hipFunction_t rf = cg_rtc ? rtc_kernel((RtcChain*)h_chain.rtc, cft, true) : nullptr;
                if (cg_rtc && rf) {                       // the chain's own kernels, compiled at run time (chain_rtc.hip)
                    void* args[] = {&a, &F, &fs};
                    const hipError_t e = rtc_launch(rf, (unsigned)cblocks, 0u, stream, args, nullptr);
                    *picked = "cost_sweep_chunked_kernel (run-time chain code)";
                    return e;
                }
                if (!cg_rtc) {                            // (cg_rtc without a kernel: FkPlan register path below)
                if (cft == SGPMP_FIELD_RBF)
                    hipLaunchKernelGGL((cost_sweep_chunked_kernel<ChainCode_panda::N, ChainCode_panda, SGPMP_FIELD_RBF>),
                                       dim3((unsigned)cblocks), dim3(256), 0, stream, a, F, fs);
                else if (cft == SGPMP_FIELD_SDF)
                    hipLaunchKernelGGL((cost_sweep_chunked_kernel<ChainCode_panda::N, ChainCode_panda, SGPMP_FIELD_SDF>),
                                       dim3((unsigned)cblocks), dim3(256), 0, stream, a, F, fs);
                else
                    hipLaunchKernelGGL((cost_sweep_chunked_kernel<ChainCode_panda::N, ChainCode_panda, SGPMP_FIELD_OCCUPANCY>),
                                       dim3((unsigned)cblocks), dim3(256), 0, stream, a, F, fs);
                *picked = "cost_sweep_chunked_kernel";
                return hipGetLastError();
                }
            }
            if (cg_static && flat && !F.has_grid && pairs_ok && sph_ok && !tg.no_dual_sweep) {
                long long pblocks = ((batch + 1) / 2 + 3) / 4;
                long long pcap = 256LL * 20;          // 20 workgroups per CU (4 resident): measured optimum (tools/k3_grid_sweep.sh)
                if (tg.k3_blocks > 0) pcap = tg.k3_blocks;
                if (pblocks > pcap) pblocks = pcap;
                if (pblocks < 1) pblocks = 1;
                const bool pf = T <= 64 && T % 2 == 0 && !tg.k3_no_one && !tg.k3_no_lds_prefetch;
                const bool one = T <= 64 && !tg.k3_no_one;
                const bool pf_multi = T > 64 && T % 2 == 0 && !tg.k3_no_lds_prefetch;
                *picked = pf ? "cost_sweep_dual_pf_kernel" : pf_multi ? "cost_sweep_dual_pf_multi_kernel"
                                                                      : "cost_sweep_dual_kernel";
#define DUAL_LAUNCH(FT)                                                                                    \
                if (pf)                                                                                    \
                    hipLaunchKernelGGL((cost_sweep_dual_pf_kernel<ChainCode_panda::N, ChainCode_panda, FT>),          \
                                       dim3((unsigned)pblocks), dim3(256), 0, stream, a, F);               \
                else if (pf_multi)                                                                         \
                    hipLaunchKernelGGL((cost_sweep_dual_pf_multi_kernel<ChainCode_panda::N, ChainCode_panda, FT>),    \
                                       dim3((unsigned)pblocks), dim3(256), 0, stream, a, F);               \
                else if (one && FT == SGPMP_FIELD_RBF)                                                     \
                    hipLaunchKernelGGL((cost_sweep_dual_kernel<ChainCode_panda::N, ChainCode_panda, true, SGPMP_FIELD_RBF>), \
                                       dim3((unsigned)pblocks), dim3(256), 0, stream, a, F);               \
                else                                                                                       \
                    hipLaunchKernelGGL((cost_sweep_dual_kernel<ChainCode_panda::N, ChainCode_panda, false, FT>),      \
                                       dim3((unsigned)pblocks), dim3(256), 0, stream, a, F)
                if (ft == SGPMP_FIELD_RBF) { DUAL_LAUNCH(SGPMP_FIELD_RBF); }
                else if (ft == SGPMP_FIELD_SDF) { DUAL_LAUNCH(SGPMP_FIELD_SDF); }
                else { DUAL_LAUNCH(SGPMP_FIELD_OCCUPANCY); }
#undef DUAL_LAUNCH
                return hipGetLastError();
            }
        }
        if (cg_static) {
        *picked = f64 ? "cost_sweep_kernel<f64, generated chain>" : "cost_sweep_kernel<f32, generated chain>";
        if (flat)
            hipLaunchKernelGGL((cost_sweep_kernel<real, ChainCode_panda::N, 1000, true>), dim3((unsigned)blocks),
                               dim3(256), 0, stream, a, P, F);
        else
            hipLaunchKernelGGL((cost_sweep_kernel<real, ChainCode_panda::N, 1000, false>), dim3((unsigned)blocks),
                               dim3(256), 0, stream, a, P, F);
        return hipGetLastError();
        }
    }
#define COST_REG(NN, NJJ)                                                                          \
    if (reg && n == NN && nj == NJJ) {                                                             \
        *picked = f64 ? "cost_sweep_kernel<f64, register FK>" : "cost_sweep_kernel<f32, register FK>"; \
        hipLaunchKernelGGL((cost_sweep_kernel<real, NN, NJJ, false>), dim3((unsigned)blocks), dim3(256), 0, \
                           stream, a, P, F);                                                       \
        return hipGetLastError();                                                                  \
    }
    COST_REG(7, 10) COST_REG(7, 7) COST_REG(6, 6) COST_REG(3, 3) COST_REG(2, 2)
#undef COST_REG
    if (reg) {               // no instantiation for this (n, joints): fall back to the generic path
        int max_pts = n_links;
        lds = (size_t)max_pts * 3 * block * sizeof(real);
        while (lds > 64 * 1024 && block > 64) { block >>= 1; lds >>= 1; }
        blocks = (batch + block / 64 - 1) / (block / 64);
        if (blocks > cap) blocks = cap;
    }
    *picked = fk ? (f64 ? "cost_sweep_kernel<f64, generic FK>" : "cost_sweep_kernel<f32, generic FK>")
                 : (f64 ? "cost_sweep_kernel<f64, no FK>" : "cost_sweep_kernel<f32, no FK>");
#define COST_CASE(NN)                                                                              \
    case NN:                                                                                       \
        if (fk)                                                                                    \
            hipLaunchKernelGGL((cost_sweep_kernel<real, NN, -1, false>), dim3((unsigned)blocks),   \
                               dim3(block), lds, stream, a, P, F);                                 \
        else if (flat)                                                                             \
            hipLaunchKernelGGL((cost_sweep_kernel<real, NN, 0, true>), dim3((unsigned)blocks),     \
                               dim3(block), 0, stream, a, P, F);                                   \
        else                                                                                       \
            hipLaunchKernelGGL((cost_sweep_kernel<real, NN, 0, false>), dim3((unsigned)blocks),    \
                               dim3(block), 0, stream, a, P, F);                                   \
        break;
    switch (n) {
        COST_CASE(1) COST_CASE(2) COST_CASE(3) COST_CASE(4) COST_CASE(5) COST_CASE(6) COST_CASE(7) COST_CASE(8)
        default: return hipErrorInvalidValue;
    }
#undef COST_CASE
    return hipGetLastError();
}

// What sgpmp_last_cost_kernel reports for a sweep with body_cost_kernel behind it.  A program that holds the body term is never
// FLAT, so the sweep is one of cost_dispatch's four non-FLAT forms, in either dtype.
static const char* body_sweep_name(const char* sweep) {
    static const char* const names[][2] = {
        {"cost_sweep_kernel<f32, generated chain>", "cost_sweep_kernel<f32, generated chain> + body_cost_kernel"},
        {"cost_sweep_kernel<f64, generated chain>", "cost_sweep_kernel<f64, generated chain> + body_cost_kernel"},
        {"cost_sweep_kernel<f32, register FK>", "cost_sweep_kernel<f32, register FK> + body_cost_kernel"},
        {"cost_sweep_kernel<f64, register FK>", "cost_sweep_kernel<f64, register FK> + body_cost_kernel"},
        {"cost_sweep_kernel<f32, generic FK>", "cost_sweep_kernel<f32, generic FK> + body_cost_kernel"},
        {"cost_sweep_kernel<f64, generic FK>", "cost_sweep_kernel<f64, generic FK> + body_cost_kernel"},
        {"cost_sweep_kernel<f32, no FK>", "cost_sweep_kernel<f32, no FK> + body_cost_kernel"},
        {"cost_sweep_kernel<f64, no FK>", "cost_sweep_kernel<f64, no FK> + body_cost_kernel"},
    };
    for (const auto& n : names)
        if (std::strcmp(sweep, n[0]) == 0 || std::strcmp(sweep, n[1]) == 0) return n[1];
    return "cost sweep + body_cost_kernel";
}

// The same for body_self_cost_kernel, behind a bare sweep or behind body_cost_kernel (program order: the body term first).
static const char* body_self_sweep_name(const char* sweep) {
#define BSELF_NAMES(s) {s, s " + body_self_cost_kernel"}, {s " + body_cost_kernel", s " + body_cost_kernel + body_self_cost_kernel"}
    static const char* const names[][2] = {
        BSELF_NAMES("cost_sweep_kernel<f32, generated chain>"), BSELF_NAMES("cost_sweep_kernel<f64, generated chain>"),
        BSELF_NAMES("cost_sweep_kernel<f32, register FK>"), BSELF_NAMES("cost_sweep_kernel<f64, register FK>"),
        BSELF_NAMES("cost_sweep_kernel<f32, generic FK>"), BSELF_NAMES("cost_sweep_kernel<f64, generic FK>"),
        BSELF_NAMES("cost_sweep_kernel<f32, no FK>"), BSELF_NAMES("cost_sweep_kernel<f64, no FK>"),
    };
#undef BSELF_NAMES
    for (const auto& n : names)
        if (std::strcmp(sweep, n[0]) == 0 || std::strcmp(sweep, n[1]) == 0) return n[1];
    return "cost sweep + body_self_cost_kernel";
}

hipError_t launch_cost(int dtype, int n, int T, const CostProgram& h_prog, const ChainDev* d_chain,
                       const ChainDev& h_chain, const void* trajs, long long batch,
                       long long batch_offset, const void* spheres, int n_spheres,
                       const void* is_weights, int rows_per_particle, double is_dt, void* costs,
                       double* costs64, hipStream_t stream, const SgpmpToggles& tg, const char** picked) {
    hipError_t e;
    if (dtype == SGPMP_F64)
        e = cost_dispatch<double>(n, T, h_prog, d_chain, h_chain, (const double*)trajs, batch,
                                  batch_offset, (const double*)spheres, n_spheres,
                                  (const double*)is_weights, rows_per_particle, is_dt, (double*)costs,
                                  costs64, stream, tg, picked);
    else
        e = cost_dispatch<float>(n, T, h_prog, d_chain, h_chain, (const float*)trajs, batch,
                                 batch_offset, (const float*)spheres, n_spheres, (const float*)is_weights,
                                 rows_per_particle, is_dt, (float*)costs, costs64, stream, tg, picked);
    // end-effector goal terms act on the last waypoint only: one thread per trajectory, added to
    // the costs the sweep has just written (same stream)
    for (int i = 0; i < h_prog.n_terms && e == hipSuccess; ++i)
        if (h_prog.terms[i].kind == SGPMP_COST_EE_GOAL)
            e = launch_ee_goal(dtype, n, T, h_prog.terms[i], d_chain, trajs, batch, costs, costs64, stream);
    // body collision spheres (SGPMP_COST_BODY_SDF): the sweep skips the kind; body_cost_kernel (body_sdf.hip) adds the term to
    // the costs in the same way, one wave per trajectory
    // the body's sphere pairs (SGPMP_COST_BODY_SELF): likewise body_self_cost_kernel (body_self.hip); the two kinds in program order
    for (int i = 0; i < h_prog.n_terms && e == hipSuccess; ++i)
        if (h_prog.terms[i].kind == SGPMP_COST_BODY_SDF) {
            if (!launch_body_cost) return hipErrorInvalidValue;      // (a build without body_sdf.hip: sgpmp_set_costs has refused)
            e = launch_body_cost(dtype, n, T, h_prog.terms[i], d_chain, trajs, batch, costs, costs64, stream);
            if (e == hipSuccess && picked) *picked = body_sweep_name(*picked);
        } else if (h_prog.terms[i].kind == SGPMP_COST_BODY_SELF) {
            if (!launch_body_self_cost) return hipErrorInvalidValue; // (a build without body_self.hip: likewise)
            e = launch_body_self_cost(dtype, n, T, h_prog.terms[i], d_chain, trajs, batch, costs, costs64, stream);
            if (e == hipSuccess && picked) *picked = body_self_sweep_name(*picked);
        }
    return e;
}

// ---------------------------------------------------------------------------------- EE goal term
// CostGoal + EESE3DistanceField (cost_functions.py:308-321, fields.py:146-150): K * dist^2 on the last
// waypoint, dist = SE3_distance(H_ee, H_target).  SE3_distance is third-party (torch_robotics) and
// un-vendored; this build defines it as  w_pos |p - p*| + w_rot angle(R*^T R)  (DESIGN.md).
// (EeTarget, se3_distance and the row's cost ee_goal_add live in update_common.h: update_kernel evaluates the term itself when it
// is the step's only end-effector goal -- one launch less per iteration)
template <typename real>
__global__ void ee_goal_kernel(int n, int T, const ChainDev* __restrict__ ch, const real* __restrict__ trajs,
                               long long batch, EeTarget<real> tg, real* __restrict__ costs,
                               double* __restrict__ costs64) {
    __shared__ real jr[SGPMP_MAX_JOINTS * SGPMP_EE_JR];
    __shared__ int ji[SGPMP_MAX_JOINTS * 2];
    ee_stage_chain<real>(ch, jr, ji, threadIdx.x, blockDim.x);
    const int nj = ch->n_joints;
    __syncthreads();
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const double add = ee_goal_add<real>(jr, ji, nj, trajs + ((size_t)b * T + (T - 1)) * 2 * n, tg);
    if (costs) costs[b] = (real)((double)costs[b] + add);
    if (costs64) costs64[b] += add;
}

hipError_t launch_ee_goal(int dtype, int n, int T, const CostTerm& term, const ChainDev* d_chain,
                          const void* trajs, long long batch, void* costs, double* costs64,
                          hipStream_t stream) {
    const int block = 128;
    const unsigned grid = (unsigned)((batch + block - 1) / block);
    if (grid == 0) return hipSuccess;
    if (dtype == SGPMP_F64)
        hipLaunchKernelGGL((ee_goal_kernel<double>), dim3(grid), dim3(block), 0, stream, n, T, d_chain,
                           (const double*)trajs, batch, make_ee_target<double>(term), (double*)costs, costs64);
    else
        hipLaunchKernelGGL((ee_goal_kernel<float>), dim3(grid), dim3(block), 0, stream, n, T, d_chain,
                           (const float*)trajs, batch, make_ee_target<float>(term), (float*)costs, costs64);
    return hipGetLastError();
}

// Value and joint-space gradient of the end-effector field (EESE3DistanceField.compute_cost, fields.py:146-150, at
// this build's SE(3) distance d = w_pos |p - p*| + w_rot theta, theta = angle(R*^T R)): what
// FieldFactor.get_error(calc_jacobian=True) (field_factor.py:34-38) obtains with torch.autograd.grad for
// CostGoal.get_linear_system (cost_functions.py:323-337).  For a revolute joint j (axis z_j through o_j, world frame)
//   d|p - p*| / dq_j = u . (z_j x (p - o_j)),  u = (p - p*) / |p - p*|
//   d theta / dq_j   = z_j . a,                a = axis of E = R R*^T = vee(E - E^T) / |vee(E - E^T)|
// (dR/dq_j = [z_j]x R, tr([z]x E) = -z . vee(E - E^T), vee(E - E^T) = 2 sin(theta) a).  Both directions are taken as
// 0 where they are undefined (|p - p*| = 0, theta = 0 or pi).  traj_T = 0: q is [B,n]; traj_T = T: q is a
// trajectory batch [B,T,2n] and the configuration is its LAST waypoint.  value[b * out_stride + out_offset],
// grad[(b * out_stride + out_offset) * n + k].
template <typename real>
__global__ void ee_grad_kernel(int n, int traj_T, const ChainDev* __restrict__ ch, const real* __restrict__ q,
                               long long batch, EeTarget<real> tg, long long out_stride, long long out_offset,
                               real* __restrict__ value, real* __restrict__ grad) {
    using O = RealOps<real>;
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const real* qb = traj_T > 0 ? q + ((size_t)b * traj_T + (traj_T - 1)) * 2 * n : q + (size_t)b * n;
    real Z[SGPMP_MAX_JOINTS][3], Oj[SGPMP_MAX_JOINTS][3];
    real R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0};
    const int nj = ch->n_joints;
    for (int j = 0; j < nj; ++j) {
        const JointDev& J = ch->j[j];
        real F[9], tt[3], Rn[9];
        for (int i = 0; i < 9; ++i) F[i] = (real)J.R[i];
        for (int i = 0; i < 3; ++i) tt[i] = (real)J.t[i];
        for (int r = 0; r < 3; ++r) p[r] += R[r * 3 + 0] * tt[0] + R[r * 3 + 1] * tt[1] + R[r * 3 + 2] * tt[2];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c)
                Rn[r * 3 + c] = R[r * 3 + 0] * F[c] + R[r * 3 + 1] * F[3 + c] + R[r * 3 + 2] * F[6 + c];
        for (int r = 0; r < 3; ++r) { Z[j][r] = Rn[r * 3 + 2]; Oj[j][r] = p[r]; }     // joint axis and origin
        if (J.revolute) {
            real sn, cs;
            O::sincos_(qb[J.qidx], &sn, &cs);
            for (int r = 0; r < 3; ++r) {
                const real aa = Rn[r * 3 + 0], bb = Rn[r * 3 + 1];
                Rn[r * 3 + 0] = aa * cs + bb * sn;
                Rn[r * 3 + 1] = bb * cs - aa * sn;
            }
        }
        for (int i = 0; i < 9; ++i) R[i] = Rn[i];
    }
    // distance and its directions
    const real dx = p[0] - tg.p[0], dy = p[1] - tg.p[1], dz = p[2] - tg.p[2];
    const real dpos = O::sqrt_(dx * dx + dy * dy + dz * dz);
    real tr = 0;
    for (int i = 0; i < 9; ++i) tr += R[i] * tg.R[i];
    const real cth = fmin(fmax((tr - (real)1) * (real)0.5, (real)-1), (real)1);
    const real dist = tg.w_pos * dpos + tg.w_rot * acos(cth);
    real E[9];                                                             // E = R R*^T
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            E[r * 3 + c] = R[r * 3 + 0] * tg.R[c * 3 + 0] + R[r * 3 + 1] * tg.R[c * 3 + 1] + R[r * 3 + 2] * tg.R[c * 3 + 2];
    real w[3] = {E[7] - E[5], E[2] - E[6], E[3] - E[1]};
    const real wn = O::sqrt_(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const bool interior = cth > (real)-1 && cth < (real)1 && wn > (real)0;   // (acos has no slope to offer at +-1)
    const real outer = tg.square ? (real)2 * dist : (real)1;                 // d f / d dist
    const real su = dpos > (real)0 ? outer * tg.w_pos / dpos : (real)0;
    const real sa = interior ? outer * tg.w_rot / wn : (real)0;
    const real gp[3] = {su * dx, su * dy, su * dz};                          // d f / d p
    const real ta[3] = {sa * w[0], sa * w[1], sa * w[2]};                    // d f / d (rotation vector)
    const size_t o = (size_t)(b * out_stride + out_offset);
    if (value) value[o] = tg.square ? dist * dist : dist;
    real* gb = grad + o * n;
    for (int k = 0; k < n; ++k) gb[k] = 0;
    for (int j = 0; j < nj; ++j) {
        if (!ch->j[j].revolute) continue;
        const real rx = p[0] - Oj[j][0], ry = p[1] - Oj[j][1], rz = p[2] - Oj[j][2];
        const real cx = Z[j][1] * rz - Z[j][2] * ry, cy = Z[j][2] * rx - Z[j][0] * rz, cz = Z[j][0] * ry - Z[j][1] * rx;
        gb[ch->j[j].qidx] += gp[0] * cx + gp[1] * cy + gp[2] * cz + Z[j][0] * ta[0] + Z[j][1] * ta[1] + Z[j][2] * ta[2];
    }
}

hipError_t launch_ee_grad(int dtype, int n, const CostTerm& term, const ChainDev* d_chain, const void* q,
                          long long batch, int traj_T, long long out_stride, long long out_offset, void* value,
                          void* grad, hipStream_t stream) {
    const int block = 64;
    const unsigned grid = (unsigned)((batch + block - 1) / block);
    if (grid == 0) return hipSuccess;
    if (dtype == SGPMP_F64)
        hipLaunchKernelGGL((ee_grad_kernel<double>), dim3(grid), dim3(block), 0, stream, n, traj_T, d_chain,
                           (const double*)q, batch, make_ee_target<double>(term), out_stride, out_offset,
                           (double*)value, (double*)grad);
    else
        hipLaunchKernelGGL((ee_grad_kernel<float>), dim3(grid), dim3(block), 0, stream, n, traj_T, d_chain,
                           (const float*)q, batch, make_ee_target<float>(term), out_stride, out_offset,
                           (float*)value, (float*)grad);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------- standalone ops
// FK callable: q [B,n] -> frames [B,L,4,4]  (cost_functions.py:51-52).
template <typename real>
__global__ void fk_frames_kernel(int n, const ChainDev* __restrict__ ch, const real* __restrict__ q,
                                 long long batch, real* __restrict__ frames) {
    using O = RealOps<real>;
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const int L = ch->n_joints + 1;
    real R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0};
    real* out = frames + (size_t)b * L * 16;
    auto emit = [&](int l) {
        real* o = out + l * 16;
        for (int r = 0; r < 3; ++r) {
            o[r * 4 + 0] = R[r * 3 + 0]; o[r * 4 + 1] = R[r * 3 + 1]; o[r * 4 + 2] = R[r * 3 + 2];
            o[r * 4 + 3] = p[r];
        }
        o[12] = 0; o[13] = 0; o[14] = 0; o[15] = 1;
    };
    emit(0);
    for (int j = 0; j < ch->n_joints; ++j) {
        const JointDev& J = ch->j[j];
        real F[9], tt[3], Rn[9];
        for (int i = 0; i < 9; ++i) F[i] = (real)J.R[i];
        for (int i = 0; i < 3; ++i) tt[i] = (real)J.t[i];
        for (int r = 0; r < 3; ++r) p[r] += R[r * 3 + 0] * tt[0] + R[r * 3 + 1] * tt[1] + R[r * 3 + 2] * tt[2];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c)
                Rn[r * 3 + c] = R[r * 3 + 0] * F[c] + R[r * 3 + 1] * F[3 + c] + R[r * 3 + 2] * F[6 + c];
        if (J.revolute) {
            real s, c;
            O::sincos_(q[(size_t)b * n + J.qidx], &s, &c);
            for (int r = 0; r < 3; ++r) {
                const real aa = Rn[r * 3 + 0], bb = Rn[r * 3 + 1];
                Rn[r * 3 + 0] = aa * c + bb * s;
                Rn[r * 3 + 1] = bb * c - aa * s;
            }
        }
        for (int i = 0; i < 9; ++i) R[i] = Rn[i];
        emit(j + 1);
    }
}

hipError_t launch_fk(int dtype, int n, const ChainDev* d_chain, int n_links, const void* q,
                     long long batch, void* frames, hipStream_t stream) {
    const int block = 128;
    const unsigned grid = (unsigned)((batch + block - 1) / block);
    if (grid == 0) return hipSuccess;
    if (dtype == SGPMP_F64)
        hipLaunchKernelGGL((fk_frames_kernel<double>), dim3(grid), dim3(block), 0, stream, n, d_chain,
                           (const double*)q, batch, (double*)frames);
    else
        hipLaunchKernelGGL((fk_frames_kernel<float>), dim3(grid), dim3(block), 0, stream, n, d_chain,
                           (const float*)q, batch, (float*)frames);
    return hipGetLastError();
}

template <typename real>
__global__ void grid_lookup_kernel(const TermK<real> tm, const real* __restrict__ xy, long long batch,
                                   real* __restrict__ out) {
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    out[b] = grid_value<real>(tm, xy[2 * b], xy[2 * b + 1]);
}

hipError_t launch_grid_lookup(int dtype, const CostTerm& term, const void* xy, long long batch,
                              void* out, hipStream_t stream) {
    const int block = 256;
    const unsigned grid = (unsigned)((batch + block - 1) / block);
    if (grid == 0) return hipSuccess;
    if (dtype == SGPMP_F64)
        hipLaunchKernelGGL((grid_lookup_kernel<double>), dim3(grid), dim3(block), 0, stream,
                           make_termk<double>(term), (const double*)xy, batch, (double*)out);
    else
        hipLaunchKernelGGL((grid_lookup_kernel<float>), dim3(grid), dim3(block), 0, stream,
                           make_termk<float>(term), (const float*)xy, batch, (float*)out);
    return hipGetLastError();
}

// LinkDistanceField / LinkSelfDistanceField.compute_cost on explicit frames [B,L,4,4] -> [B].
template <typename real>
__global__ void field_eval_kernel(const TermK<real> tm, const real* __restrict__ frames, long long batch,
                                  int n_links, const real* __restrict__ sph, int n_sph,
                                  real* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    real* col = reinterpret_cast<real*>(lds_raw) + threadIdx.x;
    const int stride = blockDim.x;
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long bb = b < batch ? b : batch - 1;
    const real* f = frames + (size_t)bb * n_links * 16;
    for (int l = 0; l < n_links; ++l)
        for (int c = 0; c < 3; ++c) col[(l * 3 + c) * stride] = f[l * 16 + c * 4 + 3];
    if (tm.n_interp > 0) add_interp_points<real>(tm, n_links, col, stride);
    real v;
    if (tm.kind == SGPMP_COST_SPHERES) v = spheres_field<real>(tm, tm.n_points, col, stride, sph, n_sph);
    else if (tm.kind == SGPMP_COST_VOXEL_SDF) v = voxel_field<real>(tm, tm.n_points, col, stride);
    else v = self_field<real>(tm, tm.n_points, col, stride);
    if (b < batch) out[b] = v;
}

// LinkDistanceField.distances / compute_collision / compute_distance (fields.py:40-61) and the same three of
// LinkSelfDistanceField (fields.py:100-112) on explicit frames [B,L,4,4]; no interpolated points there.
//   other = spheres [O,4]:  D[l][o] = |p_l - c_o| - r_o                       (n_other = O)
//   other = null (self):    D[i][j] = |p_i - p_j|                             (n_other = L)
//   mode 0: out [B,L,n_other] = D;  mode 1: out [B] = any(D < buffer) -- self: over the pairs i - j >= 2 only
//   (torch.tril(.., diagonal=-2), fields.py:106);  mode 2: out [B] = sum of D.
// One thread per (configuration, link) in mode 0, per configuration otherwise.
template <typename real>
__global__ void link_dist_kernel(const real* __restrict__ frames, long long batch, int n_links,
                                 const real* __restrict__ sph, int n_other, int mode, real buffer,
                                 real* __restrict__ out) {
    using O = RealOps<real>;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = mode == 0 ? batch * n_links : batch;
    if (i >= total) return;
    const long long b = mode == 0 ? i / n_links : i;
    const real* f = frames + (size_t)b * n_links * 16;
    const int l0 = mode == 0 ? (int)(i - b * n_links) : 0, l1 = mode == 0 ? l0 + 1 : n_links;
    real acc = 0;
    bool hit = false;
    for (int l = l0; l < l1; ++l) {
        const real px = f[l * 16 + 3], py = f[l * 16 + 7], pz = f[l * 16 + 11];
        for (int o = 0; o < n_other; ++o) {
            real cx, cy, cz, r = 0;
            if (sph) { cx = sph[o * 4]; cy = sph[o * 4 + 1]; cz = sph[o * 4 + 2]; r = sph[o * 4 + 3]; }
            else { cx = f[o * 16 + 3]; cy = f[o * 16 + 7]; cz = f[o * 16 + 11]; }
            const real dx = px - cx, dy = py - cy, dz = pz - cz;
            const real dist = O::sqrt_(dx * dx + dy * dy + dz * dz) - r;
            if (mode == 0) out[(size_t)i * n_other + o] = dist;
            acc += dist;
            if (dist < buffer && (sph || l - o >= 2)) hit = true;
        }
    }
    if (mode == 1) out[i] = hit ? (real)1 : (real)0;
    if (mode == 2) out[i] = acc;
}

hipError_t launch_link_dist(int dtype, const void* frames, long long batch, int n_links, const void* spheres,
                            int n_other, int mode, double buffer, void* out, hipStream_t stream) {
    const long long total = mode == 0 ? batch * n_links : batch;
    if (total <= 0) return hipSuccess;
    const int block = 64;
    const unsigned grid = (unsigned)((total + block - 1) / block);
    if (dtype == SGPMP_F64)
        hipLaunchKernelGGL((link_dist_kernel<double>), dim3(grid), dim3(block), 0, stream, (const double*)frames, batch,
                           n_links, (const double*)spheres, n_other, mode, buffer, (double*)out);
    else
        hipLaunchKernelGGL((link_dist_kernel<float>), dim3(grid), dim3(block), 0, stream, (const float*)frames, batch,
                           n_links, (const float*)spheres, n_other, mode, (float)buffer, (float*)out);
    return hipGetLastError();
}

// EESE3DistanceField.compute_cost on explicit frames [B,L,4,4]: distance of the LAST link frame.
template <typename real>
__global__ void ee_field_kernel(EeTarget<real> tg, const real* __restrict__ frames, long long batch, int n_links,
                                real* __restrict__ out) {
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const real* f = frames + ((size_t)b * n_links + (n_links - 1)) * 16;
    real R[9], p[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) R[r * 3 + c] = f[r * 4 + c];
        p[r] = f[r * 4 + 3];
    }
    real dist = se3_distance<real>(R, p, tg);
    if (tg.square) dist = dist * dist;
    out[b] = dist;
}

// ---------------------------------------------------------------------------------- field Jacobians
// FieldFactor.get_error(calc_jacobian=True) (field_factor.py:28-38): the field value at a batch of
// joint configurations q [B,n] and its gradient with respect to q, analytically instead of through
// autograd.  The field is a function of the link positions p_l(q); with g_l = df/dp_l,
//   df/dq_j = z_j . sum_{l after joint j} (p_l - o_j) x g_l = z_j . (M_j - o_j x F_j),
// F_j = sum g_l, M_j = sum p_l x g_l over the links behind revolute joint j (axis z_j through o_j),
// accumulated from the end effector backwards.  Interpolated link points (fields.py:68-74) hand their
// gradient to the two links they lie between.  One thread per configuration; any joint order.
// NJ > 0: chain length known at compile time and no interpolated points -- every loop unrolls and the
// per-thread arrays live in registers (NJ = 0 is the generic form, whose arrays go to scratch).
template <typename real, int NJ>
__global__ void __launch_bounds__(64)
field_grad_kernel(const ChainDev* __restrict__ ch, TermK<real> tm, int n, const real* __restrict__ q,
                  long long batch, int traj_T, const real* __restrict__ spheres, int n_spheres,
                  real* __restrict__ value, real* __restrict__ grad) {
    using O = RealOps<real>;
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    // traj_T = 0: q is [B, n].  traj_T = T: q is a trajectory batch [P, T, 2n] and configuration b is
    // waypoint 1 + b % (T-1) of trajectory b / (T-1) (the waypoint range of CostCollision)
    const real* qb = traj_T > 0 ? q + ((size_t)(b / (traj_T - 1)) * traj_T + 1 + b % (traj_T - 1)) * 2 * n
                                : q + (size_t)b * n;
    const int nj = NJ > 0 ? NJ : ch->n_joints;
    constexpr int MP = NJ > 0 ? NJ + 1 : SGPMP_MAX_POINTS;
    constexpr int MJ = NJ > 0 ? NJ : SGPMP_MAX_JOINTS;
    real P[MP][3], G[MP][3];
    real Z[MJ][3], Oj[MJ][3];
    real R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0};
    P[0][0] = P[0][1] = P[0][2] = 0;
#pragma unroll
    for (int j = 0; j < nj; ++j) {
        const JointDev& J = ch->j[j];
        real F[9], tt[3], Rn[9];
        for (int i = 0; i < 9; ++i) F[i] = (real)J.R[i];
        for (int i = 0; i < 3; ++i) tt[i] = (real)J.t[i];
        for (int r = 0; r < 3; ++r) p[r] += R[r * 3 + 0] * tt[0] + R[r * 3 + 1] * tt[1] + R[r * 3 + 2] * tt[2];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c)
                Rn[r * 3 + c] = R[r * 3 + 0] * F[c] + R[r * 3 + 1] * F[3 + c] + R[r * 3 + 2] * F[6 + c];
        for (int r = 0; r < 3; ++r) { Z[j][r] = Rn[r * 3 + 2]; Oj[j][r] = p[r]; }     // joint axis and origin
        if (J.revolute) {
            real sn, cs;
            O::sincos_(qb[J.qidx], &sn, &cs);
            for (int r = 0; r < 3; ++r) {
                const real aa = Rn[r * 3 + 0], bb = Rn[r * 3 + 1];
                Rn[r * 3 + 0] = aa * cs + bb * sn;
                Rn[r * 3 + 1] = bb * cs - aa * sn;
            }
        }
        for (int i = 0; i < 9; ++i) R[i] = Rn[i];
        for (int r = 0; r < 3; ++r) P[j + 1][r] = p[r];
    }
    const int n_links = nj + 1;
    int npts = n_links;
    if (NJ == 0 && tm.n_interp > 0)
        for (int i = tm.interp_lo; i < tm.interp_hi; ++i)
            for (int a = 0; a < tm.n_interp; ++a, ++npts)
                for (int r = 0; r < 3; ++r) P[npts][r] = P[i][r] + (P[i + 1][r] - P[i][r]) * tm.alpha[a];
#pragma unroll
    for (int l = 0; l < npts; ++l) G[l][0] = G[l][1] = G[l][2] = 0;
    real val = 0;
    if (tm.kind == SGPMP_COST_SPHERES && (tm.flags & 15) == SGPMP_FIELD_SDF) {
        // sdf (fields.py:79-83): value = max over (point, sphere) of r - dist (clamped from above at 0 with
        // clamp_sdf).  The reference differentiates it by autograd (field_factor.py:35): the gradient is that of
        // the arg-max pair -- torch's max(-1)[0].max(-1)[0] keeps the FIRST maximum, spheres within a point
        // first, then points, hence point-major order and a strict comparison here -- i.e. -(p - c)/dist on that
        // point, and exactly zero where the clamp is active (clamp(max=0) passes the gradient for sdf <= 0).
        const bool clampv = (tm.flags & SGPMP_FLAG_SDF_CLAMP) != 0;
        real best = (real)-__builtin_inff();
        int bl = 0;
        real bg[3] = {0, 0, 0};
#pragma unroll
        for (int l = 0; l < npts; ++l)
            for (int o = 0; o < n_spheres; ++o) {
                const real dx = P[l][0] - spheres[o * 4], dy = P[l][1] - spheres[o * 4 + 1], dz = P[l][2] - spheres[o * 4 + 2];
                const real dist = O::sqrt_(dx * dx + dy * dy + dz * dz);
                real sd = spheres[o * 4 + 3] - dist;
                const bool cut = clampv && sd > (real)0;
                if (cut) sd = 0;
                if (sd > best) {
                    best = sd; bl = l;
                    const real w = cut ? (real)0 : (real)-1 / dist;
                    bg[0] = w * dx; bg[1] = w * dy; bg[2] = w * dz;
                }
            }
        val = best;
#pragma unroll
        for (int l = 0; l < npts; ++l)
            if (l == bl) { G[l][0] = bg[0]; G[l][1] = bg[1]; G[l][2] = bg[2]; }
    } else if (tm.kind == SGPMP_COST_SPHERES) {              // rbf (occupancy is refused by the host)
        for (int o = 0; o < n_spheres; ++o) {
            const real cx = spheres[o * 4], cy = spheres[o * 4 + 1], cz = spheres[o * 4 + 2], rr = spheres[o * 4 + 3];
            const real ir2 = (real)1 / (rr * rr);
#pragma unroll
            for (int l = 0; l < npts; ++l) {
                const real dx = P[l][0] - cx, dy = P[l][1] - cy, dz = P[l][2] - cz;
                const real e = O::exp_((real)-0.5 * (dx * dx + dy * dy + dz * dz) * ir2);
                val += e;
                const real w = -e * ir2;
                G[l][0] += w * dx; G[l][1] += w * dy; G[l][2] += w * dz;
            }
        }
    } else if (tm.kind == SGPMP_COST_VOXEL_SDF) {
        if (tm.flags & SGPMP_FLAG_GRID_DISTANCE) {
            // the query: min over the points of the interpolated distance d and dd/dp on the FIRST arg-min point (point order,
            // strict comparison); a NaN distance anywhere makes the value and the gradient NaN
            real best = (real)__builtin_inff(), bad = 0;
            int bl = 0;
            real bg[3] = {0, 0, 0};
#pragma unroll
            for (int l = 0; l < npts; ++l) {
                real dd[3];
                const real d = voxel_sdf_distance<real, true>(tm, P[l][0], P[l][1], P[l][2], dd);
                if (!(d == d)) bad = d;
                if (d < best) { best = d; bl = l; bg[0] = dd[0]; bg[1] = dd[1]; bg[2] = dd[2]; }
            }
            const bool nan = !(bad == bad);
            val = nan ? bad : best;
#pragma unroll
            for (int l = 0; l < npts; ++l)
                if (l == bl) { G[l][0] = nan ? bad : bg[0]; G[l][1] = nan ? bad : bg[1]; G[l][2] = nan ? bad : bg[2]; }
        } else {
#pragma unroll
            for (int l = 0; l < npts; ++l) val += voxel_sdf_field<real, true>(tm, P[l][0], P[l][1], P[l][2], G[l]);
        }
    } else {                                                 // SELF: the full L x L sum of fields.py:124
        // = diagonal (value 1 each, no gradient) + twice the strict lower triangle
        val = (real)npts;
#pragma unroll
        for (int i = 1; i < npts; ++i)
#pragma unroll
            for (int j = 0; j < i; ++j) {
                const real dx = P[i][0] - P[j][0], dy = P[i][1] - P[j][1], dz = P[i][2] - P[j][2];
                const real e = O::exp_((dx * dx + dy * dy + dz * dz) * tm.K2);
                val += (real)2 * e;
                const real w = (real)4 * tm.K2 * e;
                G[i][0] += w * dx; G[i][1] += w * dy; G[i][2] += w * dz;
                G[j][0] -= w * dx; G[j][1] -= w * dy; G[j][2] -= w * dz;
            }
    }
    if (NJ == 0 && tm.n_interp > 0) {                                   // interpolated points -> their two links
        int m = n_links;
        for (int i = tm.interp_lo; i < tm.interp_hi; ++i)
            for (int a = 0; a < tm.n_interp; ++a, ++m)
                for (int r = 0; r < 3; ++r) {
                    G[i][r] += ((real)1 - tm.alpha[a]) * G[m][r];
                    G[i + 1][r] += tm.alpha[a] * G[m][r];
                }
    }
    if (value) value[b] = val;
    real Fs[3] = {0, 0, 0}, Ms[3] = {0, 0, 0};
    real* gb = grad + (size_t)b * n;
    for (int k = 0; k < n; ++k) gb[k] = 0;
#pragma unroll
    for (int j = nj - 1; j >= 0; --j) {
        const int l = j + 1;
        Fs[0] += G[l][0]; Fs[1] += G[l][1]; Fs[2] += G[l][2];
        Ms[0] += P[l][1] * G[l][2] - P[l][2] * G[l][1];
        Ms[1] += P[l][2] * G[l][0] - P[l][0] * G[l][2];
        Ms[2] += P[l][0] * G[l][1] - P[l][1] * G[l][0];
        if (ch->j[j].revolute) {
            const real ox = Oj[j][0], oy = Oj[j][1], oz = Oj[j][2];
            const real tx = Ms[0] - (oy * Fs[2] - oz * Fs[1]);
            const real ty = Ms[1] - (oz * Fs[0] - ox * Fs[2]);
            const real tz = Ms[2] - (ox * Fs[1] - oy * Fs[0]);
            gb[ch->j[j].qidx] += Z[j][0] * tx + Z[j][1] * ty + Z[j][2] * tz;
        }
    }
}

hipError_t launch_field_grad(int dtype, int n, const CostTerm& term, const ChainDev* d_chain, int n_joints,
                             const void* q, long long batch, int traj_T, const void* spheres, int n_spheres,
                             void* value, void* grad, hipStream_t stream) {
    const int block = 64;
    const unsigned grid = (unsigned)((batch + block - 1) / block);
    if (grid == 0) return hipSuccess;
#define FG_LAUNCH(REAL, NJ)                                                                         \
    hipLaunchKernelGGL((field_grad_kernel<REAL, NJ>), dim3(grid), dim3(block), 0, stream, d_chain,  \
                       make_termk<REAL>(term), n, (const REAL*)q, batch, traj_T, (const REAL*)spheres, \
                       n_spheres, (REAL*)value, (REAL*)grad)
    const int nj = term.n_interp > 0 ? 0 : n_joints;       // specialised chain lengths: 10 (Panda), 7
    if (dtype == SGPMP_F64) {
        if (nj == 10) FG_LAUNCH(double, 10); else if (nj == 7) FG_LAUNCH(double, 7); else FG_LAUNCH(double, 0);
    } else {
        if (nj == 10) FG_LAUNCH(float, 10); else if (nj == 7) FG_LAUNCH(float, 7); else FG_LAUNCH(float, 0);
    }
#undef FG_LAUNCH
    return hipGetLastError();
}

hipError_t launch_field_eval(int dtype, const CostTerm& term, const void* frames, long long batch,
                             int n_links, const void* spheres, int n_spheres, void* out,
                             hipStream_t stream) {
    const int block = 64;
    const unsigned grid = (unsigned)((batch + block - 1) / block);
    if (grid == 0) return hipSuccess;
    if (term.kind == SGPMP_COST_EE_GOAL) {
        if (dtype == SGPMP_F64)
            hipLaunchKernelGGL((ee_field_kernel<double>), dim3(grid), dim3(block), 0, stream,
                               make_ee_target<double>(term), (const double*)frames, batch, n_links, (double*)out);
        else
            hipLaunchKernelGGL((ee_field_kernel<float>), dim3(grid), dim3(block), 0, stream,
                               make_ee_target<float>(term), (const float*)frames, batch, n_links, (float*)out);
        return hipGetLastError();
    }
    const size_t esz = dtype == SGPMP_F64 ? 8 : 4;
    const size_t lds = (size_t)term.n_points * 3 * block * esz;
    if (dtype == SGPMP_F64)
        hipLaunchKernelGGL((field_eval_kernel<double>), dim3(grid), dim3(block), lds, stream,
                           make_termk<double>(term), (const double*)frames, batch, n_links,
                           (const double*)spheres, n_spheres, (double*)out);
    else
        hipLaunchKernelGGL((field_eval_kernel<float>), dim3(grid), dim3(block), lds, stream,
                           make_termk<float>(term), (const float*)frames, batch, n_links,
                           (const float*)spheres, n_spheres, (float*)out);
    return hipGetLastError();
}
