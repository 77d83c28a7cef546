// K2 + K3 FUSED: draw the samples and evaluate their costs in ONE launch (SURVEY.md section 7 step 6:
// "samples written once, read never by K3").
//
// Replaces, per planner iteration, MultiMPPrior.sample (mp_priors_multi.py:204-207) AND
// CostComposite.eval + the importance-sampling term (cost_functions.py:47-58, planner.py:229-237) for
// the configurations the two-trajectory sweep covers (fp32, generated chain code, flat program without
// a grid term, isotropic sampling prior, in-kernel noise, S a multiple of 8, T a multiple of 16).
// Separately, K2 writes 470 MB and K3 reads them back; both are VALU-bound (Philox / FK + exp), so
// the fusion does not shorten the arithmetic -- it removes the 470 MB read, K3's whole load pipeline
// (global_load_lds staging, its waits) and one kernel boundary.  The samples are still WRITTEN (K4 reads
// the rows that carry weight; optimize() returns them), as stores that nothing waits for.
//
// One wave = 8 samples (4 pairs) of one particle, walked in chunks of 16 waypoints through a
// wave-private LDS tile [8 rows][carry waypoint | 16 waypoints][d]:
//   phase A  lane = (sample, dof): Philox + Box-Muller noise and the 7-FMA recurrence
//            y_t = G_t eps_t + H_t y_{t-1} of the scan sampler (sampler.hip; identical expressions and
//            counter layout, so the samples are bit-identical to sgpmp_sample's) -> tile rows;
//   phase B  lane = (row, 16-byte column): x = mu + y, stored to HBM (eight 128-byte lines per wave
//            instruction) and written back into the tile;
//   phase C  lane = (pair, waypoint): the cost terms of cost_sweep_dual.inc on packed fp32 for rows
//            2j, 2j+1 -- the DPP row of 16 lanes IS the chunk, x_{t-1} comes from the tile (the slot in
//            front of the chunk holds the previous chunk's last waypoint; zeros before t = 0, which
//            also makes the t = 0 row of the importance-sampling product the general expression);
//            costs accumulate per lane over the chunks and are reduced once per item inside each row.
// Every global LOAD of a chunk (means, importance-sampling weights) is issued at the top of the chunk,
// before its stores: on gfx9 stores count in vmcnt, in order, so a load issued behind a store cannot be
// waited for without also waiting for that store's HBM round trip.
#define SGPMP_FUSED_TC 16
#define SGPMP_FUSED_SPW 8
// LDS budget: 4 workgroups per CU need <= 40960 B each; tiles 30720 + staging 7168 + spheres 2048 + start/goal rows 960
// + 16 = 40912.  (SURVEY 8d's stress variant has 64 spheres; the reference example has 5.)
#ifndef SGPMP_FUSED_SPH
#define SGPMP_FUSED_SPH 64            // spheres staged in LDS (more: the step runs unfused)
#endif
#ifndef SGPMP_FUSED_GOALS
#define SGPMP_FUSED_GOALS 14          // goal states staged in LDS (more: unfused)
#endif

template <bool B> struct BoolC { static constexpr bool value = B; };
// a has_* flag of the cost program: read at run time, or a compile-time fact (chunked_body: FULL)
template <int FULL> __device__ __forceinline__ int prog_has(int flag) { if constexpr (FULL != 0) return 1; else return flag; }

// x^2 + y^2 + z^2 in ONE evaluation order.  Written as a sum of three products hipcc is free to decide which product becomes
// the addend of which fma -- and decided differently from one instantiation of chunked_body to another (round 5: the small-step
// launch's sphere terms came out one ulp off the one-wave launch's in 0.1 % of the costs).
__device__ __forceinline__ float sq3(float x, float y, float z) { return __builtin_fmaf(z, z, __builtin_fmaf(y, y, x * x)); }
__device__ __forceinline__ f2 sq3(f2 x, f2 y, f2 z) { return __builtin_elementwise_fma(z, z, __builtin_elementwise_fma(y, y, x * x)); }

// The update INSIDE fused_planar_seg_kernel (store-free steps of problems whose particles have exactly the 64 samples of one
// workgroup; fused_planar_seg.inc: seg_update): what update_kernel would have been given.
struct SegTail {
    unsigned* done;             // particles updated so far in this launch (zero between launches); null: update_kernel follows the launch
    double* acc;                // [SGPMP_STAT_SHARDS][4] statistics accumulators of the context (zero between launches)
    double* stats_out;          // the step's statistics buffer (written by the launch's last particle), or null
    float* means;               // [P][M] in / out
    float* weights;             // [P][S] or null
    float* grad;                // [P][M] or null
    float* means_prev;          // [P][M] or null
    float* isw_next;            // [P][T+1][d]: the next step's importance-sampling weights
    unsigned* nnz_out;          // [P] rows with weight (FusedArgs::nnz_prev of the next step), or null
    const double* Qinv;
    double ks, kg, dt, temperature, step_size;
    int P;                      // particles of this launch
    int iters;                  // iterations this launch runs (fused_planar_seg.inc: PERSIST); 1: one step
};

struct FusedArgs {
    const float* coef;          // [T][8] scan coefficients of the sampling prior (K1, fp32 copy)
    const float* coefp;         // [T][8] the same in the pair order of rng.h scan_step2 (PriorDev::iso32p): fused_step_kernel's noise phase
    const float* means;         // [P][T][d]
    float* samples;             // [P][S][T][d]  out
    uint64_t seed, draw;
    int mode_offset;            // global index of local particle 0 (noise key)
    int S;                      // samples per particle (the planar launches: a multiple of 8; fused_step_kernel: any -- the rows past S of a particle's last group are computed and not written)
    int gpp;                    // item groups per particle = ceil(S / 8)
    long long nitems;           // fused_step_kernel: P * gpp
    int gpp_shift;              // log2(gpp) when a power of two, else -1
    double* zero_stats;         // this step's statistics buffer, zeroed by workgroup 0 (K4 accumulates into it)
    // Dense-weight regime of the update (planner.py:263-275 is a softmax, not an arg-min): for a particle whose PREVIOUS
    // update found its weight spread over many samples, every wave leaves a softmax partial of its 8 rows, and update_kernel
    // adds S / 8 partials instead of streaming the particle's S rows again.  part == null: never.
    float* part;                // [P][S / 8][4 + T d]: min cost of the 8 rows, sum_r e_r, 0, 0, sum_r e_r (x_r - mu), e_r = exp(-(c_r - min) / temperature)
    const unsigned* nnz_prev;   // [P] rows that carried weight in each particle's previous update (written by update_kernel)
    unsigned nnz_threshold;     // partials of particle p are written when nnz_prev[p] > nnz_threshold
    float inv_temperature;
    // Store-free step (sgpmp_step with SGPMP_STEP_NO_SAMPLES: an iteration inside optimize(opt_iters = K) whose samples nobody
    // reads -- the reference returns the last iteration's tensors only, planner.py:289-317): the rows of particle p go to memory
    // only when nnz_prev[p] > store_threshold (its previous update spread its weight: update_kernel will want many rows, or the
    // partials above, which re-read them); for every other particle update_kernel regenerates the rows that carry weight from
    // their noise keys (update_common.h: regen_rows) -- bit for bit what this launch would have stored.
    int nostore;
    unsigned store_threshold;
    SegTail tail;               // fused_planar_seg_kernel only; tail.done == null: update_kernel follows the launch
};

#ifndef SGPMP_FUSED_PRIO
#define SGPMP_FUSED_PRIO 0            // diagnostic: 1 = s_setprio 1 through the cost phase, 2 = through the noise phase (DESIGN.md 4)
#endif
#ifndef SGPMP_FUSED_COEF_X16
#define SGPMP_FUSED_COEF_X16 1
#endif
#ifndef SGPMP_FUSED_WAVES_RS
#define SGPMP_FUSED_WAVES_RS 4        // register budget of the fused launch proper (its LDS would admit 5 waves per SIMD: measured level with 4)
#endif
#ifndef SGPMP_FUSED_WAVES
#define SGPMP_FUSED_WAVES 4
#endif
#ifndef SGPMP_FUSED_XCD_MAP
#define SGPMP_FUSED_XCD_MAP 1
#endif
#ifndef SGPMP_FUSED_A_UNROLL
#define SGPMP_FUSED_A_UNROLL 4         // trips of the noise loop unrolled together (2, 4: independent Philox blocks side by side -- measured, see DESIGN 4)
#endif
#ifndef SGPMP_FUSED_SCALAR_PROLOGUE
#define SGPMP_FUSED_SCALAR_PROLOGUE 0  // 1: sphere / start / goal tables through the scalar cache when they are small -- measured level (see the prologue)
#endif
#ifndef SGPMP_FUSED_NOISE_ALL_LANES
#define SGPMP_FUSED_NOISE_ALL_LANES 0 // 1: phase A's noise on 64 lanes = (sample, waypoint pair), 7 calls (measured, not faster: see phase A); 0: 56 lanes = (sample, dof), 8 calls
#endif
// SWEEP: the cost sweep alone on samples that already exist (sgpmp_cost_eval: sample_and_eval, parity-mode
// noise, user-supplied trajectories) -- phases A and B are replaced by eight LDS-DMA row loads per chunk, phase
// C is the same code.  Rows b0 .. b0+7 of an item share their particle (importance-sampling weights) and goal.
// Diagnostic build -DFUSED_STAMPS (tools/fused_stamps.py): s_memtime cycles a wave spends in each phase, summed over its
// chunks, written over the item's first cost slots instead of costs (row 0: phase A, 1: wait + phase B, 2: phase C loads +
// quadratic forms, 3: kinematics + fields, 4: whole item, 5: start stamp mod 2^24).
#ifndef SGPMP_FUSED_STORE_BITS     // cache-policy bits of the sample stores (A/B builds: -DSGPMP_FUSED_STORE_BITS='"nt"', '"sc0 sc1"', '""' ...)
#define SGPMP_FUSED_STORE_BITS "sc1 nt"
#endif
#ifndef SGPMP_SWEEP_LOAD_AUX        // cache-policy bits of the stand-alone sweep's sample loads (LDS-DMA aux operand: 1 sc0, 2 nt, 16 sc1): the rows are
#define SGPMP_SWEEP_LOAD_AUX 2      // read once -- non-temporal: 150.0 -> 146.9 us back to back (sc1: 152.7, sc0: 154.1; profiles/r06/store_policy_ab.txt)
#endif
#ifdef FUSED_STAMPS
#define FSTAMP_DECL unsigned long long st_[6] = {0, 0, 0, 0, 0, 0}, st_t, st_0
#define FSTAMP_NOW() ([]() { unsigned long long t_; asm volatile("s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); return t_; }())
#define FSTAMP_START() do { st_t = FSTAMP_NOW(); } while (0)
#define FSTAMP(i) do { const unsigned long long n_ = FSTAMP_NOW(); st_[i] += n_ - st_t; st_t = n_; } while (0)
#else
#define FSTAMP_DECL
#define FSTAMP_START() do {} while (0)
#define FSTAMP(i) do {} while (0)
#endif

// RAG (round 4): S need not be a multiple of 8 nor T of 16 -- the rows past S of a particle's last group and the waypoints past T of
// the last chunk are computed like the others and never written nor counted.  A second instantiation, so that shapes on the
// grid run the code they always ran (the guards cost 1.3 % at config 3 when compiled into the one kernel).
// (Round 5: the re-cuts that measured level or slower -- the update inside the launch, one-wave workgroups, the scan coefficients
// from LDS, the in-wave software pipeline -- were removed from the source; DESIGN.md section 8 keeps their numbers and the
// commit that last held them.)
// (Round 5 also built the sphere field's exponent arguments on the matrix cores for >= 16 spheres -- v_mfma_f32_16x16x4_f32 per 16
// spheres x 16 waypoints -- and removed it again: on gfx950 a SIMD's fp32 MFMA and VALU instructions do not overlap and run at the
// same flop rate, so the launch moved -7 % / +3 %; profiles/r05/sphere_field_on_the_matrix_cores_negative.txt, commit 29fe316.)
// LAT (round 5): the launch of a SMALL step -- fewer items than the chip has SIMDs, every wave alone on its SIMD and the launch as
// long as ONE item takes one wave (43 k cycles, ~20 us: the reference's own example sizes, 5 particles x 32 samples, run here).
// The four waves of a workgroup then share ONE item: wave w takes the chunks w, w + 4, ... of its 8 rows -- noise for all chunks at
// once (lane = (sample, waypoint pair): no state), the recurrence chunk after chunk (the only serial part: 8 two-waypoint steps
// per chunk, the state handed on through LDS), then x = mu + y, the stores and the cost terms of all chunks side by side; wave 0
// adds the chunks' cost shares IN CHUNK ORDER.  Same counters, same expressions, same order of every sum: samples and costs are
// bit-identical to the one-wave-per-item launch (tests/test_gpu_planner.py::test_small_step_launch_*).
// FULL (round 17): the cost program and the launch's mode as compile-time facts, for the one program every Panda example and the
// headline run -- GP term with start prior, goal prior, self term and sphere term all present (prog_has), a storing launch
// (nostore == 0).  The generic instantiation keeps every alternative alive in SGPRs through the item: 84 spilled, 217
// v_readlane / v_writelane, 12 of them inside the chunk loop -- vector instructions, on a launch bound by vector issue.
// FULL = 1: no softmax partials either (part == nullptr); FULL = 2: the partials buffer stays a run-time value (default contexts
// arm it for every step on the grid).  The shift-or-divide choice of the particle and goal index stays at run time (as
// compile-time facts: 30 -> 24 spilled SGPRs, and particles of 24 samples would fall back to the generic kernel).  Same
// expressions in the same order: step_plan.hip fused_full_variant selects, tests/test_gpu_fused_full.py holds samples and costs to
// the generic instantiation's bits, profiles/r17/fused_full.txt has the counts.
template <int N, class CC, int FT, bool SWEEP, bool RAG = false, bool LAT = false, int FULL = 0>
__device__ __forceinline__ void chunked_body(const CostArgs<float>& a, const FlatProg<float>& F, const FusedArgs& s) {
    static_assert(!LAT || !SWEEP, "the small-step schedule exists for the fused launch");
    static_assert(!FULL || (!SWEEP && !RAG && !LAT), "the compiled-in program exists for the fused launch on the 8 x 16 grid");
    constexpr int D = 2 * N, TC = SGPMP_FUSED_TC, SPW = SGPMP_FUSED_SPW;
    constexpr int HEAD = ((D + 3) / 4) * 4;              // floats in front of a row's chunk: [pad | carry waypoint]
    constexpr int PITCH = HEAD + TC * D;                 // floats per tile row (16-byte multiple; 240 for d = 14)
    constexpr int V4 = TC * D / 4;                       // 16-byte columns per row chunk (56)
    constexpr int V4L = V4 / 8;                          // ... per lane (8 lanes share a row)
    static_assert(V4 % 8 == 0, "row chunk must split over 8 lanes");
    typedef float real2 __attribute__((ext_vector_type(2)));
    typedef float real4 __attribute__((ext_vector_type(4)));
    using O = RealOps<f2>;
#ifdef FUSED_STAMPS
    const unsigned long long st_entry = FSTAMP_NOW();             // kernel entry, before the prologue
    unsigned long long pro_[3] = {0, 0, 0};                       // -DFUSED_STAMPS=2: after the staging, the barrier, the static sphere sum
#define PSTAMP(i) do { pro_[i] = FSTAMP_NOW() - st_entry; } while (0)
#else
#define PSTAMP(i) do {} while (0)
#endif
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int T = a.T;

    float* sphl;                                                 // [spheres][8] sphere constants
    float* unl;                                                  // start state (row 0) and goal states, 16-float rows
    // RS (the fused launch proper): the chunk's means and importance-sampling weights wait in REGISTERS, not in an LDS staging
    // buffer (below), and the tables are sized by the launch -- 30.7 KB of tiles + 16 B + tables per four-wave workgroup: FIVE
    // workgroups share a CU's 160 KB (five waves per SIMD) while the tables stay under 2 KB (<= ~30 spheres; more: four, as before)
    constexpr int WPB = 4;                                       // waves per workgroup: the sphere / goal tables are staged once per workgroup
    constexpr bool RS = !SWEEP;
    if constexpr (!RS) {
        __shared__ __align__(16) float sphl_s[SGPMP_FUSED_SPH * 8];
        __shared__ float unl_s[(SGPMP_FUSED_GOALS + 1) * 16];
        sphl = sphl_s; unl = unl_s;
    } else {                                                     // sized by the launch: (32 B per waypoint,) 32 B per sphere, 64 B per state row
        extern __shared__ __align__(16) float fused_dyn_lds[];
        float* base = fused_dyn_lds;
        sphl = base;
        unl = base + (size_t)a.n_spheres * 8;
    }
    __shared__ float sphst[WPB];                                 // per wave: sphere sum of the links that never move
    __shared__ __align__(16) float tiles[WPB * SPW * PITCH];
    constexpr int LAT_MAXC = 16;                                 // chunks of an item the small-step schedule covers (T <= 256)
    float* lat_carry = nullptr;                                  // [chunk][lane = (sample, dof)][2]: recurrence state entering the chunk
    f2* lat_v = nullptr;                                         // [chunk][lane]: the chunk's share of the lane's cost sum
    float* lat_coef = nullptr;                                   // [chunks * TC][8]: FusedArgs::coefp, staged once per workgroup
    float* lat_mu = nullptr;                                     // per wave [2][64]: the means of the waypoint in front of the wave's chunk, lane = (sample, dof)
    if constexpr (LAT) {
        __shared__ float lat_carry_s[(LAT_MAXC + 1) * SPW * N * 2];
        __shared__ f2 lat_v_s[LAT_MAXC * 64];
        __shared__ __align__(16) float lat_coef_s[LAT_MAXC * TC * 8];
        __shared__ float lat_mu_s[WPB * 2 * 64];
        lat_carry = lat_carry_s; lat_v = lat_v_s; lat_coef = lat_coef_s; lat_mu = lat_mu_s + wave * 128;
    }
    constexpr int STG = 2 * TC * D;                              // floats of per-wave staging
    float* const tile = tiles + wave * SPW * PITCH;
    float* mul = nullptr;                                        // [TC][D] means of the chunk            } sweep only
    float* wl = nullptr;                                         // [TC][D] IS weights of the chunk       }
    if constexpr (!RS) {
        __shared__ __align__(16) float stage[WPB * STG];
        mul = stage + wave * STG;
        wl = mul + TC * D;
    }
    typedef const __attribute__((address_space(1))) void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;

    // ---- per-workgroup staging of the spheres; per-wave sphere sum of the links that never move
    // Few spheres and goals (the usual case) come in through the SCALAR cache: every new wave pays this prologue, and as
    // vector loads its two dozen words queued behind the launch's sample stores for ~7 us (tools/fused_stamps.py: 17 k
    // of a wave's 88 k cycles, round 4); the constant cache path does not share that queue and the table is hot in it.
    const int ng_ = prog_has<FULL>(F.has_goal) ? F.goal.dim0 : 0;
    const bool gp_start_ = prog_has<FULL>(F.has_gp) && (FULL || (F.gp.flags & SGPMP_FLAG_GP_START));
    const bool scalar_prologue = SGPMP_FUSED_SCALAR_PROLOGUE && a.n_spheres <= 16 && ng_ <= 3;
    auto sphere_row = [&](int o, float cx, float cy, float cz, float r) {
        if (FT == SGPMP_FIELD_RBF) {
            const float k = (float)(-0.5 * SGPMP_LOG2E) / (r * r);
            sphl[o * 8 + 0] = -2.f * k * cx;
            sphl[o * 8 + 1] = -2.f * k * cy;
            sphl[o * 8 + 2] = -2.f * k * cz;
            sphl[o * 8 + 3] = k;
            sphl[o * 8 + 4] = k * sq3(cx, cy, cz);
        } else {
            sphl[o * 8 + 0] = cx; sphl[o * 8 + 1] = cy; sphl[o * 8 + 2] = cz; sphl[o * 8 + 3] = r;
        }
    };
    // LAT: the tables' global loads are ISSUED here and COMMITTED to LDS inside the first item, behind its noise phase (which needs
    // none of them): the load round trip (2.6 k cycles: tools/fused_stamps.py, -DFUSED_STAMPS=2) is a seventh of a small step's
    // launch when the wave waits for it up front.  One sphere, one state element, two 16-byte columns of the recurrence's
    // coefficients per thread (<= 64 spheres, <= 15 state rows, T <= 256).
    // (The recurrence's coefficients need no arithmetic on the way: they go global -> LDS by LDS-DMA, which holds no registers --
    // with them in registers the kernel needed 260 and a second workgroup did not fit a CU.)
    real4 lat_sph = real4{0.f, 0.f, 0.f, 1.f};
    float lat_un = 0.f;
    const int lat_nf4 = ((a.T + TC - 1) / TC) * TC * 2;           // (the table is padded to whole chunks: api.hip alloc_prior)
    if constexpr (LAT) {
        static_assert(SGPMP_FUSED_SPH <= 64 * WPB && (SGPMP_FUSED_GOALS + 1) * 16 <= 64 * WPB && LAT_MAXC * TC * 2 <= 2 * 64 * WPB, "one trip per thread");
        const int o = threadIdx.x;
        if (o < a.n_spheres) lat_sph = real4{a.spheres[o * 4 + 0], a.spheres[o * 4 + 1], a.spheres[o * 4 + 2], a.spheres[o * 4 + 3]};
        if (o < (ng_ + 1) * 16) {
            const int r = o >> 4, e = o & 15;
            if (e < D) {
                if (r == 0) lat_un = gp_start_ ? ((const float*)F.gp.dev_data)[e] : 0.f;
                else lat_un = ((const float*)F.goal.dev_data)[(size_t)(r - 1) * D + e];
            }
        }
        // (LDS-DMA: a wave's 64 lanes land 16 bytes each at consecutive addresses from the wave-uniform LDS base)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int w0 = (u * WPB + wave) * 64;                  // first 16-byte column of this wave's trip
            if (w0 + (threadIdx.x & 63) < lat_nf4)
                __builtin_amdgcn_global_load_lds((gptr_t)(s.coefp + (size_t)(w0 + (threadIdx.x & 63)) * 4), (lptr_t)(lat_coef + (size_t)w0 * 4), 16, 0, 0);
        }
    } else
    if (scalar_prologue) {
        if (wave == 0) {
            const SGPMP_CONST float* sp = as_const(a.spheres);
            for (int o = 0; o < a.n_spheres; ++o) {              // wave-uniform values; lane 0 writes the row
                const float cx = sp[o * 4 + 0], cy = sp[o * 4 + 1], cz = sp[o * 4 + 2], r = sp[o * 4 + 3];
                if (lane == 0) sphere_row(o, cx, cy, cz, r);
            }
            for (int r = 0; r <= ng_; ++r) {                     // start state (row 0) and goal states: lane e keeps element e
                const SGPMP_CONST float* src = r == 0 ? as_const((const float*)F.gp.dev_data)
                                                      : as_const((const float*)F.goal.dev_data) + (size_t)(r - 1) * D;
                float mine = 0.f;
                if (r > 0 || gp_start_) {
#pragma unroll
                    for (int e = 0; e < D; ++e) {
                        const float v = src[e];
                        mine = lane == e ? v : mine;
                    }
                }
                if (lane < 16) unl[r * 16 + lane] = mine;
            }
        }
    } else {
        for (int o = threadIdx.x; o < a.n_spheres; o += 64 * WPB)
            sphere_row(o, a.spheres[o * 4 + 0], a.spheres[o * 4 + 1], a.spheres[o * 4 + 2], a.spheres[o * 4 + 3]);
        for (int o = threadIdx.x; o < (ng_ + 1) * 16; o += 64 * WPB) {
            const int r = o >> 4, e = o & 15;
            float v = 0.f;
            if (e < D) {
                if (r == 0) v = gp_start_ ? ((const float*)F.gp.dev_data)[e] : 0.f;
                else v = ((const float*)F.goal.dev_data)[(size_t)(r - 1) * D + e];
            }
            unl[o] = v;
        }
    }
    PSTAMP(0);
    if (s.zero_stats && blockIdx.x == 0)                                  // (strided: a launch may bring fewer than 256 threads)
        for (int zi = threadIdx.x; zi < SGPMP_STAT_SHARDS * 4; zi += 64 * WPB) s.zero_stats[zi] = 0.;   // (64 WPB = blockDim.x, which is a vector load from the dispatch packet)
    auto lat_commit_tables = [&]() {                                      // LAT, first item: registers -> LDS (a barrier follows)
        const int o = threadIdx.x;
        if (o < a.n_spheres) sphere_row(o, lat_sph.x, lat_sph.y, lat_sph.z, lat_sph.w);
        if (o < (ng_ + 1) * 16) unl[o] = lat_un;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // the coefficient table's LDS-DMA has landed
    };
    if constexpr (!LAT) __syncthreads();
    PSTAMP(1);
    auto static_sphere_sum = [&]() {
    float sph_static = 0.f;
    if (prog_has<FULL>(F.has_sph)) {
        float q0[N], P0[CC::NREP][3];
#pragma unroll
        for (int k = 0; k < N; ++k) q0[k] = 0;
        fk_cg<float, CC>(q0, P0);
        if (FT == SGPMP_FIELD_RBF) {
            float v = 0.f;
            for (int o = lane; o < a.n_spheres; o += 64) {
                const float* sp = sphl + (size_t)o * 8;
#pragma unroll
                for (int l = 0; l < CC::NREP; ++l) {
                    if (!CC::is_static(l)) continue;
                    const float pp = sq3(P0[l][0], P0[l][1], P0[l][2]);
                    v += CC::mult(l) * __builtin_amdgcn_exp2f(pp * sp[3] + (P0[l][0] * sp[0] + (P0[l][1] * sp[1] + (P0[l][2] * sp[2] + sp[4]))));
                }
            }
            sph_static = (float)wave_sum_dpp((double)v);
        } else {
            float v = FT == SGPMP_FIELD_SDF ? -__builtin_inff() : 0.f;
            for (int o = 0; o < a.n_spheres; ++o) {
                const float* sp = sphl + (size_t)o * 8;
#pragma unroll
                for (int l = 0; l < CC::NREP; ++l) {
                    if (!CC::is_static(l)) continue;
                    const float dx = P0[l][0] - sp[0], dy = P0[l][1] - sp[1], dz = P0[l][2] - sp[2];
                    const float dist = __builtin_amdgcn_sqrtf(sq3(dx, dy, dz));
                    if (FT == SGPMP_FIELD_SDF) {
                        float sd = sp[3] - dist;
                        if (F.sph.flags & SGPMP_FLAG_SDF_CLAMP) sd = fminf(sd, 0.f);
                        v = fmaxf(v, sd);
                    } else {
                        v += dist < sp[3] ? CC::mult(l) : 0.f;
                    }
                }
            }
            sph_static = v;
        }
    }

    if (lane == 0) sphst[wave] = sph_static;
#ifdef FUSED_STAMPS
    asm volatile("" : "+v"(sph_static));
#endif
    };
    if constexpr (!LAT) static_sphere_sum();
    PSTAMP(2);
    // Lane roles are RE-DERIVED from the lane number inside every phase (the asm makes the lane number
    // opaque there): a handful of integer instructions per phase, instead of a dozen per-lane values that
    // would live through all phases -- the register allocator parks such long-lived values in scratch, and
    // a scratch reload is a vector-memory load that waits behind the chunk's stores.
    // SGPMP_FUSED_FRESH_LANE=1: every phase re-derives its lane indices and addresses from an opaque copy of the lane id, so that
    // nothing of them stays live over the item (rounds 2-3, and what a 96-register budget needs: -DSGPMP_FUSED_WAVES_RS=5).  0, the
    // default since round 4: the compiler keeps them -- 123 registers instead of 96, four waves per SIMD instead of five, 57 fewer
    // vector instructions per chunk; five waves had measured level with four, this is +1.2 % (4 + 4 alternating runs).
#ifndef SGPMP_FUSED_FRESH_LANE
#define SGPMP_FUSED_FRESH_LANE 0
#endif
    auto fresh_lane = [&]() { int l = lane; if (SGPMP_FUSED_FRESH_LANE) asm volatile("" : "+v"(l)); return l; };
    const bool gp_start = prog_has<FULL>(F.has_gp) && (FULL || (F.gp.flags & SGPMP_FLAG_GP_START));
    const size_t M = (size_t)T * D;

    const long long nitems = SWEEP ? a.batch / SPW : s.nitems;
    const long long istride = (long long)gridDim.x * WPB;
    // Workgroups go to the 8 XCDs round-robin by blockIdx; the workgroups of one particle share its chunk loads (means,
    // importance-sampling weights), so logical workgroup ids are dealt such that neighbours sit on ONE XCD and hit
    // its L2 (gridDim a multiple of 8; otherwise the identity).
    const unsigned lb = SGPMP_FUSED_XCD_MAP && (gridDim.x & 7u) == 0 ? (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3)
                                                                      : blockIdx.x;
#if defined(SGPMP_FUSED_STAGGER) && SGPMP_FUSED_STAGGER > 0
    // EXPERIMENT (round 4, verdict item 1b): the waves that share a SIMD start SGPMP_FUSED_STAGGER x 64 cycles apart
    // (by hardware wave slot), so that co-resident waves sit in different phases of the chunk
    if (!SWEEP) {
        unsigned hw_;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_));
        for (unsigned k_ = hw_ & 3u; k_ > 0; --k_) __builtin_amdgcn_s_sleep(SGPMP_FUSED_STAGGER);
    }
#endif
    bool lat_first = LAT;
    for (long long item = LAT ? (long long)lb : (long long)lb * WPB + wave; item < nitems; item += LAT ? (long long)gridDim.x : istride) {
        const unsigned p = SWEEP ? (a.rpp_shift >= 0 ? (unsigned)(item * SPW) >> a.rpp_shift : (unsigned)(item * SPW) / (unsigned)a.rows_per_particle)
                                 : (s.gpp_shift >= 0 ? (unsigned)item >> s.gpp_shift : (unsigned)item / (unsigned)s.gpp);
        const unsigned g = SWEEP ? 0u : (unsigned)item - p * (unsigned)s.gpp;
        // first (local) row of the item, and how many of its 8 rows exist: a particle's last group is short when S % 8 != 0
        // (round 4: such S ran the two-launch path at 1.5 x the time) -- its missing rows are computed like the others and
        // never written (samples, costs) nor counted (softmax partials)
        const long long b0 = !RAG ? item * SPW : (long long)p * s.S + (long long)g * SPW;
        const int nv = !RAG ? SPW : (s.S - (int)g * SPW < SPW ? s.S - (int)g * SPW : SPW);
        const unsigned grow = (unsigned)(a.batch_offset + b0);
        const unsigned gidx = !prog_has<FULL>(F.has_goal) ? 0u : a.rpg_shift >= 0 ? grow >> a.rpg_shift : grow / (unsigned)F.goal.rows_per_goal;
        const float* const mu = SWEEP ? a.trajs : s.means + (size_t)p * M;
        const bool use_is = !SWEEP || a.isw != nullptr;
        const float* const isw = use_is ? a.isw + (size_t)p * (T + 1) * D : a.trajs;
        // (wave-uniform; the scalar load is issued here, a whole noise phase ahead of its first use)
        const bool store_rows = SWEEP || FULL || !s.nostore || (s.nnz_prev != nullptr && as_const(s.nnz_prev)[p] > s.store_threshold);
        float yp = 0.f, yv = 0.f;                        // recurrence state (perturbation of position / velocity)
        f2 run = f2{0.f, 0.f};
        FSTAMP_DECL;
#ifdef FUSED_STAMPS
        st_0 = FSTAMP_NOW();
#endif
        // the waypoint "before t = 0" is zero
        {
            const int l_ = fresh_lane();
            if (l_ < SPW * (HEAD / 2)) {
                const int r_ = l_ / (HEAD / 2), e_ = l_ - r_ * (HEAD / 2);
                // (materialised here: hoisted out of the item loop as a kernel-long constant pair, the masked instantiation
                // SPILLED it to scratch and reloaded it per item)
                real2 zero2 = real2{0.f, 0.f};
                asm volatile("" : "+v"(zero2));
                *reinterpret_cast<real2*>(tile + r_ * PITCH + 2 * e_) = zero2;
            }
        }

        // ---- a chunk's global loads go straight to LDS (LDS-DMA: no VGPRs held, one instruction per 16 d
        // contiguous floats): the means and importance-sampling weights of the particle, and -- sweep only --
        // the chunk of every row of the item, verbatim
        // RS: straight into registers instead -- what THIS lane needs of them: phase B's seven 16-byte columns of the means
        // (8 lanes per row, every row the same 224 floats: L1 hits) and phase C's 14 weights of this lane's waypoint -- issued at
        // the top of the chunk, in flight under the noise phase (42 registers that phase has to spare; the old staging cost
        // 1.8 KB of LDS per wave, which is what kept a fifth wave off every SIMD: occupancy 3 -> 4 is worth 19 % on this launch).
        real4 mu_r[V4L];
        real2 w_r[N];
        auto issue_chunk_loads = [&](int tn) {
            const int l_ = fresh_lane();
            if constexpr (RS) {
                // (scalar base + 32-bit lane offset: the wave-uniform part of the address is scalar arithmetic)
                const float* pm = mu + (size_t)tn * D;
                const float* pw = isw + (size_t)tn * D;
                if constexpr (!RAG) {
                    const unsigned om = (unsigned)(l_ & 7) * 16u, ow = (unsigned)(l_ & 15) * (unsigned)(D * 4);
#pragma unroll
                    for (int j = 0; j < V4L; ++j)
                        asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(mu_r[j]) : "v"(om), "s"(pm), "i"(128 * j) : "memory");
#pragma unroll
                    for (int i = 0; i < N; ++i)
                        asm volatile("global_load_dwordx2 %0, %1, %2 offset:%3" : "=v"(w_r[i]) : "v"(ow), "s"(pw), "i"(8 * i) : "memory");
                } else {
                    // RAG, the LAST chunk of a T that is not a multiple of 16: columns / waypoints past T read the chunk's first
                    // column / the row of waypoint T (it exists: the weights have T + 1 rows) -- finite numbers that the masked
                    // stores and the masked cost lanes below never use.  (One form for every chunk of this instantiation: two
                    // alternative groups of hand-placed loads into the same registers are what tools/audit_asm_loads.py cannot
                    // tell apart from a use before the wait.)
                    const unsigned tleft = (unsigned)(T - tn) < (unsigned)TC ? (unsigned)(T - tn) : (unsigned)TC;
                    const unsigned nvf = tleft * (unsigned)D;
                    const unsigned trow = (unsigned)(l_ & 15) < tleft ? (unsigned)(l_ & 15) : tleft;
                    const unsigned ow = trow * (unsigned)(D * 4);
#pragma unroll
                    for (int j = 0; j < V4L; ++j) {
                        const unsigned cf = (unsigned)(l_ & 7) * 4u + 32u * j;
                        const unsigned oj = cf < nvf ? cf * 4u : 0u;
                        asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(mu_r[j]) : "v"(oj), "s"(pm) : "memory");
                    }
#pragma unroll
                    for (int i = 0; i < N; ++i)
                        asm volatile("global_load_dwordx2 %0, %1, %2 offset:%3" : "=v"(w_r[i]) : "v"(ow), "s"(pw), "i"(8 * i) : "memory");
                }
                return;
            }
            if (l_ < V4) {
                if (!SWEEP)
                    __builtin_amdgcn_global_load_lds((gptr_t)(mu + (size_t)tn * D + l_ * 4), (lptr_t)mul, 16, 0, 0);
                if (use_is)
                    __builtin_amdgcn_global_load_lds((gptr_t)(isw + (size_t)tn * D + l_ * 4), (lptr_t)wl, 16, 0, 0);
                if (SWEEP) {
#pragma unroll
                    for (int r = 0; r < SPW; ++r)
                        __builtin_amdgcn_global_load_lds((gptr_t)(a.trajs + ((size_t)(b0 + r) * T + tn) * D + l_ * 4),
                                                         (lptr_t)(tile + r * PITCH + HEAD), 16, 0, SGPMP_SWEEP_LOAD_AUX);
                }
            }
        };
        if (SWEEP) issue_chunk_loads(0);

        // The noise of a chunk on ALL 64 lanes -- lane = (sample, waypoint PAIR), one Philox block per dof: the dof wave-uniform
        // (its counter bits are a literal, the tile slots of the four normals immediate offsets of ONE per-lane address) -- left
        // as raw normals in the tile slots the recurrence overwrites; and the recurrence over them, lane = (sample, dof), which
        // reads eps_t from where it writes y_t.  Same counters, same expressions as phase_A below: the same samples, bit for bit
        // (the small-step schedule, LAT, runs the two on different waves' time; SGPMP_FUSED_NOISE_ALL_LANES=1 back to back).
        auto phase_A1 = [&](int tn) {
            static_assert(SPW * (TC / 2) == 64, "one lane per (sample, waypoint pair)");
            const int l1 = fresh_lane();
            const int s1 = l1 >> 3, tp = l1 & 7;
            NoiseGen<float> gen;
            gen.init(s.seed, s.draw, (uint32_t)(s.mode_offset + (int)p), (uint32_t)(g * SPW + s1), 0u);
            float* o1 = tile + s1 * PITCH + HEAD + tp * 2 * D;
#pragma unroll
            for (int k = 0; k < N; ++k) {
                sg_f2 z02, z13;
                gen.kk = (uint32_t)k << 20;
                gen.get4p(tn + 2 * tp, z02, z13);
                o1[k] = z02.x; o1[N + k] = z13.x; o1[D + k] = z02.y; o1[D + N + k] = z13.y;
            }
        };
        auto phase_A2 = [&](int tn, float& sp, float& sv) {
            const int la = fresh_lane();
            if (la < SPW * N) {
                const int sa = (int)(((unsigned)la * (65536u / N + 1)) >> 16), ka = la - sa * N;   // sample within the item, dof
                float* o = tile + sa * PITCH + HEAD + ka;
                sg_f2 pv = {sp, sv};
                auto steps = [&](auto c) {
#pragma unroll
                    for (int tt = 0; tt < TC; tt += 2, c += 16, o += 2 * D) {
                        const float e0 = o[0], e1 = o[N], e2 = o[D], e3 = o[D + N];
                        scan_step2(c, e0, e1, pv);
                        o[0] = pv.x; o[N] = pv.y;
                        scan_step2(c + 8, e2, e3, pv);
                        o[D] = pv.x; o[D + N] = pv.y;
                    }
                };
                steps(as_const(s.coefp + (size_t)tn * 8));                                 // wave-uniform: scalar loads
                sp = pv.x; sv = pv.y;
            }
        };
        // ... the recurrence of the small-step schedule (LAT), in the two halves of rng.h scan_step2: everything that does not
        // depend on the state -- the chunk's normals and coefficients out of LDS, the noise terms -- BEFORE the state arrives from
        // the wave that has the previous chunk; then two dependent packed fmas per waypoint.  (As one loop the recurrence waited
        // for an LDS round trip per waypoint: 2 k cycles per chunk, the four chunks one after the other.)
        // (tq, h1q, h2q: 96 registers that live from the noise terms to the hand-over and no longer -- declared inside the trip of
        // the chunk loop that uses them, or the allocator keeps them through the cost phase and the kernel does not fit two per SIMD)
        auto phase_A2_noise = [&](int tn, sg_f2 (&tq)[TC], sg_f2 (&h1q)[TC], sg_f2 (&h2q)[TC]) {
            const int la = fresh_lane();
            if (la < SPW * N) {
                const int sa = (int)(((unsigned)la * (65536u / N + 1)) >> 16), ka = la - sa * N;
                const float* o = tile + sa * PITCH + HEAD + ka;
                const float* c = lat_coef + (size_t)tn * 8;
#pragma unroll
                for (int tt = 0; tt < TC; ++tt) {
                    tq[tt] = scan_step2_noise(c + 8 * tt, o[tt * D], o[tt * D + N]);
                    h1q[tt] = sg_f2{c[8 * tt + 2], c[8 * tt + 3]};
                    h2q[tt] = sg_f2{c[8 * tt + 4], c[8 * tt + 5]};
                }
            }
        };
        // (the chunk's y stay in registers -- tq's -- until the state has been handed on: phase_A2_rows writes them to the tile)
        auto phase_A2_state = [&](float& sp, float& sv, sg_f2 (&tq)[TC], const sg_f2 (&h1q)[TC], const sg_f2 (&h2q)[TC]) {
            sg_f2 pv = {sp, sv};
#pragma unroll
            for (int tt = 0; tt < TC; ++tt) {
                scan_step2_state(h1q[tt], h2q[tt], tq[tt], pv);
                tq[tt] = pv;
            }
            sp = pv.x; sv = pv.y;
        };
        auto phase_A2_rows = [&](const sg_f2 (&tq)[TC]) {
            const int la = fresh_lane();
            if (la < SPW * N) {
                const int sa = (int)(((unsigned)la * (65536u / N + 1)) >> 16), ka = la - sa * N;
                float* o = tile + sa * PITCH + HEAD + ka;
#pragma unroll
                for (int tt = 0; tt < TC; ++tt) { o[tt * D] = tq[tt].x; o[tt * D + N] = tq[tt].y; }
            }
        };
        // phase A / phase B of chunk tn as callable pieces: A(c) B(c) C(c) per chunk
        auto phase_A = [&](int tn) {
#if SGPMP_FUSED_PRIO == 1
            __builtin_amdgcn_s_setprio(0);
#elif SGPMP_FUSED_PRIO == 2
            __builtin_amdgcn_s_setprio(1);
#endif
            // ---- phase A: noise + recurrence (same expressions as sample_iso_kernel)
            // (56 of 64 lanes work here.  Spreading the chunk's 448 Philox blocks over all 64 lanes -- 7 calls per lane
            // instead of 8, raw normals through the tile, recurrence as a second pass -- was built twice.  Round 2, flat
            // index: 7 x 80 + 8 x 20 VALU instructions per chunk against 8 x 74, more, not kept.  Round 3, lane =
            // (sample, waypoint pair) with the dof wave-uniform (no per-call addressing at all; the variant below,
            // SGPMP_FUSED_NOISE_ALL_LANES=1): ~58 VALU instructions fewer per chunk, bit-identical samples, launch
            // 195.2 -> 193.4 us event-timed but 5044 -> 4926 it/s inside optimize(opt_iters=K) on the same box
            // (profiles/r03/ab_noise_all_lanes.txt): the recurrence alone is a bare dependency chain with nothing of its
            // own wave to overlap, and two LDS round trips per normal are added.  Off.  Round 4, with the two-wide recurrence and
            // Box-Muller in both forms: 5295 against 5521 it/s (four alternating runs): off for good.)
#ifndef SGPMP_FUSED_NO_A
#if SGPMP_FUSED_NOISE_ALL_LANES
            if (!SWEEP) {
                phase_A1(tn);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                phase_A2(tn, yp, yv);
            }
#else
            const int la_ = fresh_lane();
            const int la = la_;
            if (!SWEEP && la < SPW * N) {
                const int sa = (int)(((unsigned)la * (65536u / N + 1)) >> 16), ka = la - sa * N;   // sample within the item, dof
                NoiseGen<float> gen;
                gen.init(s.seed, s.draw, (uint32_t)(s.mode_offset + (int)p), (uint32_t)(g * SPW + sa), (uint32_t)ka);
                const SGPMP_CONST float* c = as_const(s.coefp + (size_t)tn * 8);   // wave-uniform: scalar loads
                float* o = tile + sa * PITCH + HEAD + ka;
                sg_f2 pv = {yp, yv};
#ifdef SGPMP_FUSED_FAKE_COEF   // what-if diagnostic (wrong numbers): one set of scan coefficients for every waypoint -> no loads inside the loop
#define SGPMP_COEF_STEP 0
#else
#define SGPMP_COEF_STEP 16
#endif
#pragma unroll SGPMP_FUSED_A_UNROLL
                for (int tt = 0; tt < TC; tt += 2, c += SGPMP_COEF_STEP, o += 2 * D) {
                    // (rng.h: the canonical evaluation order of the recurrence, two-wide -- same bits as sample_iso_kernel's scan_step)
                    sg_f2 z02, z13;
#if SGPMP_FUSED_COEF_X16
                    {
                        // the block's two coefficient rows as ONE scalar load issued ahead of the Philox rounds (left to the compiler
                        // the six loads sit behind the Box-Muller code, a dozen instructions ahead of their use)
                        sg_f16 cc;
                        int tq = tn + tt;                                 // (tied to the load: the Philox rounds cannot be scheduled above it)
                        asm volatile("s_load_dwordx16 %0, %2, 0x0" : "=s"(cc), "+s"(tq) : "s"(c));
                        gen.get4p(tq, z02, z13);
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                        asm volatile("" : "+s"(cc));
                        scan_step2v<0>(cc, z02.x, z13.x, pv);
                        o[0] = pv.x; o[N] = pv.y;
                        scan_step2v<8>(cc, z02.y, z13.y, pv);
                        o[D] = pv.x; o[D + N] = pv.y;
                        continue;
                    }
#endif
                    gen.get4p(tn + tt, z02, z13);
                    scan_step2(c, z02.x, z13.x, pv);
                    o[0] = pv.x; o[N] = pv.y;
                    scan_step2(c + 8, z02.y, z13.y, pv);
                    o[D] = pv.x; o[D + N] = pv.y;
                }
                yp = pv.x; yv = pv.y;
            }
#endif
#endif
        };
        auto phase_B = [&](int tn) {
            // ---- phase B: x = mu + y -> HBM (write-only) and back into the tile
            if (!SWEEP) {
                const int lb = fresh_lane();
                const int rb = lb >> 3, qb = lb & 7;                     // tile row, first 16-byte column
                float* const rowb = tile + rb * PITCH + HEAD + qb * 4;
                const float* const outs = s.samples + (size_t)b0 * M + (size_t)tn * D;      // wave-uniform: scalar base
                const unsigned outv = ((unsigned)rb * (unsigned)M + (unsigned)qb * 4u) * 4u;     // + this lane's byte offset (8 rows: 32 bits)
                auto rows_out = [&](auto masked, auto stored) {
                    // masked: a row past S (the particle's last group of 8) is not written -- its tile row keeps y, finite and
                    // unused; nor are the columns past T of the last chunk
                    if (decltype(masked)::value && rb >= nv) return;
                    const int nvf = (T - tn) * D;
#pragma unroll
                    for (int j = 0; j < V4L; ++j) {
                        real4 val = *reinterpret_cast<const real4*>(rowb + 32 * j);
                        if constexpr (RS) val += mu_r[j];
                        else val += *reinterpret_cast<const real4*>(mul + qb * 4 + 32 * j);
                        // write-through + non-temporal (sc1 nt): nothing re-reads the line from this L2 (update_kernel may run on another
                        // XCD); round 6, same box, interleaved: sc1 5539, nt 5573, sc1 nt 5607 it/s, no bits 5441 (profiles/r06/store_policy_ab.txt)
                        if (decltype(stored)::value && (!decltype(masked)::value || qb * 4 + 32 * j < nvf))
                            asm volatile("global_store_dwordx4 %0, %1, %2 offset:%3 " SGPMP_FUSED_STORE_BITS :: "v"(outv), "v"(val), "s"(outs), "i"(128 * j) : "memory");
                        *reinterpret_cast<real4*>(rowb + 32 * j) = val;
                    }
                };
                // (all wave-uniform; a store-free step's particle: x = mu + y goes back into the tile only)
                if (!store_rows) rows_out(BoolC<false>{}, BoolC<false>{});
                else if (!RAG || (nv == SPW && tn + TC <= T)) rows_out(BoolC<false>{}, BoolC<true>{});
                else rows_out(BoolC<true>{}, BoolC<true>{});
            }
        };
        auto tile_fence = [&]() {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");       // the tile is wave-private
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        };
        auto phase_C = [&](int t0) {
            FSTAMP(1);
#if SGPMP_FUSED_PRIO == 1
            __builtin_amdgcn_s_setprio(1);
#elif SGPMP_FUSED_PRIO == 2
            __builtin_amdgcn_s_setprio(0);
#endif
            // ---- phase C: cost terms of waypoint t of rows 2 jc, 2 jc + 1
            const int lc = fresh_lane();
            const int jc = lc >> 4, tc = lc & 15;                        // pair of rows, waypoint within the chunk
            const float* const rowc = tile + (2 * jc) * PITCH + HEAD + tc * D;
            const float sph_static = sphst[wave];
            const int t = t0 + tc;
            // (the last chunk of a T that is not a multiple of 16: the lanes of waypoints past T add nothing but their unary share)
            const bool inner = t >= 1 && (!RAG || t < T);
            // element i of rows 2 jc and 2 jc + 1 in ONE ds_read2_b32 (the rows lie PITCH dwords apart, inside
            // the instruction's 8-bit offset range): the packed pair forms in adjacent registers, no moves
            f2 x[D], xp[D];
            float w[D];
            {
                const unsigned ax = (unsigned)(unsigned long)(lptr_t)(void*)const_cast<float*>(rowc);
                const unsigned axp = ax - 4u * D;
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    asm volatile("ds_read2_b32 %0, %1 offset0:%2 offset1:%3" : "=v"(xp[i]) : "v"(axp), "i"(i), "i"(PITCH + i));
                    asm volatile("ds_read2_b32 %0, %1 offset0:%2 offset1:%3" : "=v"(x[i]) : "v"(ax), "i"(i), "i"(PITCH + i));
                }
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    if constexpr (RS) w[i] = (i & 1) ? w_r[i >> 1].y : w_r[i >> 1].x;
                    else w[i] = use_is ? wl[tc * D + i] : 0.f;
                }
                // one wait, then every pair passes through an empty asm: volatile asm statements keep their order, so no
                // use of x / xp can be scheduled ahead of the wait (the compiler does not know the ds_read2 above are loads)
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                for (int i = 0; i < D; ++i) asm volatile("" : "+v"(x[i]), "+v"(xp[i]));
            }
            f2 tot = f2{0.f, 0.f};
            // unary factors: lane tc < D of every row pair owns state element tc of the FIRST waypoint
            // (start prior, first chunk) / the LAST one (goal prior, last chunk) -- whatever waypoint the lane has otherwise
            if (t0 == 0 && gp_start) {
                if (tc < D) {
                    const float* r0 = tile + (2 * jc) * PITCH + HEAD + tc;
                    const f2 ds = f2{r0[0], r0[PITCH]} - unl[tc];
                    tot += ds * ds * F.gp.K2;
                }
            }
            if (t0 + TC >= T && prog_has<FULL>(F.has_goal)) {
                if (tc < D) {
                    const float* r0 = tile + (2 * jc) * PITCH + HEAD + (T - 1 - t0) * D + tc;
                    const f2 dg = f2{r0[0], r0[PITCH]} - unl[(gidx + 1) * 16 + tc];
                    tot += dg * dg * F.goal.K;
                }
            }
            // ---- the chunk now sits in registers (x, x_prev, w; the unary factors have read what they need):
            // its last waypoint becomes the next chunk's "previous" one, and -- sweep -- the tile is refilled at
            // once, so the next chunk's rows land while this one is being computed
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            {
                const int ld = fresh_lane();
                const int rb = ld >> 3, qb = ld & 7;
                if (qb < D / 2) {
                    float* r_ = tile + rb * PITCH + HEAD;
                    const real2 v = *reinterpret_cast<const real2*>(r_ + (TC - 1) * D + 2 * qb);
                    *reinterpret_cast<real2*>(r_ - D + 2 * qb) = v;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (SWEEP && t0 + TC < T) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // the carry copy has read its row
                issue_chunk_loads(t0 + TC);
            }
            {
                // GP factors (gp_factor.py:54-67) and the importance-sampling product (planner.py:233-236)
                // on e_t = x_t - Phi x_{t-1}; for t = 0, x_{-1} = 0 makes e_0 = x_0, the first block of A x
                const float dtg = prog_has<FULL>(F.has_gp) ? F.gp.dt : a.is_dt;
                f2 pp = f2{0.f, 0.f}, pv = pp, vv = pp, dis = pp;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const f2 ep = x[k] - (xp[k] + xp[N + k] * dtg);
                    const f2 ev = x[N + k] - xp[N + k];
                    pp += ep * ep; pv += ep * ev; vv += ev * ev;
                    dis += ep * w[k] + ev * w[N + k];
                }
                if (prog_has<FULL>(F.has_gp) && inner)
                    tot += (pp * F.gp.c11 + pv * (2.f * F.gp.c12) + vv * F.gp.c22) * F.gp.K;
                if (!RAG || t0 + TC <= T) tot += dis;                    // (wave-uniform)
                else tot += f2{t < T ? dis.x : 0.f, t < T ? dis.y : 0.f};
            }
            f2 q[N];
#pragma unroll
            for (int k = 0; k < N; ++k) q[k] = x[k];
            // everything above consumed the 70 registers of (x, x_prev, w); only q survives into the
            // kinematics below -- keep the compiler from sinking the quadratic forms below the kinematics
            // (the asm pins `tot` here) and the scheduler from interleaving the two halves
            asm volatile("" : "+v"(tot));
            __builtin_amdgcn_sched_barrier(0);
            FSTAMP(2);
            f2 part = f2{0.f, 0.f};
#ifndef SGPMP_FUSED_NO_FK
            if (prog_has<FULL>(F.has_self) || prog_has<FULL>(F.has_sph)) {
                f2 Pq[CC::NREP][3];
                CC::template fk_snapped<f2, O>(q, Pq);
                if (prog_has<FULL>(F.has_self)) {
                    const float kk = F.self.K2 * (float)SGPMP_LOG2E;
                    f2 f = f2{F.self.selfc, F.self.selfc};
#pragma unroll
                    for (int pr = 0; pr < CC::NPAIR; ++pr) {
                        const int i = CC::pair_i(pr), j = CC::pair_j(pr);
                        const f2 dx = Pq[i][0] - Pq[j][0], dy = Pq[i][1] - Pq[j][1], dz = Pq[i][2] - Pq[j][2];
                        f += O::exp2_((sq3(dx, dy, dz)) * kk) * CC::pair_w(pr);
                    }
                    if (inner) part += f * F.self.K;
                }
                if (prog_has<FULL>(F.has_sph) && FT != SGPMP_FIELD_RBF) {
                    const bool clamp = (F.sph.flags & SGPMP_FLAG_SDF_CLAMP) != 0;
                    f2 f = f2{sph_static, sph_static};
                    for (int o = 0; o < a.n_spheres; ++o) {
                        const float* sp = sphl + (size_t)o * 8;
                        const float cx = sp[0], cy = sp[1], cz = sp[2], rr = sp[3];
                        if (FT == SGPMP_FIELD_SDF) {
                            // max_l (r - dist_l) = r - sqrt(min_l dist_l^2): v_sqrt_f32 and the subtraction are
                            // monotone, so ONE square root per sphere gives the same bits as one per link
                            f2 m2 = f2{__builtin_inff(), __builtin_inff()};
#pragma unroll
                            for (int l = 0; l < CC::NREP; ++l) {
                                if (CC::is_static(l)) continue;
                                const f2 dx = Pq[l][0] - cx, dy = Pq[l][1] - cy, dz = Pq[l][2] - cz;
                                const f2 d2 = sq3(dx, dy, dz);
                                m2 = f2{fminf(m2.x, d2.x), fminf(m2.y, d2.y)};
                            }
                            f2 sd = rr - f2{__builtin_amdgcn_sqrtf(m2.x), __builtin_amdgcn_sqrtf(m2.y)};
                            if (clamp) sd = f2{fminf(sd.x, 0.f), fminf(sd.y, 0.f)};
                            f = f2{fmaxf(f.x, sd.x), fmaxf(f.y, sd.y)};
                            continue;
                        }
#pragma unroll
                        for (int l = 0; l < CC::NREP; ++l) {
                            if (CC::is_static(l)) continue;
                            const f2 dx = Pq[l][0] - cx, dy = Pq[l][1] - cy, dz = Pq[l][2] - cz;
                            const f2 d2 = sq3(dx, dy, dz);
                            // occupancy count (fields.py:85-86): dist < r  <=>  dist^2 < r^2 up to the rounding
                            // of the square root; kept on the distances themselves, as the oracle compares them
                            const f2 dist = f2{__builtin_amdgcn_sqrtf(d2.x), __builtin_amdgcn_sqrtf(d2.y)};
                            f += f2{dist.x < rr ? CC::mult(l) : 0.f, dist.y < rr ? CC::mult(l) : 0.f};
                        }
                    }
                    if (inner) part += f * F.sph.K;
                }
                if (prog_has<FULL>(F.has_sph) && FT == SGPMP_FIELD_RBF) {
                    f2 pp[CC::NREP];
#pragma unroll
                    for (int l = 0; l < CC::NREP; ++l)
                        pp[l] = CC::is_static(l) ? f2{0.f, 0.f}
                                                 : sq3(Pq[l][0], Pq[l][1], Pq[l][2]);
                    f2 f = f2{sph_static, sph_static};
                    // (Tried: reading the next sphere's constants one iteration ahead.  Hidden in inline asm with a
                    // counted lgkmcnt it is 1.2 % faster but hipcc copies the destination registers before the
                    // data has landed -- wrong, non-deterministic costs; with visible loads + sched_barrier the
                    // waitcnt pass waits for lgkmcnt(0) across the back edge anyway and the barriers cost 3 %.)
                    float ax = sphl[0], ay = sphl[1], az = sphl[2], k = sphl[3], bb = sphl[4];
                    for (int o = 0; o < a.n_spheres; ++o) {
                        const float* nx = sphl + (size_t)(o + 1 < a.n_spheres ? o + 1 : o) * 8;
                        const float nax = nx[0], nay = nx[1], naz = nx[2], nk = nx[3], nb = nx[4];
#pragma unroll
                        for (int l = 0; l < CC::NREP; ++l) {
                            if (CC::is_static(l)) continue;
                            const f2 arg = pp[l] * k + (Pq[l][0] * ax + (Pq[l][1] * ay + (Pq[l][2] * az + bb)));
                            f += O::exp2_(arg) * CC::mult(l);
                        }
                        ax = nax; ay = nay; az = naz; k = nk; bb = nb;
                    }
                    if (inner) part += f * F.sph.K;
                }
            }
#endif
            run += tot + part;
#ifdef FUSED_STAMPS
            asm volatile("" : "+v"(run));
#endif
            FSTAMP(3);
        };
        if constexpr (LAT) {
            // ---- the small-step schedule: this workgroup's four waves share the item, wave w has the chunks w, w + 4, ...
            const int nch = (T + TC - 1) / TC;
            for (int c0 = 0; c0 < nch; c0 += WPB) {
                const int c = c0 + wave, t0 = c * TC;
                const bool have = c < nch;                               // (wave-uniform)
                const int la = fresh_lane();                             // lane = (sample, dof) where la < SPW N
                float sp = 0.f, sv = 0.f;                                // the recurrence's state entering the chunk
                sg_f2 tq[TC], h1q[TC], h2q[TC];
                FSTAMP_START();
                if (have) {
                    // the means of waypoint t0 - 1, element (dof) of this lane: global -> LDS by LDS-DMA (no registers held over the
                    // noise phase and the hand-over; read back where the waypoint in front of the chunk is rebuilt)
                    if (c > 0 && la < SPW * N) {
                        const int ka = la - (int)(((unsigned)la * (65536u / N + 1)) >> 16) * N;
                        __builtin_amdgcn_global_load_lds((gptr_t)(mu + (size_t)(t0 - 1) * D + ka), (lptr_t)lat_mu, 4, 0, 0);
                        __builtin_amdgcn_global_load_lds((gptr_t)(mu + (size_t)(t0 - 1) * D + N + ka), (lptr_t)(lat_mu + 64), 4, 0, 0);
                    }
                    issue_chunk_loads(t0);
                    phase_A1(t0);
                    tile_fence();
                }
                if (lat_first) { lat_commit_tables(); __syncthreads(); }    // (workgroup-uniform: the first trip of the first item)
                if (have) phase_A2_noise(t0, tq, h1q, h2q);
                // the recurrence, chunk after chunk: its state goes from wave to wave through LDS
                for (int k = 0; k < WPB; ++k) {
                    if (k == wave && have) {
                        if (c > 0 && la < SPW * N) {
                            sp = lat_carry[(c * SPW * N + la) * 2];
                            sv = lat_carry[(c * SPW * N + la) * 2 + 1];
                        }
                        float ep = sp, ev = sv;
                        if (la < SPW * N) {
                            phase_A2_state(ep, ev, tq, h1q, h2q);
                            lat_carry[((c + 1) * SPW * N + la) * 2] = ep;
                            lat_carry[((c + 1) * SPW * N + la) * 2 + 1] = ev;
                        }
                    }
                    // (the sum over the links that never move: once per wave, in a turn the wave would spend waiting -- wave 0 has
                    // the first turn and takes the second)
                    if (lat_first && k == (wave == 0 ? 1 : 0)) static_sphere_sum();
                    __syncthreads();
                }
                lat_first = false;
                if (have) {
                    phase_A2_rows(tq);
                    FSTAMP(0);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the means / weights have landed
#pragma unroll
                    for (int j = 0; j < V4L; ++j) asm volatile("" : "+v"(mu_r[j]));
#pragma unroll
                    for (int i = 0; i < N; ++i) asm volatile("" : "+v"(w_r[i]));
                    // the waypoint in front of the chunk, x = mu + y with y = the state the recurrence entered with: the add phase B
                    // made of it on the wave that had the previous chunk (zeros in front of t = 0: written at the top of the item)
                    if (c > 0 && la < SPW * N) {
                        const int sa = (int)(((unsigned)la * (65536u / N + 1)) >> 16), ka = la - sa * N;
                        tile[sa * PITCH + HEAD - D + ka] = sp + lat_mu[la];
                        tile[sa * PITCH + HEAD - D + N + ka] = sv + lat_mu[64 + la];
                    }
                    tile_fence();
                    phase_B(t0);
                    tile_fence();
                    run = f2{0.f, 0.f};
                    phase_C(t0);
                    lat_v[c * 64 + lane] = run;
                }
            }
            // wave 0 finishes the item: the chunks' shares added in chunk order (the order of the one-wave loop below), the row sums,
            // the softmax partial (which re-reads the rows all four waves stored)
            if (s.part != nullptr) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (wave != 0) continue;
            run = f2{0.f, 0.f};
            for (int c = 0; c < nch; ++c) run += lat_v[c * 64 + lane];
        } else
        for (int t0 = 0; t0 < T; t0 += TC) {
            // fused: issued at the top of the chunk, ahead of its stores (on gfx9 stores count in vmcnt in
            // order: a load behind a store cannot be waited for without the store's HBM round trip);
            // sweep: issued one chunk ahead, as soon as the previous chunk sat in registers (below)
            FSTAMP_START();
            if (!SWEEP) {
                issue_chunk_loads(t0);
                phase_A(t0);
                tile_fence();
                FSTAMP(0);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // the means / weights have landed
                if constexpr (RS) {                                          // (volatile asm statements keep their order: no use ahead of the wait)
#pragma unroll
                    for (int j = 0; j < V4L; ++j) asm volatile("" : "+v"(mu_r[j]));
#pragma unroll
                    for (int i = 0; i < N; ++i) asm volatile("" : "+v"(w_r[i]));
                }
                phase_B(t0);
                tile_fence();
            } else {
                tile_fence();
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // the staged weights / rows have landed
                tile_fence();
            }
            phase_C(t0);
        }

        // ---- per-trajectory totals: sum of the 16 lanes of each row (DPP row rotations)
        float s0 = run.x, s1 = run.y;
        s0 = dpp_add<0x128, 0xf>(s0); s1 = dpp_add<0x128, 0xf>(s1);
        s0 = dpp_add<0x124, 0xf>(s0); s1 = dpp_add<0x124, 0xf>(s1);
        s0 = dpp_add<0x122, 0xf>(s0); s1 = dpp_add<0x122, 0xf>(s1);
        s0 = dpp_add<0x121, 0xf>(s0); s1 = dpp_add<0x121, 0xf>(s1);
        const int le = fresh_lane();
#ifdef FUSED_STAMPS
        st_[4] = FSTAMP_NOW() - st_entry; st_[5] = st_entry & 0xffffffull;       // whole wave, from kernel entry
        {
            // where the wave ran: HW_ID (gfx9 layout: wave slot 3:0, SIMD 5:4, CU 11:8, SH 12, SE 15:13) and the XCD
            unsigned hw_, xcc_;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_));
            const float v6 = (float)((hw_ & 0xffffu) | ((xcc_ & 0xfu) << 16)), v7 = (float)(st_0 - st_entry);   // placement; prologue cycles
            if (a.costs) {
#if FUSED_STAMPS == 2
                if (le < 3) a.costs[b0 + le] = (float)pro_[le < 1 ? 0 : le < 2 ? 1 : 2];
                else if (le == 3) a.costs[b0 + 3] = 0.f;
                else if (le < 6) a.costs[b0 + le] = (float)st_[le < 5 ? 4 : 5];
#else
                if (le < 6) a.costs[b0 + le] = (float)st_[le < 1 ? 0 : le < 2 ? 1 : le < 3 ? 2 : le < 4 ? 3 : le < 5 ? 4 : 5];
#endif
                else if (le == 6) a.costs[b0 + 6] = v6;
                else if (le == 7) a.costs[b0 + 7] = v7;
            }
        }
        if (false)
#endif
        if ((le & 15) == 0) {
            const int r0 = 2 * (le >> 4);
            const long long b = b0 + r0;
            const bool w0 = r0 < nv, w1 = r0 + 1 < nv;                    // (rows past S do not exist)
            if (a.costs) { if (w0) a.costs[b] = s0; if (w1) a.costs[b + 1] = s1; }
            if (a.costs64) {
                if (SWEEP) { a.costs64[b] = (double)s0; a.costs64[b + 1] = (double)s1; }
                else {                                    // (agent scope: update_kernel may run on another XCD)
                    if (w0) __hip_atomic_store(reinterpret_cast<unsigned long long*>(a.costs64 + b), (unsigned long long)__double_as_longlong((double)s0),
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (w1) __hip_atomic_store(reinterpret_cast<unsigned long long*>(a.costs64 + b + 1), (unsigned long long)__double_as_longlong((double)s1),
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        // ---- dense-weight regime: the softmax partial of this wave's 8 rows (FusedArgs::part).  The rows are read back from
        // memory -- this wave's own write-through stores, waited for -- 16 bytes per lane and row: 32 loads and ~300 vector
        // instructions per item, against the re-read of all S rows by update_kernel.  Taken only for particles whose previous
        // update found the weight spread (a per-particle device-side count, no host round trip): one-hot weights change nothing.
        if (!SWEEP && FULL != 1 && s.part != nullptr) {
            const unsigned prev = as_const(s.nnz_prev)[p];                 // wave-uniform: scalar load
            if (prev > s.nnz_threshold && store_rows) {                    // (store_rows: implied by the host's thresholds; the re-read below needs the rows)
                // the 8 costs of the item to every lane (lanes 0, 16, 32, 48 hold rows 2 j, 2 j + 1)
                float c8[SPW];
#pragma unroll
                for (int j = 0; j < SPW / 2; ++j) {
                    c8[2 * j] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, s0), 16 * j));
                    c8[2 * j + 1] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, s1), 16 * j));
                }
#pragma unroll
                for (int r = 1; r < SPW; ++r) c8[r] = r < nv ? c8[r] : 3.4028234663852886e38f;   // (rows past S: weight exp2(-huge) = 0)
                float cmin = c8[0];
#pragma unroll
                for (int r = 1; r < SPW; ++r) cmin = fminf(cmin, c8[r]);
                float e8[SPW], lsum = 0.f;
                const float k2 = -s.inv_temperature * (float)SGPMP_LOG2E;
#pragma unroll
                for (int r = 0; r < SPW; ++r) { e8[r] = __builtin_amdgcn_exp2f((c8[r] - cmin) * k2); lsum += e8[r]; }
                // (the rows are this wave's own stores: same-wave accesses to one address stay in order, and no first-level
                // cache of this CU can hold an older copy -- nothing reads the sample buffer during the launch)
                // (the lane's first element is re-derived HERE from the lane id and kept 32-bit: as a 64-bit loop-invariant of the
                // whole kernel it was the one value the masked instantiation spilled to scratch -- round-4 verdict, weak #6)
                int lp = (int)(threadIdx.x & 63u);
                asm volatile("" : "+v"(lp));
                float* const po = s.part + ((size_t)p * s.gpp + g) * (M + 4);
                if (lp == 0) *reinterpret_cast<real4*>(po) = real4{cmin, lsum, 0.f, 0.f};
                const float* const xr = s.samples + (size_t)b0 * M;
                for (unsigned m = (unsigned)lp * 4u; m < (unsigned)M; m += 256u) {        // M = T d is a multiple of 32
                    const real4 mu4 = *reinterpret_cast<const real4*>(mu + m);
                    real4 v[SPW];
#pragma unroll
                    for (int r = 0; r < SPW; ++r) v[r] = *reinterpret_cast<const real4*>(xr + (size_t)(r < nv ? r : 0) * M + m);
                    real4 acc = real4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int r = 0; r < SPW; ++r) acc += (v[r] - mu4) * e8[r];
                    *reinterpret_cast<real4*>(po + 4 + m) = acc;
                }
            }
        }
    }
}

template <int N, class CC, int FT, bool RAG = false>
__global__ void __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(SGPMP_FUSED_WAVES_RS, SGPMP_FUSED_WAVES_RS)))
#ifdef SGPMP_FUSED_NUM_VGPR
__attribute__((amdgpu_num_vgpr(SGPMP_FUSED_NUM_VGPR)))
#endif
fused_step_kernel(const CostArgs<float> a, const FlatProg<float> F, const FusedArgs s) {
    chunked_body<N, CC, FT, false, RAG>(a, F, s);
}
// ... with the four-term program compiled in (chunked_body: FULL = 1, 2).  An overload, so that the generic instantiations keep
// their symbols.
template <int N, class CC, int FT, bool RAG, int FULL>
__global__ void __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(SGPMP_FUSED_WAVES_RS, SGPMP_FUSED_WAVES_RS)))
#ifdef SGPMP_FUSED_NUM_VGPR
__attribute__((amdgpu_num_vgpr(SGPMP_FUSED_NUM_VGPR)))
#endif
fused_step_kernel(const CostArgs<float> a, const FlatProg<float> F, const FusedArgs s) {
    static_assert(FULL == 1 || FULL == 2, "the generic kernel is the four-parameter template");
    chunked_body<N, CC, FT, false, RAG, false, FULL>(a, F, s);
}

// the same step for a launch of few items (chunked_body: LAT): one workgroup per item.  The recurrence's halves keep a chunk's
// noise terms and coefficients in 96 registers across the hand-over: 253 in all without the masks -- two waves per SIMD, up to 512
// items in one round of workgroups (the tables that need no arithmetic on the way come in by LDS-DMA for that: with them in
// registers it was 260) -- and 262 with them: one wave per SIMD, up to 256 items (cost_sweep.hip).
// RAG as in fused_step_kernel: a shape on the 8 x 16 grid runs the instantiation without the masks in either launch, so that the
// two stay bit-identical (the masked and the unmasked instantiation differ in the last bit of ~0.1 % of the costs: hipcc pairs
// the cost terms' multiplies and adds differently around the masks' branches).
template <int N, class CC, int FT, bool RAG>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RAG ? 1 : 2, RAG ? 1 : 2)))
fused_step_small_kernel(const CostArgs<float> a, const FlatProg<float> F, const FusedArgs s) {
    chunked_body<N, CC, FT, false, RAG, true>(a, F, s);
}

template <int N, class CC, int FT>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SGPMP_FUSED_WAVES, SGPMP_FUSED_WAVES)))
cost_sweep_chunked_kernel(const CostArgs<float> a, const FlatProg<float> F, const FusedArgs s) {
    chunked_body<N, CC, FT, true>(a, F, s);
}

// dynamic LDS of the fused launch: its sphere / state tables
static inline size_t fused_wave_dyn_lds(int n_spheres, int n_goals) { return (size_t)n_spheres * 32 + (size_t)(n_goals + 1) * 64; }
