// Internal declarations shared by the HIP translation units of libsgpmp.so (gfx950 only).
#pragma once
#ifndef __HIPCC_RTC__                        // (hiprtc brings the runtime header and the fixed-width types itself)
#include <hip/hip_runtime.h>
#include <stdint.h>
#endif
#include "../../include/sgpmp.h"

#define SGPMP_TILE 16                       // state blocks padded to one 16x16 MFMA tile
#define SGPMP_MAX_D (2 * SGPMP_MAX_DOF)
#define SGPMP_MAX_LINKS (SGPMP_MAX_JOINTS + 1)
#define SGPMP_MAX_POINTS 32                 // links + interpolated points per field term
#define SGPMP_WAVE 64

// ---------------------------------------------------------------------------------- prior factor
// Device-resident result of K1 for one prior (INIT or SAMPLE).
struct PriorDev {
    double* blocks;    // [4][d][d]  D0, D, Dlast, E
    double* G;         // [T][d][d]
    double* H;         // [T][d][d]
    double* iso64;     // [T][8]  g11 g21 g22 h11 h12 h21 h22 0   (valid when isotropic)
    float* iso32;      // [T][8]
    float* iso32p;     // [T][8]  g11 g21 | h11 h21 | h12 h22 | g22 0: the same numbers in the pair order of rng.h scan_step2 (fused_step_kernel)
    float* slabpre;    // [5][T][4]  isotropic priors, n = 2, 3: prefix products H_t .. H_{start} of the scan's 2 x 2 propagators from the
                       //            start of t's segment, built by the host in fp64 (table 2: the in-chunk segments of fused_planar.inc;
                       //            tables 3, 4: segments of 8 and of 16 waypoints, fused_planar_seg.inc; 0, 1: unused since round 5)
    double* scan64;    // [T][7][4]  fp64 contexts, isotropic priors: the Kogge-Stone tables of fused_step_f64_kernel (cost_sweep_kernel.inc:
                       //            GenArgs64) -- A_t^(r) = H_t .. H_{t - 2^r + 1}, r = 0 .. 5 (zero where t - 2^r lies before t's pass of 64
                       //            waypoints), and C_t = H_t .. H_{start of the pass}; built by the host in fp64 (api.hip: upload_scan64)
    double* Qinv;      // [d][d]   one-step GP precision of this prior
    float* G32;        // [T][d][d] fp32 copies for the dense sampler
    float* H32;
    int* status;       // 0 ok, 1 not PD / non-finite
    double ks, kg;     // 1/sigma_start^2, 1/sigma_goal^2 (kg < 0: not goal-directed)
    double dt;
    int isotropic;
    int valid;
    // per-mode precisions (MultiMPPrior.set_Sigma_invs): n_factor_modes > 0 -> G/H/G32/H32 are
    // [modes][T][d][d] and Dm/Em hold the given blocks; 0 -> one shared closed-form factor
    int n_factor_modes;
    double* Dm;        // [modes][T][d][d]
    double* Em;        // [modes][T-1][d][d]
};

// ---------------------------------------------------------------------------------- cost program
struct CostTerm {
    int kind;
    int flags;
    double K;             // term weight: GP 1/sigma_gp^2, others 1/sigma^2
    double K2;            // GP: 1/sigma_start^2 ; SELF: -1/(2 margin^2)
    double dt;
    double c11, c12, c22; // GP: 12/dt^3, -6/dt^2, 4/dt
    const void* dev_data; // GP: start [d]; GOAL_PRIOR: goals [G,d]; GRID: grid [dim0,dim1]  (ctx dtype)
    int dim0, dim1;
    long long rows_per_goal;   // GOAL_PRIOR: nppg * S
    double inv_cell, off_x, off_y;
    double selfc;         // SELF: q-independent part of the LxL sum (diagonal, coincident and rigid pairs)
    int n_points;         // links + interpolated points
    int n_interp, interp_lo, interp_hi;
    double alpha[SGPMP_MAX_INTERP];
    double target[16];    // EE_GOAL: target end-effector frame
    double w_pos, w_rot;  // EE_GOAL
    const void* body;     // BODY_SDF: the context's body table (DEVICE: int32 link[SGPMP_MAX_BODY], then [SGPMP_MAX_BODY][4] centre
    int n_body;           // and radius in the ctx dtype) and its sphere count; filled by finalize_program, host use only
};

struct CostProgram {
    int n_terms;
    int needs_fk;         // has link-position fields (SPHERES / SELF) evaluated inside the sweep
    int n_ee;             // EE_GOAL terms (evaluated by ee_goal_kernel after the sweep)
    CostTerm terms[SGPMP_MAX_TERMS];
};

struct JointDev {
    double R[9];          // fixed rotation of the joint origin (RPY)
    double t[3];          // fixed translation
    int revolute;
    int qidx;
};

// Result of the host-side chain analysis (api.hip: analyse_chain).  Link frames that always
// coincide are merged into one representative point with a multiplicity, and link pairs whose
// distance does not depend on q are folded into a constant -- both exact rewrites of the sums in
// fields.py:79,86,124 that the register-resident FK path of the cost sweep exploits.
struct FkPlan {
    int fast;                                   // chain is revolute-first: register path usable
    int codegen_id;                             // 0 none; 1 = ChainCode_panda (chain_code_generated.h); 2 = compiled at run time (ChainDev::rtc)
    int n_rep;                                  // distinct link positions
    float mult[SGPMP_MAX_LINKS];                // multiplicity of link l if representative, else 0
    float wpair[SGPMP_MAX_LINKS * SGPMP_MAX_LINKS];   // [i*ML+j], i>j: 2 m_i m_j if q-dependent, else 0
    int n_cpairs;                               // q-independent representative pairs (host use)
    double cpair_w[SGPMP_MAX_LINKS * SGPMP_MAX_LINKS / 2];
    double cpair_d2[SGPMP_MAX_LINKS * SGPMP_MAX_LINKS / 2];
    double diag;                                // sum_l m_l^2  (i == j and coincident terms)
};

struct ChainDev {
    int n_joints;
    int n_links;          // n_joints + 1
    JointDev j[SGPMP_MAX_JOINTS];
    float Rf[SGPMP_MAX_JOINTS][9];              // fp32 copies of the joint constants
    float tf[SGPMP_MAX_JOINTS][3];
    FkPlan plan;
    void* rtc;                                  // HOST: RtcChain* of this chain's run-time compiled kernels (chain_rtc.hip), or null
};

// ---------------------------------------------------------------------------------- debug toggles
// Development switches (A/B of kernel variants, tests of the fallback paths).  Read from the
// SGPMP_* environment variables ONCE, when a context is created; `sgpmp_set_option` changes them on
// a live context.  Nothing on the launch path calls getenv().
struct SgpmpToggles {
    int force_generic_fk;     // SGPMP_FORCE_GENERIC_FK     link positions through LDS, any chain
    int no_flat_program;      // SGPMP_NO_FLAT_PROGRAM      interpret the term list instead of named fields
    int no_chain_codegen;     // SGPMP_NO_CHAIN_CODEGEN     run-time chain constants instead of generated code
    int no_dual_sweep;        // SGPMP_NO_DUAL_SWEEP        one trajectory per wave
    int k3_no_one;            // SGPMP_K3_NO_ONE            no single-pass specialisation
    int k3_no_lds_prefetch;   // SGPMP_K3_NO_LDS_PREFETCH   register-held prefetch
    int no_small_sampler;     // SGPMP_NO_SMALL_SAMPLER     standard sampler for tiny launches
    int no_fused_step;        // SGPMP_NO_FUSED_STEP        K2 and K3 as separate kernels inside sgpmp_step
    int no_chunked_sweep;     // SGPMP_NO_CHUNKED_SWEEP     64-lane-pass two-trajectory sweeps instead of the chunked one
    int no_step_pipeline;     // SGPMP_NO_STEP_PIPELINE     sgpmp_pipeline_begin .. _end run their steps as one chain
    int gpmp_cholesky;        // SGPMP_GPMP_CHOLESKY        GPMP solve by round 3's block Cholesky through LDS instead of the register-resident block-Thomas kernel
    int no_dense_partials;    // SGPMP_NO_DENSE_PARTIALS    update_kernel re-reads all rows with weight even when the weights are spread (round 3)
    int comm_packet_event;    // SGPMP_COMM_PACKET_EVENT    statistics all-reduce chained by the update kernel's own stop event (hipExtLaunchKernelGGL) instead of a plain event record behind it: +16 us instead of +9 us per iteration at one rank on this round's boxes (round 2's boxes had it the other way round)
    int no_planar_tail;       // SGPMP_NO_PLANAR_TAIL       store-free steps of S = 64 planar problems: update_kernel (+ regeneration, if planar_store_free) instead of the update inside fused_planar_seg_kernel
    int planar_store_free;    // SGPMP_PLANAR_STORE_FREE    store-free steps (SGPMP_STEP_NO_SAMPLES) also for fused_planar_seg_kernel: measured SLOWER at config 2 (the launch saves 3.8 us, the update's regeneration costs 5.2: 42.4 k -> 40.0 k it/s, profiles/r05), hence opt-in
    int no_planar_seg;        // SGPMP_NO_PLANAR_SEG        planar one-launch step as fused_planar_kernel (8 samples per wave through an LDS tile) even where fused_planar_seg_kernel (lane = sample, wave = time segment) applies
    int no_ee_fold;           // SGPMP_NO_EE_FOLD           the step's end-effector goal term by a launch of ee_goal_kernel in front of update_kernel (rounds 1-4) instead of inside it
    int f64_fields_f32;       // SGPMP_F64_FIELDS_F32       fp64 steps (fused_step_f64_kernel) evaluate the LINK fields -- forward kinematics, self-distance and sphere fields -- on the packed-fp32 code of the fp32 launches, from the fp64 waypoint rounded to fp32; samples, means, GP / goal-prior / importance-sampling terms stay fp64.  Opt-in: the collision part of a cost then carries fp32's ~1e-6 relative error (~1e-9 of a total cost at the reference's hyper-parameters)
    int no_persist_planar;    // SGPMP_NO_PERSIST_PLANAR    sgpmp_optimize runs the store-free iterations of a planar S = 64 problem as one launch each (round 5) instead of ONE launch for all of them (fused_planar_seg.inc: PERSIST)
    int no_small_step;        // SGPMP_NO_SMALL_STEP        small steps through fused_step_kernel (one wave per item) instead of fused_step_small_kernel (one workgroup per item)
    int fused_generic;        // SGPMP_FUSED_GENERIC        fused_step_kernel's generic instantiation (the cost program read at run time) even where the one with the four-term program compiled in applies (fused_step.inc: FULL)
    long long persist_max_iters;  // SGPMP_PERSIST_MAX_ITERS    iterations ONE launch of fused_planar_seg_kernel<.., PERSIST> runs at most (0: 2048 -- ~25 ms at BASELINE configs[1]: a launch must stay far below the driver's hang detection); longer calls take several such launches
    long long small_step_items;   // SGPMP_SMALL_STEP_ITEMS     items (groups of 8 samples) up to which a step counts as small (0: default 512 -- two workgroups per CU -- for shapes on the launch's 8 x 16 grid, 256 for the others)
    long long store_free_min_bytes;   // SGPMP_STORE_FREE_MIN_BYTES  a store-free step that REGENERATES rows in update_kernel is taken when one waypoint of all the step's samples (P S 2n floats) has at least this many bytes (0: the measured break-even, SGPMP_STORE_FREE_BREAK_EVEN; 1: always)
    long long pipe_split;     // SGPMP_PIPE_SPLIT           first chain's share of the particles in 16ths (0 = default 8)
    long long k3_blocks;      // SGPMP_K3_BLOCKS            workgroup cap of the dual sweep (0: default)
};

// ---------------------------------------------------------------------------------- update_kernel's scratch
// The dynamic LDS of one particle's update (update_common.h: update_particle), front to back, every region on 16 bytes:
// S weights (double) + S indices (int) | the new means for the importance-sampling tail, M elements | the regeneration of a
// store-free step (regen_lds_bytes) | the folded end-effector term, S doubles.  Kernels and host (update_plan.hip) read it here.
// A workgroup's dynamic LDS at most, and the reserve for the kernels' static LDS.  The code objects say more than the reserve
// (.group_segment_fixed_size, profiles/r14/update_plan.txt): update_kernel 1072 bytes with fp32 means and 1840 with fp64
// (scratch[8], nnz_s, red3[12], ee_jr, ee_ji), update_kernel_quad 0.  Kept at its value: which shapes launch is behaviour.
#define SGPMP_UPD_LDS_LIMIT 65536
#define SGPMP_UPD_LDS_RESERVE 256
constexpr size_t upd_lds_round(size_t bytes) { return (bytes + 15) & ~(size_t)15; }
constexpr bool upd_lds_fits(size_t bytes) { return bytes + SGPMP_UPD_LDS_RESERVE <= SGPMP_UPD_LDS_LIMIT; }
constexpr size_t upd_weights_bytes(int S) { return (size_t)S * 12; }
constexpr size_t upd_means_offset(int S) { return upd_lds_round(upd_weights_bytes(S)); }
// the regeneration: rows + tables + segment end states + (more rows with weight than one round holds) the carried sums
constexpr size_t regen_lds_bytes(int recipe, int T, int n, int R) {
    return (size_t)R * T * 2 * n * 4 + (size_t)T * 12 * 4 + (recipe == 2 ? (size_t)R * 16 * n * 2 * 4 : 0) + (size_t)T * 2 * n * 8;
}

#ifndef __HIPCC_RTC__     // host-side declarations: not part of the run-time (hiprtc) translation unit of chain_rtc.hip
// ---------------------------------------------------------------------------------- collectives (comm.hip)
// RCCL communicator of one context; every function returns NULL on success or a static error string.
struct SgpmpComm;
const char* comm_unique_id(unsigned char* out128);
const char* comm_create(const unsigned char* id128, int world, int rank, SgpmpComm** out);
void comm_destroy(SgpmpComm* c);
int comm_rank(const SgpmpComm* c);
int comm_world(const SgpmpComm* c);
const char* comm_library_name();
int comm_test_hooks();
const char* comm_info(const SgpmpComm* c, int* world, int* rank, int* version);   // asked of RCCL itself
const char* comm_allreduce_stats(SgpmpComm* c, double* stats, hipStream_t stream);
const char* comm_allreduce_f64(SgpmpComm* c, double* buf, size_t count, hipStream_t stream);
hipStream_t comm_side_stream(SgpmpComm* c);
const char* comm_mark_reduced(SgpmpComm* c, double* buf);
const char* comm_step_begin(SgpmpComm* c, hipStream_t stream, double** slot, hipEvent_t* k4_done);
const char* comm_step_begin2(SgpmpComm* c, hipStream_t s0, hipStream_t s1, double** slot0, double** slot1,
                             hipEvent_t* done0, hipEvent_t* done1);
const char* comm_step_end(SgpmpComm* c, double* stats, bool two_halves);
const char* comm_stats_wait(SgpmpComm* c, double* stats, hipStream_t stream);
const char* comm_allgather(SgpmpComm* c, const void* send, void* recv, size_t bytes, hipStream_t stream);

// ---------------------------------------------------------------------------------- context view (api.hip)
// `struct sgpmp_ctx` is private to api.hip; entry points that live next to their kernels (traj_dense.hip) read a context through
// this view and report through sgpmp_set_error (the message sgpmp_last_error() returns; the code is handed back).
struct SgpmpCtxView {
    sgpmp_dims dims;
    int have_chain;
    const ChainDev* h_chain;      // HOST copy of the chain (valid when have_chain)
    const ChainDev* d_chain;      // DEVICE copy
    const CostProgram* prog;      // HOST, finalized (point counts resolved, pushed to the device); null: no cost program set
    const uint32_t* pair_mask;    // [SGPMP_MAX_LINKS] bit j of word i: links i - j >= 2 whose distance depends on q
    const SgpmpToggles* tg;       // the context's development switches (the ones launch_cost picks its kernel by)
};
// fills *out; runs finalize_program when costs are set and returns its status (out->prog stays null when it fails)
int sgpmp_ctx_view(sgpmp_ctx* c, SgpmpCtxView* out);
int sgpmp_set_error(int code, const char* msg);
int sgpmp_ctx_dtype(const sgpmp_ctx* c);          // SGPMP_F32 | SGPMP_F64: all an entry point without a cost program needs

// ---------------------------------------------------------------------------------- run-time chain kernels (chain_rtc.hip)
struct RtcChain;
const char* rtc_chain_get(const char* struct_src, int n_dof, RtcChain** out);       // null on success, else the reason
hipFunction_t rtc_kernel(RtcChain* c, int ft, bool sweep, bool rag = false, bool small = false); // compiled on first use; null: unavailable (rag: the fused launch for S, T off its 8 x 16 grid)
hipError_t rtc_launch(hipFunction_t f, unsigned blocks, unsigned dyn_lds, hipStream_t stream, void** args, hipEvent_t done);
const char* rtc_verify(RtcChain* c, const ChainDev& chain, int field_type_hint, int* mismatch = nullptr);   // generated code == this chain?  (*mismatch: 1 = no, 0 = kernels unavailable)
const char* rtc_error(const RtcChain* c);
void rtc_stats(const RtcChain* c, double* compile_s, int* compiled, int* from_cache);
long long rtc_compile_check_c(const char* struct_src, int field_type, char* err, size_t err_len);   // compile only: bytes, or -1

// ---------------------------------------------------------------------------------- launchers
// (defined in the .hip files; all asynchronous on `stream`)
hipError_t launch_prior_factor(int n, int T, double dt, double ks, double kg, const double* d_qc_inv,
                               int isotropic, PriorDev out, hipStream_t stream);

hipError_t launch_prior_factor_blocks(int n, int T, int n_modes, const double* d_D, const double* d_E,
                                      PriorDev out, hipStream_t stream);
hipError_t launch_prior_quadform(int dtype, int n, int T, long long rows, int n_modes, const void* x,
                                 const void* means, const PriorDev& prior, double* out, hipStream_t stream);

hipError_t launch_sample(int dtype, int n, int T, const PriorDev& prior, uint64_t seed, uint64_t draw,
                         const void* means, int n_modes, int mode_offset, int n_samples,
                         const void* eps, int eps_modes, int eps_mode_offset, void* out,
                         hipStream_t stream, const SgpmpToggles& tg, double* zero_stats = nullptr);

hipError_t launch_noise(int dtype, int n, int T, int n_modes, int mode_offset, int S, uint64_t seed, uint64_t draw, void* out,
                        hipStream_t stream);

hipError_t launch_cost(int dtype, int n, int T, const CostProgram& h_prog, const ChainDev* d_chain,
                       const ChainDev& h_chain, const void* trajs, long long batch,
                       long long batch_offset, const void* spheres, int n_spheres,
                       const void* is_weights, int rows_per_particle, double is_dt, void* costs,
                       double* costs64, hipStream_t stream, const SgpmpToggles& tg, const char** picked);

// What the fused launch and the update behind it agree on, per particle, through the count of rows that carried weight in
// the particle's PREVIOUS update (a device word: stream-ordered, no host round trip, the same in every run):
//  * dense-weight regime (FusedArgs::part): particles above `threshold` get softmax partials from the launch;
//  * store-free steps (FusedArgs::nostore): only particles above `store_threshold` have their rows written.
struct FusedDenseHost {
    float* part;                  // [P][ceil(S / 8)][4 + T d], or null (not an fp32 chain-code step, switched off)
    unsigned* nnz;                // [P] rows with weight in each particle's previous update
    unsigned threshold;           // partials for particles with nnz above it
    double temperature;
    unsigned store_threshold;     // store-free steps: rows are stored for particles with nnz above it only
    // the update INSIDE fused_planar_seg_kernel (StepPlan::update_in_launch; fused_planar_seg.inc: seg_update) -- what update_kernel
    // would have been given
    unsigned* tail_done;          // finished-particle counter of this launch (zero between launches)
    double* tail_acc;             // [SGPMP_STAT_SHARDS][4] statistics accumulators (zero between launches)
    double* stats_out;            // the step's statistics buffer or null
    void* weights; void* grad; void* means_prev;   // K4's optional outputs (context dtype)
    double step_size;
};
// bytes of one waypoint of all samples of a step above which a regenerating store-free step is faster than a storing one
// (step_plan.hip: plan_step has the measurement)
#define SGPMP_STORE_FREE_BREAK_EVEN 2800000LL
// The step's end-effector goal term evaluated by update_kernel itself (update_common.h: EeFold) instead of ee_goal_kernel
struct EeFoldHost {
    const CostTerm* term;         // the SGPMP_COST_EE_GOAL term
    const ChainDev* d_chain;      // DEVICE chain
    void* costs;                  // [P][S] cost output of the step (context dtype) or null
};
// How update_kernel regenerates the rows a store-free step did not write (update_common.h: RegenArgs)
struct RegenHost {
    int recipe;                   // 0: all rows are in memory; 1: fused_step_kernel's rows; 2: fused_planar_seg_kernel's (segments of L)
    int L;
    uint64_t seed, draw;
    int mode_offset;              // global index of the launch's particle 0
    const float* coef;            // recipe 1: PriorDev::iso32p; 2: PriorDev::iso32
    const float* pre;             // recipe 2: the segment table of PriorDev::slabpre
    unsigned store_threshold;
    int beside_chain;             // the launch is one half of a two-chain step: it runs beside the other half's fused launch (which update
                                  // kernel launch_update takes; set with recipe 0 too)
};
// update_kernel_quad (update.hip): particles per workgroup, one wave each; the most samples and the range of particles of a
// half's launch that takes it by default (update_plan.hip: update_quad_applies has the measurements)
#define SGPMP_UPD_QUAD 4
#define SGPMP_UPD_QUAD_MAX_S 256
#define SGPMP_UPD_QUAD_MIN_P 512
#define SGPMP_UPD_QUAD_END_P 1024
// Development switch `update_wide` (sgpmp_set_option / SGPMP_UPDATE_WIDE): > 0: every update launch takes update_kernel (one
// 256-thread workgroup per particle); < 0: update_kernel_quad wherever it can run, also where it is not the faster one; 0: the
// measured rule.  PROCESS-WIDE, unlike the switches of SgpmpToggles: the callers of plan_update read it here
// (one variable for the whole library: C++17 inline).  SGPMP_UPDATE_WIDE is read ONCE per process, by the first sgpmp_create;
// after that only sgpmp_set_option changes it, for every context of the process.
inline int g_sgpmp_update_wide = 0;

// ---------------------------------------------------------------------------------- the update launch (update_plan.hip)
// ONE decision per update launch, a function of its arguments alone (no HIP call): tail kept or dropped, the regions of the
// kernel's scratch, one wave or one workgroup per particle, grid, vector width.
struct UpdateShape { int dtype, costs_dtype, n, T, S, P; };
// isw_tail: the next step's importance-sampling weights are wanted (written if the new means fit beside the weights);
// regen_recipe, beside_chain: RegenHost's; ee_fold: EeFoldHost::term is there; has_nnz: the per-particle row counts are there
struct UpdateWants { bool isw_tail; int regen_recipe; bool ee_fold; bool beside_chain; bool has_nnz; };
struct UpdatePlan {
    UpdateShape shape; bool ok;   // false: not this shape -- launch_update returns hipErrorInvalidValue
    bool tail;                    // the kernel writes the next step's weights (what the step reports as prepared, when P > 0)
    int regen_rows;               // RegenArgs::R
    unsigned regen_off, ee_off;   // where the regeneration and the end-effector term's S doubles begin in a particle's scratch
    unsigned slice, lds;          // one particle's scratch, rounded; dynamic LDS of the launch (quad: four slices)
    bool quad; unsigned grid; int vw; const char* kernel;   // update_kernel_quad?  workgroups, elements per thread and load
};
UpdatePlan plan_update(const UpdateShape& shape, const UpdateWants& wants, int update_wide);
int update_regen_rows(int dtype, int n, int T, int S, int recipe);   // rows per round update_kernel can regenerate; 0: not this shape
bool update_ee_fold_fits(int dtype, int n, int T, int S);

// ---------------------------------------------------------------------------------- the step's launches (step_plan.hip)
// ONE decision per launch sequence: which kernels a particle range's step runs.  plan_step is a function of its arguments
// alone (apart from the lookup of a run-time chain's kernel, compiled on first use: no device call, no context), so the
// choice is a function of the shape -- the same in every run, as one optimize(K) call or K calls, sharded or not.
struct StepShape {
    int dtype, n, T, S, n_spheres;
    int P, offset;                // the particle range the sequence runs and the global index of its particle 0
    int particles_total;          // particles of the whole step (a two-chain step launches halves): what a regenerating store-free step is judged on
    int particles_global;         // ... of all ranks: what the small-step launch is judged on
};
struct StepWants {                // what the caller offers
    bool eps;                     // the caller brings the noise: sampler + sweep
    bool no_samples;              // SGPMP_STEP_NO_SAMPLES: nobody reads this step's samples
    bool update_in_launch_ok;     // nothing wants update_kernel's own outputs (per-step mean statistics do)
    int iters;                    // iterations asked of ONE launch (sgpmp_optimize; 1 otherwise)
};
enum StepFamily { STEP_NONE = 0, STEP_CHAIN, STEP_CHAIN_RTC, STEP_PLANAR_TILE, STEP_PLANAR_SEG, STEP_F64 };
enum StepEe { STEP_EE_NONE = 0, STEP_EE_FOLD, STEP_EE_LAUNCH };
struct StepPlan {
    StepShape shape;
    int family;                   // STEP_NONE: sampler + sweep as launches of their own
    bool ragged;                  // chain code: S, T off the launch's grid of 8 rows x 16 waypoints (the masked instantiation)
    bool small;                   // chain code: one WORKGROUP per item (fused_step_small_kernel)
    bool mixed;                   // fp64: link fields on the packed-fp32 code
    int field_type;               // chain code: SGPMP_FIELD_* of the sphere term
    int L;                        // planar: waypoints per wave of the lane-per-sample launch the SHAPE allows (0: none); the launch is
                                  // STEP_PLANAR_SEG when its grid fits too
    int seg_table;                // ... and its table of PriorDev::slabpre (3: segments of 8, 4: of 16)
    unsigned seg_lds;             // STEP_PLANAR_SEG: dynamic LDS of the launch (with the update's share when it runs inside)
    hipFunction_t rtc_fn;         // STEP_CHAIN_RTC: the kernel
    long long block_cap;          // workgroups of the grid-stride launches at most
    bool partials;                // the launch leaves softmax partials for the update (FusedDenseHost::part must be there)
    int full;                     // chain code: fused_step_kernel's instantiation (fused_full_variant; 0: the generic one)
    int regen_recipe;             // store-free step whose update_kernel regenerates rows: RegenHost::recipe (0: the step stores, or has no update_kernel)
    bool update_in_launch;        // the launch updates its particles itself: no update_kernel behind it
    int max_iters;                // iterations one such launch may carry (1, or the PERSIST cap)
    int iters;                    // ... and carries: StepWants::iters where the plan can (the caller compares), else 1
    int ee;                       // StepEe: the end-effector goal term(s) of a fused step
    const char* kernel;           // what sgpmp_last_cost_kernel reports
};
StepPlan plan_step(const StepShape& shape, const StepWants& wants, const PriorDev& prior, const CostProgram& prog,
                   const ChainDev& chain, const SgpmpToggles& tg);
// Which instantiation of fused_step_kernel a chain-code plan launches (fused_step.inc: FULL).  0: the generic one, which reads the
// cost program at run time.  1, 2: the program compiled in -- exactly GP term with start prior + goal prior + self term + sphere
// term, a storing launch of the library's own chain code on the 8 x 16 grid, one wave per item; 1 without softmax partials, 2 with
// the partials buffer armed.  A function of its arguments alone (tests/host_asan/fused_full_table.cpp walks it).
int fused_full_variant(const StepPlan& plan, const CostProgram& prog, const SgpmpToggles& tg);
// what update_kernel is told behind a launch of this plan (recipe 0: nothing to regenerate)
static inline RegenHost plan_regen(const StepPlan& plan, const PriorDev& prior, uint64_t seed, uint64_t draw, unsigned store_threshold) {
    RegenHost r = {};
    r.beside_chain = plan.shape.P < plan.shape.particles_total;   // (a half of a two-chain step: api.hip, plan_two_chains)
    if (plan.regen_recipe == 0) return r;
    r.recipe = plan.regen_recipe; r.L = r.recipe == 2 ? plan.L : 0; r.seed = seed; r.draw = draw; r.mode_offset = plan.shape.offset;
    r.coef = r.recipe == 1 ? prior.iso32p : prior.iso32;
    r.pre = r.recipe == 2 ? prior.slabpre + (size_t)plan.seg_table * plan.shape.T * 4 : nullptr;
    r.store_threshold = store_threshold;
    return r;
}
struct StepIo {
    const PriorDev* prior; const CostProgram* prog; const ChainDev* chain;
    uint64_t seed, draw;
    const void* means; void* samples; const void* spheres; const void* isw;
    double* zero_stats; void* costs; double* costs64;
    hipStream_t stream;
    FusedDenseHost dense;
};
// K2 + K3 fused (cost_sweep.hip / fused_step.inc): enqueues exactly what the plan says (never a plan of STEP_NONE)
hipError_t launch_fused_step(const StepPlan& plan, const StepIo& io);

hipError_t launch_is_weights(int dtype, int n, int T, const PriorDev& prior, const void* means,
                             int n_particles, double temperature, void* out, double* zero_stats,
                             hipStream_t stream);

struct UpdateIo {                 // (everything behind `stream` may be null / zero; isw_prior and isw_next: both or neither)
    const void* costs; const void* samples; void* means; double temperature, step_size;
    void* weights; void* grad; void* means_prev; double* stats; hipStream_t stream; hipEvent_t done;
    const PriorDev* isw_prior; void* isw_next; void* means_copy; const float* part; unsigned* nnz; unsigned nnz_threshold;
    RegenHost regen; EeFoldHost ee;
};
static inline UpdateWants update_wants(const UpdateIo& io) {
    return {io.isw_prior && io.isw_next, io.regen.recipe, io.ee.term != nullptr, io.regen.beside_chain != 0, io.nnz != nullptr};
}
// K4 (update.hip): enqueues exactly what the plan says; P <= 0 is a successful no-op
hipError_t launch_update(const UpdatePlan& plan, const UpdateIo& io);

hipError_t launch_stats_add(double* dst, const double* src, hipStream_t stream);
hipError_t launch_mode_stats(int dtype, int n, int T, int P, long long p_offset, int nppg, int G, const void* means,
                             double* out, hipStream_t stream);
hipError_t launch_ee_goal(int dtype, int n, int T, const CostTerm& term, const ChainDev* d_chain,
                          const void* trajs, long long batch, void* costs, double* costs64,
                          hipStream_t stream);
hipError_t launch_ee_grad(int dtype, int n, const CostTerm& term, const ChainDev* d_chain, const void* q,
                          long long batch, int traj_T, long long out_stride, long long out_offset, void* value,
                          void* grad, hipStream_t stream);
hipError_t launch_field_grad(int dtype, int n, const CostTerm& term, const ChainDev* d_chain, int n_joints,
                             const void* q, long long batch, int traj_T, const void* spheres, int n_spheres,
                             void* value, void* grad, hipStream_t stream);
// A launch whose dynamic LDS (plus the kernel's static LDS) exceeds 64 KiB has the kernel's dynamic-LDS limit raised first, as the
// HIP API asks (a gfx950 workgroup may use up to 160 KiB).  Measured on the MI355X: this runtime also accepts such a launch
// without the call; every launcher makes it all the same, so that no two files of the library disagree about the contract.
template <typename Kernel>
static inline hipError_t sgpmp_allow_lds(Kernel kernel, size_t dynamic_bytes, size_t static_bytes = 0) {
    if (dynamic_bytes + static_bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dynamic_bytes);
}

// GPMP (gpmp.hip)
#define SGPMP_MAX_T_GPMP 128
#define SGPMP_MAX_GPMP_FIELDS 4   // link-field terms of one cost list
// Particles per wave and dynamic LDS of gpmp_thomas_kernel.  A particle stages per = 8 T (32 + 9 F) bytes (means and solution
// [T][16] doubles each, F field values [T] and gradients [T][8]); four particles share a wave, one per row of 16 lanes, while
// 4 per <= 150 KiB (of the 160 KiB a workgroup may use; the kernel adds 512 B of static LDS), else two.  Two always fit: the
// largest admissible request, T = 128 and F = 4, is per = 69 632 B, 2 per = 139 264 B <= 153 600 B -- a one-per-wave layout would
// need per > 76 800 B and cannot be reached, so there is none.  Raising either limit below forces a fresh look.
struct GpmpSolveLayout { int ppw; size_t per_particle, lds; };    // lds = ppw * per_particle
static inline GpmpSolveLayout gpmp_solve_layout(int T, int n_fields) {
    static_assert((size_t)2 * 8 * SGPMP_MAX_T_GPMP * (32 + 9 * SGPMP_MAX_GPMP_FIELDS) <= (size_t)150 * 1024,
                  "gpmp_thomas_kernel: two particles per wave no longer fit the LDS at the largest T and field count");
    const size_t per = (size_t)8 * T * (32 + 9 * n_fields);
    const int ppw = 4 * per <= (size_t)150 * 1024 ? 4 : 2;
    return {ppw, per, ppw * per};
}
struct GpmpFieldK {               // one link-field term of the cost list
    double K;                     // 1 / sigma^2
    const void* val;              // [P, T-1]   field values        (context dtype)
    const void* grad;             // [P, T-1, n] d field / d q       (context dtype)
};

struct GpmpArgs {
    int n, T, P;
    long long p_offset;           // global index of particle 0 (goal lookup)
    double dt, Kgp, c11, c12, c22;   // cost GP term: Q^-1 = Kgp [[c11, c12], [c12, c22]] (x) I_n
    double Ks;                    // start prior weight (0: no start factor)
    const void* start;            // [d] context dtype
    double Kg;                    // goal prior weight (0: none)
    const void* goals;            // [G, d]
    long long rows_per_goal;      // particles per goal
    int n_fields;
    GpmpFieldK f[SGPMP_MAX_GPMP_FIELDS];
    double delta;
    const double* diag_sum;       // [T*d] sum over all particles of the FIELD part of diag(A^T K A), or null
    double inv_particles;         // 1 / (global particle count)
    double step_size;
    double* scratch;              // [P][T][2][256]
    int* status;                  // set to 1 when a pivot is not positive
};

hipError_t launch_gpmp_diag(int dtype, const GpmpArgs& a, double* diag_sum, hipStream_t stream);
hipError_t launch_gpmp_solve(int dtype, const GpmpArgs& a, void* means, void* d_theta, void* costs,
                             hipStream_t stream, bool cholesky = false);

// The Hermite weights of the dense trajectories as a plain table (traj_dense.hip: hermite_coefs, the weights hermite_state
// applies): per sub-step m = 1 .. k, q = c0 q_i + c1 v_i + c2 q_{i+1} + c3 v_{i+1}, v = c4 .. c7 likewise, in the context's dtype.
template <typename real>
struct HermiteTab { real c[SGPMP_MAX_SUBSTEPS][8]; };
void hermite_table(int dtype, int n_sub, double dt, void* out);

// GPMP with continuous-time factors (gpmp_dense.hip): collision rows on the n_sub inserted states of every interval and limit
// rows on all fine states, beside GpmpArgs.  With it GpmpFieldK::val / grad are [P, T_f - 1] / [P, T_f - 1, n] over the fine
// states 1 .. T_f - 1.
struct GpmpDenseArgs {
    int n_sub, Tf;                // k states inserted per interval; T_f = (T - 1)(k + 1) + 1
    double dt;                    // of the interpolation
    double weight;                // scales the precision of the inserted states' collision rows
    double Klim;                  // 1 / sigma_limit^2, 0: no limit rows
    int has_lo, has_hi, has_v;
    double q_lo[SGPMP_MAX_DOF], q_hi[SGPMP_MAX_DOF], v_max[SGPMP_MAX_DOF];
    int inserted[4];              // link-field term k has rows on the inserted states (an end-effector goal has its one row)
};
// api.hip is also linked WITHOUT the kernel files (tests/host_asan: the host bookkeeping over a stub runtime): what it calls
// of gpmp_dense.hip is declared weak, and sgpmp_gpmp_set_dense refuses where the definitions are absent.
hipError_t launch_gpmp_fine(int dtype, int n, int T, const void* means, long long P, int n_sub, double dt, void* fine,
                            hipStream_t stream) __attribute__((weak));
hipError_t launch_gpmp_dense_diag(int dtype, const GpmpArgs& a, const GpmpDenseArgs& da, const void* means, double* diag_sum,
                                  hipStream_t stream) __attribute__((weak));
hipError_t launch_gpmp_dense_solve(int dtype, const GpmpArgs& a, const GpmpDenseArgs& da, void* means, void* d_theta,
                                   void* costs, hipStream_t stream) __attribute__((weak));
// SGPMP_COST_GRID_SDF (sdf.hip): hinge value [batch] and gradient [batch, n] (entries >= 2 zero) of the term at the planar
// point (q[0], q[1]); q laid out as launch_field_grad's (traj_T = 0: [B, n]; traj_T = T: waypoints 1 .. T-1 of [P, T, 2n]).
// Weak for the same reason: sgpmp_field_grad and the GPMP linearisation refuse the kind where the definition is absent.
hipError_t launch_grid_sdf_grad(int dtype, int n, const CostTerm& term, const void* q, long long batch, int traj_T, void* value,
                                void* grad, hipStream_t stream) __attribute__((weak));
// SGPMP_COST_BODY_SDF (body_sdf.hip; term.body / term.n_body: the table): body_cost_kernel adds K * sum over waypoints 1 .. T-1 of the
// field to costs / costs64 [batch] behind the sweep; body_grad_kernel: value [batch] and gradient [batch, n], q laid out as
// launch_field_grad's, the query flag included; body_eval_kernel: frames [batch, n_links, 4, 4] -> the field [batch].  Weak for
// the same reason: sgpmp_set_costs refuses the kind where the definitions are absent.
hipError_t launch_body_cost(int dtype, int n, int T, const CostTerm& term, const ChainDev* d_chain, const void* trajs,
                            long long batch, void* costs, double* costs64, hipStream_t stream) __attribute__((weak));
hipError_t launch_body_grad(int dtype, int n, const CostTerm& term, const ChainDev* d_chain, int n_joints, const void* q,
                            long long batch, int traj_T, void* value, void* grad, hipStream_t stream) __attribute__((weak));
hipError_t launch_body_eval(int dtype, const CostTerm& term, const void* frames, long long batch, int n_links, void* out,
                            hipStream_t stream) __attribute__((weak));
// SGPMP_COST_BODY_SELF (body_self.hip; term.body / term.n_body: the table, with the pair rows of sgpmp_set_body_pairs behind it;
// term.K2: the margin): the same three launches for the body's sphere pairs, with the same arguments.  Weak for the same reason.
hipError_t launch_body_self_cost(int dtype, int n, int T, const CostTerm& term, const ChainDev* d_chain, const void* trajs,
                                 long long batch, void* costs, double* costs64, hipStream_t stream) __attribute__((weak));
hipError_t launch_body_self_grad(int dtype, int n, const CostTerm& term, const ChainDev* d_chain, int n_joints, const void* q,
                                 long long batch, int traj_T, void* value, void* grad, hipStream_t stream) __attribute__((weak));
hipError_t launch_body_self_eval(int dtype, const CostTerm& term, const void* frames, long long batch, int n_links, void* out,
                                 hipStream_t stream) __attribute__((weak));
hipError_t launch_link_dist(int dtype, const void* frames, long long batch, int n_links, const void* spheres,
                            int n_other, int mode, double buffer, void* out, hipStream_t stream);
hipError_t launch_fk(int dtype, int n, const ChainDev* d_chain, int n_links, const void* q,
                     long long batch, void* frames, hipStream_t stream);
hipError_t launch_grid_lookup(int dtype, const CostTerm& term, const void* xy, long long batch,
                              void* out, hipStream_t stream);
hipError_t launch_field_eval(int dtype, const CostTerm& term, const void* frames, long long batch,
                             int n_links, const void* spheres, int n_spheres, void* out,
                             hipStream_t stream);
#endif  // !__HIPCC_RTC__
