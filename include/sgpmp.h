/*
 * sgpmp.h -- C ABI of libsgpmp.so: the MI355X (gfx950) StochGPMP inner loop.
 *
 * The reference (anindex/stoch_gpmp) is pure Python and has no FFI of its own; its boundary for this
 * path is the Python API of `stoch_gpmp.planner.StochGPMP` and `stoch_gpmp.costs.*`.  Every entry
 * point below therefore cites the reference Python function whose work it performs; the Python
 * classes in `stoch_gpmp_amd/` keep the reference's names/signatures and forward here via ctypes
 * (the binding a reference maintainer would add is shown in INTEGRATION.md).
 *
 * Conventions
 *   - All tensor memory is owned by the caller (torch tensors used as containers); the library
 *     borrows raw DEVICE pointers for the duration of the stream operation it enqueues.  The
 *     library owns only small factor / descriptor / scratch buffers inside the context.
 *   - `dtype`: SGPMP_F32 or SGPMP_F64 is the element type of every `void*` tensor argument of a
 *     context.  Prior factors are always computed in fp64.
 *   - Layouts are dense row-major: means [P,T,d], samples [P,S,T,d], costs/weights [P,S],
 *     d = 2*n_dof = (positions, velocities)  (reference planner.py:52, 215, 227).
 *   - Every call returns 0 on success or a negative SGPMP_E* code; `sgpmp_last_error()` returns a
 *     thread-local message.  All launches are asynchronous on the caller's `stream`
 *     (a hipStream_t passed as void*; NULL = default stream) except where noted.
 *   - A context is bound to the device current at creation and is not thread-safe.
 */
#ifndef SGPMP_H
#define SGPMP_H

#ifndef __HIPCC_RTC__          /* (the run-time compiler of the chain kernels has the fixed-width types built in) */
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* 2: sgpmp_step gained `flags`, sgpmp_set_priors / pipeline_* / comm_* appeared (round 2); 3: round 3 (see git log);
 * 4: sgpmp_comm_library, sgpmp_set_fk_codegen / _info / _compile, sgpmp_dense_particles (round 4);
 * 5: SGPMP_STEP_NO_SAMPLES, sgpmp_row_counts_get / _set, sgpmp_store_free_steps, sgpmp_step honours per-mode sampling
 *    precisions; the options of the retired experiments are gone (round 5);
 * 6: sgpmp_optimize (the K-loop of optimize() behind the ABI), sgpmp_row_counts_clear, sgpmp_noise, sgpmp_multi_iteration_launches;
 *    fp64 contexts draw the fp32 noise stream, widened (round 6).
 * The Python binding refuses any other value at load time. */
#define SGPMP_ABI_VERSION 6

enum { SGPMP_F32 = 0, SGPMP_F64 = 1 };
enum { SGPMP_PRIOR_INIT = 0, SGPMP_PRIOR_SAMPLE = 1 };

enum {
    SGPMP_OK = 0,
    SGPMP_EINVAL = -1,     /* bad argument / unsupported size  (Python: AssertionError/ValueError) */
    SGPMP_ENOTPD = -2,     /* prior precision not positive definite (Python: ValueError, as torch's
                              MultivariateNormal raises in the reference, README.md:35)            */
    SGPMP_EHIP = -3,       /* HIP runtime error                                                     */
    SGPMP_ESTATE = -4      /* call order violated (e.g. step before set_prior)                      */
};

/* Cost-term kinds: one per reference Cost class on the StochGPMP path. */
enum {
    SGPMP_COST_GP = 1,          /* CostGP.eval / CostGPTrajectory.eval   cost_functions.py:128-146,202-215 */
    SGPMP_COST_GOAL_PRIOR = 2,  /* CostGoalPrior.eval                    cost_functions.py:376-388         */
    SGPMP_COST_GRID = 3,        /* CostCollision + ObstacleMap           cost_functions.py:247-261, obst_map.py:164-185 */
    SGPMP_COST_SPHERES = 4,     /* CostCollision + LinkDistanceField     fields.py:63-86                   */
    SGPMP_COST_SELF = 5,        /* CostCollision + LinkSelfDistanceField fields.py:114-124                 */
    SGPMP_COST_EE_GOAL = 6,     /* CostGoal + EESE3DistanceField         cost_functions.py:282-321, fields.py:130-153
                                   (SE3_distance itself is third-party and un-vendored: DESIGN.md)      */
    SGPMP_COST_GRID_SDF = 7,    /* CostCollision + GridDistanceField: hinge on a signed-distance grid (no reference
                                   counterpart; defined at sgpmp_grid_sdf_build below)                   */
    SGPMP_COST_VOXEL_SDF = 8,   /* CostCollision + VoxelDistanceField: hinge on a voxel signed-distance field at the link
                                   points (no reference counterpart; defined at sgpmp_voxel_sdf_build below) */
    SGPMP_COST_BODY_SDF = 9,    /* CostCollision + BodyDistanceField: the same hinge at the body's collision spheres, each with
                                   its radius (no reference counterpart; defined at sgpmp_set_body below) */
    SGPMP_COST_BODY_SELF = 10   /* CostCollision + BodySelfDistanceField: hinge on the clearance between the body's own spheres,
                                   over the counted pairs (no reference counterpart; defined at sgpmp_set_body_pairs below) */
};
enum { SGPMP_FIELD_RBF = 0, SGPMP_FIELD_SDF = 1, SGPMP_FIELD_OCCUPANCY = 2 };
#define SGPMP_FLAG_GP_START 1      /* GP term includes the start-state unary factor (CostGP)  */
#define SGPMP_FLAG_SDF_CLAMP 16    /* LinkDistanceField(clamp_sdf=True)                       */
#define SGPMP_FLAG_EE_SQUARE 32    /* EESE3DistanceField(square=True)                         */
#define SGPMP_FLAG_GRID_DISTANCE 64 /* GRID_SDF: sgpmp_field_grad returns the interpolated distance d and dd/d(x, y) instead of
                                      the hinge and its gradient (GridDistanceField.compute_distance).  A query flag, not a cost:
                                      allowed only in a cost list whose single term is this one (else SGPMP_EINVAL), and the
                                      GPMP linearisation refuses a term that carries it.  VOXEL_SDF: the same query, min over
                                      the link points of d and the gradient through the first arg-min point.  BODY_SDF: min over
                                      the body's spheres of the clearance d - r and the gradient through the first arg-min sphere.
                                      BODY_SELF: min over the counted pairs of the clearance D - r_i - r_j and the gradient through
                                      the first arg-min pair */

#define SGPMP_MAX_TERMS 8
#define SGPMP_MAX_JOINTS 16
#define SGPMP_MAX_DOF 8            /* state blocks are handled as one 16x16 MFMA tile        */
#define SGPMP_MAX_INTERP 8
#define SGPMP_MAX_BODY 64          /* collision spheres of a body (sgpmp_set_body)           */
#define SGPMP_STAT_SHARDS 64       /* statistics buffers are double[SGPMP_STAT_SHARDS][4]; sum over shards */

typedef struct sgpmp_dims {
    int32_t n_dof;                 /* n;  d = 2n                                                  */
    int32_t traj_len;              /* T                                                           */
    int32_t num_particles;         /* particles held by THIS context (local shard)                */
    int32_t particle_offset;       /* global index of local particle 0 (multi-GPU sharding)       */
    int32_t num_particles_global;  /* G * nppg                                                    */
    int32_t num_samples;           /* S                                                           */
    int32_t num_goals;             /* G (1 when not goal-directed)                                */
    int32_t num_particles_per_goal;/* nppg; goal of global particle p is p / nppg                 */
    int32_t dtype;                 /* SGPMP_F32 | SGPMP_F64                                       */
    int32_t reserved;
} sgpmp_dims;

typedef struct sgpmp_cost_desc {
    int32_t kind;                  /* SGPMP_COST_*                                                */
    int32_t flags;                 /* GP: SGPMP_FLAG_GP_START; SPHERES: SGPMP_FIELD_* | SGPMP_FLAG_SDF_CLAMP;
                                      GRID_SDF, VOXEL_SDF: SGPMP_FLAG_GRID_DISTANCE                */
    double sigma;                  /* GP: sigma_gp; GOAL_PRIOR: sigma_goal_prior; collision: sigma_coll */
    double sigma2;                 /* GP: sigma_start; SELF: margin; GRID_SDF, VOXEL_SDF: margin (>= 0) */
    double dt;                     /* GP: time step; VOXEL_SDF: the z offset oz                   */
    const void* data;              /* GP: HOST double[d] start state; GOAL_PRIOR: HOST double[G*d]
                                      goal states; GRID: DEVICE grid [dim0,dim1] in ctx dtype;
                                      GRID_SDF: DEVICE sdf [dim0 = ny, dim1 = nx] in ctx dtype;
                                      VOXEL_SDF: DEVICE sdf [reserved = nz, dim0 = ny, dim1 = nx] in ctx dtype;
                                      EE_GOAL: HOST double[16] target frame (row-major 4x4), with
                                      p0 = w_pos, p1 = w_rot                                      */
    int32_t dim0, dim1;            /* GOAL_PRIOR: G, nppg*S of the cost (cost_functions.py:379);
                                      GRID, GRID_SDF: map.shape[0], map.shape[1]; VOXEL_SDF: ny, nx */
    double p0, p1, p2;             /* GRID, GRID_SDF: cell_size, c_offset[0], c_offset[1] (obst_map.py:129-140);
                                      VOXEL_SDF: cell, ox, oy                                     */
    int32_t num_interpolate;       /* fields.py:32,94                                             */
    int32_t interp_lo, interp_hi;  /* link_interpolate_range                                      */
    int32_t reserved;              /* VOXEL_SDF: nz (0 for every other kind)                      */
    double alpha[SGPMP_MAX_INTERP];/* interpolation weights torch.linspace(0,1,K+2)[1:K+1] (fields.py:69) */
} sgpmp_cost_desc;

/* One joint of a serial URDF chain: H_child = H_parent * Trans(xyz) * RPY(rpy) * Rz(q).
 * The FK callable of the reference (cost_functions.py:39,51-52) is third-party; see DESIGN.md. */
typedef struct sgpmp_joint {
    double rpy[3];
    double xyz[3];
    int32_t revolute;              /* 1: consumes the next joint coordinate; 0: fixed             */
    int32_t reserved;
} sgpmp_joint;

typedef struct sgpmp_ctx sgpmp_ctx;

int sgpmp_abi_version(void);
/* Rounds of the Philox4x32 bijection behind the in-kernel noise (csrc/rng.h, build parameter SGPMP_PHILOX_ROUNDS: 10 =
 * Random123's default, 7 = its documented Crush-resistant minimum): the CPU restatement of the stream
 * (oracle/native_noise.py) must be run with the same count. */
int sgpmp_philox_rounds(void);
const char* sgpmp_last_error(void);

/* ---- context ---------------------------------------------------------------------------------- */
/* StochGPMP.__init__ / reset bookkeeping (planner.py:20-82,181-227). Synchronous. */
int sgpmp_create(const sgpmp_dims* dims, sgpmp_ctx** out);
void sgpmp_destroy(sgpmp_ctx* ctx);

/* Development switches (kernel-variant A/B, tests of the fallback paths).  Every switch has an
 * environment variable SGPMP_<NAME> that is read ONCE, in sgpmp_create; this call changes a switch
 * on a live context.  Names: force_generic_fk, no_flat_program, no_chain_codegen, no_dual_sweep,
 * k3_no_one, k3_no_lds_prefetch, no_small_sampler, no_fused_step, no_chunked_sweep, no_step_pipeline, comm_packet_event,
 * gpmp_cholesky (GPMP solve by round 3's LDS block-Cholesky kernel), no_dense_partials (dense-weight regime: update_kernel re-reads every row with weight, as in round 3),
 * no_planar_seg (planar one-launch step through the LDS tile, fused_planar_kernel, even where the lane-per-sample launch applies),
 * planar_store_free (store-free planar steps of ANY sample count by regenerating rows in update_kernel: bit-identical, measured slower
 * than storing at BASELINE configs[1]; problems with 64 samples per particle run store-free by default, with the update inside the launch),
 * no_planar_tail (those steps with update_kernel behind the launch instead),
 * no_persist_planar (sgpmp_optimize runs the store-free iterations of such a problem one launch each, as round 5 did, instead of
 * all of them in ONE launch: bit-identical, 1.4 x slower per iteration at BASELINE configs[1]),
 * persist_max_iters (count: iterations one such launch runs at most; 0: 2048 -- a longer call takes several launches),
 * no_ee_fold (the step's end-effector goal term by a launch of ee_goal_kernel in front of update_kernel, as in rounds 1-4, instead of
 * inside update_kernel: same numbers, one launch more),
 * no_small_step (steps of up to small_step_items items -- groups of 8 samples; default 512, two per CU, 256 for shapes off the
 * launch's 8 x 16 grid -- go out as
 * fused_step_small_kernel, one WORKGROUP per item with its four waves on the item's time chunks side by side, bit-identical to
 * the one-wave-per-item launch and about twice as fast where every wave sits alone on its SIMD; 1: always fused_step_kernel),
 * small_step_items (count),
 * store_free_min_bytes (a store-free step that regenerates rows in update_kernel is taken when one waypoint of all the step's
 * samples -- P S 2n floats -- has at least this many bytes; 0: the measured break-even of 2.8 MB, below which it ran 4 .. 20 %
 * slower than a storing step; 1: always),
 * f64_fields_f32 (opt-in, fp64 contexts: the one-launch step evaluates the LINK fields -- forward kinematics, self-distance and
 * sphere fields -- on the fp32 launches' packed code from the fp64 waypoint rounded to fp32; noise, recurrence, samples, means and
 * the GP / goal-prior / importance-sampling terms stay fp64.  The collision part of a cost then carries fp32's ~1e-6 relative
 * error -- ~1e-9 of a total cost at the reference's hyper-parameters -- and the step runs 1.7 x as fast: 0.46 against 0.79 ms at BASELINE configs[2]'s shape; the occupancy COUNT is then taken on
 * fp32 link positions too: a point within fp32 rounding of a sphere's surface may count differently, one quantum 1 / sigma_coll^2),
 * update_wide (1: update launches take update_kernel, one 256-thread workgroup per particle, even where update_kernel_quad -- one
 * wave per particle, four particles per workgroup; the default for the halves of a two-chain step that store their samples, have
 * no folded end-effector term, 512 to 1023 particles and at most 256 samples per particle, where it measured faster -- applies;
 * -1: update_kernel_quad wherever it can run; 0: the rule.  Bit-identical.  PROCESS-WIDE, unlike every other switch: it holds for
 * all contexts of the process; SGPMP_UPDATE_WIDE is read once per process, by the first sgpmp_create),
 * fused_generic (fused_step_kernel's generic instantiation, which reads the cost program at run time, even where the one with the
 * four-term program compiled in applies -- sgpmp_last_fused_variant; bit-identical),
 * pipe_split (1..15) and k3_blocks (count).  (The launches that measured slower -- tail_update, small_step, planar_slabs,
 * wave_groups, fused_pipe -- were removed in round 5; DESIGN.md 8 keeps their numbers and the commit that last held them.)
 * No reference counterpart. */
int sgpmp_set_option(sgpmp_ctx* ctx, const char* name, long long value);
/* Name of the cost-sweep kernel the dispatcher chose at the last sgpmp_cost_eval / sgpmp_step
 * (static string; "" before the first launch).  For bench.py's roofline label and the tests that
 * must prove which kernel they exercised. */
const char* sgpmp_last_cost_kernel(sgpmp_ctx* ctx);
/* Which instantiation of fused_step_kernel the last fused launch of sgpmp_step / sgpmp_optimize was.  0: the generic one (and every
 * other fused launch).  1, 2: the one with the cost program compiled in -- exactly GP term with start prior, goal prior, self term
 * and sphere term, a storing step on the launch's grid of 8 samples x 16 waypoints; 1 without softmax partials (no_dense_partials),
 * 2 with the partials buffer armed (the default).  Same samples and costs, bit for bit. */
int sgpmp_last_fused_variant(sgpmp_ctx* ctx);

/* K1. GP-prior precision blocks + reverse block-Cholesky, fp64, one launch.
 * Replaces GPFactor.calc_phi/calc_Q_inv (gp_factor.py:36-52), UnaryFactor.K (unary_factor.py:19),
 * MultiMPPrior.get_const_vel_covariance (mp_priors_multi.py:170-202) and the precision->scale_tril
 * conversion torch performs on every MultiMPPrior.update_dist (mp_priors_multi.py:100-110).
 * sigma_goal < 0: not goal-directed.  qc_inv: HOST double[n*n] or NULL (= I/sigma_gp^2).
 * Synchronous (reads back the positive-definiteness flag): returns SGPMP_ENOTPD on failure. */
int sgpmp_set_prior(sgpmp_ctx* ctx, int which, double dt, double sigma_start, double sigma_gp,
                    double sigma_goal, const double* qc_inv, void* stream);
/* The two priors of StochGPMP.reset (planner.py:204-226: [0] initialisation, [1] sampling; isotropic Q_c) in one
 * call: K1 is a single wave for ~1.2 ms, so the two factorisations run concurrently (the second on a stream of the
 * context) and the call synchronises once.  sigma_goal[w] < 0: not goal-directed.  Same results and errors as two
 * sgpmp_set_prior calls. */
int sgpmp_set_priors(sgpmp_ctx* ctx, double dt, const double* sigma_start, const double* sigma_gp,
                     const double* sigma_goal, void* stream);

/* MultiMPPrior.set_Sigma_invs (mp_priors_multi.py:125-128): one precision matrix PER MODE, given by its
 * blocks -- D HOST double[n_modes][T][d][d] (diagonal blocks), E HOST double[n_modes][T-1][d][d] with
 * E[m][t] = Sigma_m^-1[t+1-block, t-block]; anything outside the block-tridiagonal band must be zero
 * (the caller checks).  K1 factors every mode (one workgroup each, fp64 MFMA); sgpmp_sample then uses
 * mode m's factor for mean m, sgpmp_prior_quadform its precision.  The planner loop: with which = SGPMP_PRIOR_SAMPLE and
 * n_modes = the context's particle count, sgpmp_step samples particle p from factor p (two-launch route: the dense sampler
 * on the matrix cores, then the sweep) while its importance-sampling term -- and sgpmp_is_weights -- keep the shared
 * closed-form precision of the last sgpmp_set_prior, exactly as the reference does after
 * planner._sample_dist.set_Sigma_invs(...) (planner.py:226,233-236: `self.Sigma_inv` is captured at reset).  A later
 * sgpmp_set_prior(s) returns to the shared factor.
 * Synchronous; SGPMP_ENOTPD when a matrix is not positive definite. */
int sgpmp_set_prior_blocks(sgpmp_ctx* ctx, int which, int n_modes, const double* D, const double* E,
                           void* stream);

/* MultiMPPrior.log_prob (mp_priors_multi.py:209-210 -> torch MultivariateNormal.log_prob): the quadratic
 * forms q_r = (x_r - mu_m)^T Sigma_m^-1 (x_r - mu_m), m = r % n_modes, for x DEVICE [rows, T*d] and
 * means DEVICE [n_modes, T*d] in ctx dtype -> out DEVICE double[rows]  (log_prob = -q/2 - M/2 log 2pi
 * + 1/2 log det Sigma_m^-1; the log-determinant is a by-product of K1's factor, see sgpmp_get_prior). */
int sgpmp_prior_quadform(sgpmp_ctx* ctx, int which, const void* x, int64_t rows, const void* means,
                         int n_modes, double* out, void* stream);

/* Test/inspection hook: copy K1's outputs to HOST buffers (any may be NULL). Synchronous.
 *   blocks  double[4*d*d]  D_0, D_interior, D_last, E = Sigma_inv[(i+1)-block, i-block]
 *   G, H    double[T*d*d]  scan coefficients:  y_t = G_t eps_t + H_t y_{t-1}  (= scale_tril @ eps);
 *           after sgpmp_set_prior_blocks: double[n_modes*T*d*d], and `blocks` are those of the shared prior of the
 *           last sgpmp_set_prior (what the step's importance-sampling term keeps using).
 *   G_t = B_t^-1 is lower triangular and Sigma^-1 = L_inv^T L_inv with diag blocks B_t, so
 *   log det Sigma^-1 = -2 sum_t sum_i log G_t[i][i]. */
int sgpmp_get_prior(sgpmp_ctx* ctx, int which, double* blocks, double* G, double* H);

/* CostComposite(cost_list, FK) compiled to a device cost program (cost_functions.py:34-58). */
int sgpmp_set_costs(sgpmp_ctx* ctx, const sgpmp_cost_desc* descs, int n_desc);
int sgpmp_set_fk(sgpmp_ctx* ctx, const sgpmp_joint* chain, int n_joints);
/* Any serial chain on the fast launches (the reference takes any FK callable, cost_functions.py:39,51-52).  The fused
 * sampler + sweep launch and the chunked sweep need the chain as straight-line, constant-folded code; the library is built
 * with that code for the Panda only.  For another chain the host generates `struct ChainCode_rt { ... };` with
 * stoch_gpmp_amd/csrc/gen/chain_codegen.py (gen_chain("rt", chain): the same generator that wrote the built-in code) and
 * hands the text over AFTER sgpmp_set_fk; the library compiles the same kernel sources around it with hiprtc for gfx950
 * (dlopen; lazily per sphere-field type; cached in memory and under $SGPMP_RTC_CACHE | ~/.cache/sgpmp), verifies the code
 * against the chain of sgpmp_set_fk (forward kinematics at random joint vectors, link and pair tables) and dispatches the chain
 * like the built-in one.  fp32 contexts, n_dof <= 7, revolute joints first.  On failure -- SGPMP_ESTATE: hiprtc or the
 * kernel sources (csrc/ next to the library, or $SGPMP_CSRC_DIR) unavailable; SGPMP_EINVAL: the code is not this chain's --
 * the chain keeps the slower run-time-constant kernels; nothing else changes.  sgpmp_set_fk resets it. */
int sgpmp_set_fk_codegen(sgpmp_ctx* ctx, const char* chain_struct_source);
/* *codegen_id: 0 run-time constants, 1 built-in code (Panda), 2 compiled at run time; seconds spent in hiprtc and the code
 * objects compiled / found in the disk cache for the current chain.  Any pointer may be NULL. */
int sgpmp_fk_codegen_info(sgpmp_ctx* ctx, int* codegen_id, double* compile_s, int* compiled, int* from_cache);
/* Compile-only check of chain code (hiprtc; no device, no context, nothing cached or loaded): SGPMP_OK and the size of the
 * gfx950 code object, or SGPMP_ESTATE with the compiler's log in sgpmp_last_error(). */
int sgpmp_fk_codegen_compile(const char* chain_struct_source, int field_type, int64_t* code_bytes);

/* ---- kernels ---------------------------------------------------------------------------------- */
/* K2. MultiMPPrior.sample (mp_priors_multi.py:204-207): out[m,s,:] = means[m,:] + scale_tril @ eps.
 * `n_modes` mean trajectories [n_modes,T,d], `n_samples` draws each -> out [n_modes,n_samples,T,d].
 * eps == NULL: counter-based Philox noise keyed by (seed, draw, mode_offset+m, s, element).
 * eps != NULL (parity mode): eps is laid out like torch's randn(n_samples, eps_modes, T*d)
 * (multivariate_normal.py:250-253) and mode m reads column eps_mode_offset + m. */
int sgpmp_sample(sgpmp_ctx* ctx, int which, uint64_t seed, uint64_t draw, const void* means,
                 int n_modes, int mode_offset, int n_samples, const void* eps, int eps_modes,
                 int eps_mode_offset, void* out, void* stream);

/* The noise itself: out[s][m][:] = the eps of sample s of mode m (global particle mode_offset + m) at draw `draw`, in the layout
 * of torch's randn(n_samples, n_modes, T*d) (multivariate_normal.py:250-253; element t*d + k: position noise of dof k at
 * waypoint t, t*d + n + k: its velocity noise) and the context's dtype -- exactly the values sgpmp_sample / sgpmp_step /
 * sgpmp_optimize draw for eps == NULL.  One counter-based stream serves fp32 and fp64 contexts (Philox4x32 + the fp32
 * Box-Muller, widened for fp64: csrc/rng.h), keyed on (seed, draw, global particle, sample, waypoint pair, dof).  What it is
 * for: feeding the SAME eps to the reference's algorithm (oracle/ref_equiv.py: TrajPrior.sample(eps=...)) -- the hardware's
 * log2 / sin / cos are approximations that a CPU restatement (oracle/native_noise.py) reproduces to an ulp of fp32, not bit
 * for bit.  The reference draws from torch's sequential generator and has no counterpart. */
int sgpmp_noise(sgpmp_ctx* ctx, uint64_t seed, uint64_t draw, int n_modes, int mode_offset, int n_samples, void* out,
                void* stream);

/* K3. CostComposite.eval (cost_functions.py:47-58): trajs [B,T,d] -> costs [B].
 * Row b of the batch is global row batch_offset + b (for CostGoalPrior's goal lookup).
 * spheres: DEVICE [n_spheres,4] (cx,cy,cz,r) in ctx dtype = observation['obstacle_spheres'].
 * is_weights: NULL, or DEVICE [B/rows_per_particle, T+1, d] importance-sampling weights (K5) whose
 * inner product with (x_0, e_0..e_{T-2}, x_{T-1}) is added (planner.py:233-236).
 * costs (ctx dtype) and costs64 (double) may each be NULL. */
int sgpmp_cost_eval(sgpmp_ctx* ctx, const void* trajs, int64_t batch, int64_t batch_offset,
                    const void* spheres, int n_spheres, const void* is_weights,
                    int rows_per_particle, void* costs, double* costs64, void* stream);

/* K5. Importance-sampling weights  a = temperature * blkdiag(K_s, Q^-1.., K_g) A mu  per particle
 * (the factored form of Sigma_inv @ mu, planner.py:226,235-236). out: DEVICE [P,T+1,d] ctx dtype. */
int sgpmp_is_weights(sgpmp_ctx* ctx, const void* means, int n_particles, double temperature,
                     void* out, void* stream);

/* K4. StochGPMP._update_distribution (planner.py:263-275): softmax(-costs/temperature) over S,
 * grad = sum_s w (x - mu), means += step_size * grad.  costs_dtype: SGPMP_F64 or the ctx dtype.
 * weights [P,S] and grad [P,T,d] in ctx dtype (may be NULL). means_prev [P,T,d] (may be NULL)
 * receives the PRE-update means, which is what optimize() returns (planner.py:252-253).
 * stats: DEVICE double[SGPMP_STAT_SHARDS][4] or NULL; each workgroup adds (sum of costs, min cost,
 * 1, -) of its particle to one shard -- the consumer sums the shards (sharding avoids serialising a
 * thousand atomics on one address). */
int sgpmp_update(sgpmp_ctx* ctx, const void* costs, int costs_dtype, const void* samples,
                 void* means, double temperature, double step_size, void* weights, void* grad,
                 void* means_prev, double* stats, void* stream);
/* Diagnostic (synchronous): the number of particles whose last update (inside sgpmp_step) spread its weight over more than
 * S / 4 samples.  For those the next step's fused launch leaves softmax partials of every 8 rows and the update adds S / 8
 * partials instead of re-reading the rows (planner.py:263-275 is a softmax; with the reference's hyper-parameters it is
 * one-hot and the count is 0).  -1: no fp32 step has run yet.  Which particles get partials is decided on the device, per
 * particle, from the row count its previous update left (stream-ordered: the same in every run; round 4 armed the partials
 * from a host word read without synchronisation).  *armed_steps (may be NULL): steps launched with the partials buffer so far. */
int sgpmp_dense_particles(sgpmp_ctx* ctx, int64_t* count, int64_t* armed_steps);
/* Those per-particle row counts are state of a run (they decide per particle how the NEXT update forms its sum -- gathered /
 * regenerated rows, or partials: equal to 1e-6, not bit for bit): StochGPMP.state_dict carries them, reset() clears them.
 * Synchronous.  get: out HOST uint32[P] (zeros before the first fp32 step); set: in HOST uint32[P], or NULL = all zero. */
int sgpmp_row_counts_get(sgpmp_ctx* ctx, uint32_t* out);
int sgpmp_row_counts_set(sgpmp_ctx* ctx, const uint32_t* in);
/* reset()'s clear (planner.py:181-227 starts a fresh problem): all zero, asynchronous on `stream`, no host synchronisation. */
int sgpmp_row_counts_clear(sgpmp_ctx* ctx, void* stream);
/* steps of this context that ran store-free so far (SGPMP_STEP_NO_SAMPLES honoured; tests and bench.py report it) */
long long sgpmp_store_free_steps(sgpmp_ctx* ctx);
/* launches of this context that ran SEVERAL iterations each (sgpmp_optimize, planar problems with 64 samples per particle) */
long long sgpmp_multi_iteration_launches(sgpmp_ctx* ctx);

/* One body of the loop at planner.py:289-299 for the context's particle shard:
 * K5 -> K2 -> K3 -> K4 on `stream` (K2 + K3 as ONE launch when the configuration qualifies, see
 * csrc/fused_step.inc; K5 folded into the previous step's K4 under SGPMP_STEP_MEANS_KEPT).  samples [P,S,T,d] is written (state_samples of the iteration);
 * costs [P,S] ctx dtype may be NULL. means updated in place. stats (DEVICE
 * double[SGPMP_STAT_SHARDS][4] or NULL) is zeroed at the start of the step and holds this step's
 * sharded sums afterwards; with a communicator attached (sgpmp_comm_init) the step also enqueues
 * their all-reduce on the side stream, so `stats` then holds the sums over ALL ranks once
 * sgpmp_stats_wait has been honoured. */
int sgpmp_step(sgpmp_ctx* ctx, uint64_t seed, uint64_t draw, const void* eps, int eps_modes,
               int eps_mode_offset, void* means, void* samples, void* costs, void* weights,
               void* grad, void* means_prev, const void* spheres, int n_spheres, double temperature,
               double step_size, double* stats, int flags, void* stream);
/* flags of sgpmp_step: */
#define SGPMP_STEP_MEANS_KEPT 1    /* the caller guarantees that `means` still holds exactly what this context's
                                      previous sgpmp_step left there: the importance-sampling weights that step's
                                      update kernel prepared for them are then used, and the K5 launch is skipped
                                      (on every path: the fused launch, or else the sampler, zeroes `stats`).
                                      Without the flag (or after anything else wrote the means) K5 runs. */
#define SGPMP_STEP_NO_SAMPLES 2    /* the caller will not read `samples` of THIS step (iterations 1 .. K - 1 of
                                      optimize(opt_iters = K): the reference returns the last iteration's tensors only,
                                      planner.py:289-317).  Where the step runs as one fused launch (fused_step_kernel,
                                      fused_planar_seg_kernel) it then does not write them -- 470 MB per launch at BASELINE
                                      configs[2] -- and update_kernel REGENERATES the rows that carry weight from their noise
                                      keys (one row per particle with the reference's one-hot weights), bit for bit what the
                                      launch would have stored: means, costs, weights, gradient come out identical to a
                                      storing step's.  (fused_planar_seg_kernel with 64 samples per particle: the workgroup
                                      holds all samples of its particle in registers and runs the update itself -- one
                                      launch per iteration, bit-identical to update_kernel.)  Rows of particles whose previous update spread its weight over more
                                      than 4 samples are still written (`samples` must be a valid buffer).  A permission,
                                      not a demand: steps on other paths store as always, and so do steps too small for the
                                      regeneration to pay (option store_free_min_bytes: below 2.8 MB of samples per waypoint a
                                      regenerating step measured 4 .. 20 % slower than a storing one).  After such a step
                                      `samples` holds rows of earlier steps. */

/* The loop of planner.py:289-299 itself (`for opt_step in range(opt_iters)`), when its iterations follow each
 * other without the caller looking at the buffers in between: bracket the sgpmp_step calls of one optimize() with
 *     sgpmp_pipeline_begin(ctx, stream);  K x sgpmp_step(..., stream);  sgpmp_pipeline_end(ctx, stream);
 * Particles are independent (every reduction of planner.py:263-275 runs over the samples of ONE particle), so
 * inside the bracket the context runs each step as TWO launch sequences, one per half of its particle range, on two
 * streams of its own: while one half's update kernel (latency-bound) runs, the other half's sampler + sweep launch
 * keeps the chip busy, across iterations.  Every buffer passed to the steps belongs to the context until
 * sgpmp_pipeline_end has returned, which makes `stream` wait for both sequences (stream-ordered like any other
 * call: no host synchronisation); results are those of unbracketed steps, bit for bit.  Steps that do not qualify
 * (not the fused launch, parity-mode noise, a communicator attached, fewer than 2 x 8192 trajectories) run as
 * usual inside the bracket.  Switch: SGPMP_NO_STEP_PIPELINE / "no_step_pipeline". */
int sgpmp_pipeline_begin(sgpmp_ctx* ctx, void* stream);
int sgpmp_pipeline_end(sgpmp_ctx* ctx, void* stream);
/* StochGPMP.optimize's loop (planner.py:289-299) as ONE call: opt_iters x sgpmp_step with in-kernel noise on `stream`,
 * draw counters draw0 .. draw0 + opt_iters - 1; step k accumulates its statistics in stats_pair[(first_slot + k) & 1]
 * (DEVICE double[2][SGPMP_STAT_SHARDS][4], or NULL); steps 0 .. K - 2 leave their pre-update means in means_prev_scratch,
 * the last one in means_prev_last (either may be NULL) -- the tensor optimize() hands out (planner.py:252-253).
 * flags: SGPMP_STEP_MEANS_KEPT speaks for the FIRST step (the later ones follow this call's own steps and always carry it);
 * SGPMP_OPT_STORE_FREE gives steps 0 .. K - 2 SGPMP_STEP_NO_SAMPLES (the reference returns the last iteration's tensors
 * only); SGPMP_OPT_PIPELINE brackets the call with sgpmp_pipeline_begin / _end when opt_iters >= 2.  Results are those of
 * the same sgpmp_step calls made one by one, bit for bit; the first failing step's status is returned (the bracket is
 * closed first).  No host synchronisation.
 * Under SGPMP_OPT_STORE_FREE, opt_iters >= 3, a planar problem with 64 samples per particle (n = 2, time segments of 8: the
 * store-free step carries its update inside the launch) runs steps 0 .. K - 2 as ONE launch (csrc/fused_planar_seg.inc:
 * PERSIST; not with a communicator, the step profiler or per-step mean statistics).  Every output is the same, bit for bit,
 * with one exception: the statistics of steps 0 .. K - 2 are not formed -- only the LAST step's slot of stats_pair,
 * (first_slot + K - 1) & 1, is written by such a call.  Option no_persist_planar. */
#define SGPMP_OPT_PIPELINE 4
#define SGPMP_OPT_STORE_FREE 8
int sgpmp_optimize(sgpmp_ctx* ctx, int opt_iters, uint64_t seed, uint64_t draw0, void* means, void* samples,
                   void* costs, void* weights, void* grad, void* means_prev_scratch, void* means_prev_last,
                   const void* spheres, int n_spheres, double temperature, double step_size,
                   double* stats_pair, int first_slot, int flags, void* stream);
/* Kernels the last sgpmp_step enqueued for its particle range (per chain when it ran as two): 2 = fused sampler + sweep,
 * then update_kernel (the default); 3-4 = separate kernels; 1 = a store-free planar step whose launch also updated its
 * particles (fused_planar_seg.inc: seg_update). */
int sgpmp_last_step_launches(sgpmp_ctx* ctx);
/* how many steps of this context ran as two chains so far (tests and bench.py report it) */
long long sgpmp_pipeline_split_steps(sgpmp_ctx* ctx);

/* ---- multi-GPU (one process per GPU; RCCL over xGMI) -------------------------------------------- */
/* The reference is single-process and has no counterpart; these calls carry out SURVEY.md 8(e):
 * particles are sharded by contiguous ranges (sgpmp_dims.particle_offset), the data path needs no
 * exchange, and the per-iteration statistics are summed over ranks.  librccl is loaded with dlopen
 * by the first of these calls; single-GPU users never need it.
 *
 * sgpmp_comm_unique_id: rank 0 obtains the 128-byte RCCL id and hands it to the other ranks by any
 *   host-side channel (the Python host uses torch.distributed's store).
 * sgpmp_comm_init: collective over all `world_size` ranks (ncclCommInitRank); attaches the
 *   communicator to the context.  From then on sgpmp_step all-reduces its `stats` by itself. */
int sgpmp_comm_unique_id(unsigned char* out128);
int sgpmp_comm_init(sgpmp_ctx* ctx, const unsigned char* id128, int world_size, int rank);
int sgpmp_comm_destroy(sgpmp_ctx* ctx);
/* What the attached communicator itself reports (ncclCommCount / ncclCommUserRank / ncclGetVersion), so that a
 * multi-GPU bench line can prove that RCCL saw N ranks: *world = 0 when no communicator is attached.
 * rccl_version: NCCL_VERSION_CODE of the loaded librccl (e.g. 22205), 0 if unavailable.  Any pointer may be NULL. */
int sgpmp_comm_info(sgpmp_ctx* ctx, int* world, int* rank, int* rccl_version);
/* Name of the collective library this process bound at its first sgpmp_comm_unique_id / sgpmp_comm_init ("" before):
 * "librccl.so.1" (or one of its fallback names) in the product library, always.  *test_hooks (may be NULL) = 1 only in
 * tests/fake_rccl/libsgpmp_testhooks.so, the build of comm.hip that honours SGPMP_RCCL_LIB (a stand-in that lets several
 * ranks share one GPU in the tests); the product library never reads that variable.  Static string. */
const char* sgpmp_comm_library(int* test_hooks);
/* Sum stats (DEVICE double[SGPMP_STAT_SHARDS][4], produced on `stream`) over all ranks, in place, on
 * the context's side stream: returns at once and never makes `stream` wait. (planner.py:668-672's
 * statistic over all particles of all GPUs.) */
int sgpmp_allreduce_stats(sgpmp_ctx* ctx, double* stats, void* stream);
/* Make `stream` wait (stream-side, not host-side) for the pending all-reduce of `stats`
 * (NULL: of every statistics buffer) -- call before reading or overwriting it. */
int sgpmp_stats_wait(sgpmp_ctx* ctx, double* stats, void* stream);
/* Per-goal statistics of the particle means -- the "weighted-mean / covariance statistics" of the trajectory
 * distribution's modes (a mode = the particles of one goal, p = g * nppg + k, planner.py:215); what a covariance
 * adaptation through MultiMPPrior.set_Sigma_invs (mp_priors_multi.py:125-128) or a mode summary consumes.
 * out DEVICE double[G][T*d + 1][2]:  [g][m] = (sum, sum of squares) of mu_p[m] over THIS context's particles of goal g,
 * [g][T*d] = (their number, 0).  sgpmp_mode_stats zeroes `out` and accumulates on `stream` (no atomics: bitwise
 * reproducible run to run for a given sharding; across shardings the additions are ordered differently -- equal to rounding).
 * sgpmp_allreduce_f64: sum any buffer of doubles over all ranks, in place, on the context's side stream (like
 * sgpmp_allreduce_stats; honour sgpmp_stats_wait(buf) before reading).
 * sgpmp_set_step_mode_stats(buf): from now on EVERY sgpmp_step produces them by itself, once per iteration: its update
 * kernel leaves a snapshot of the new means, the side stream reduces it per goal into `buf` and all-reduces the sums
 * over the ranks -- nothing is added to the steps' own stream but one event record; sgpmp_mode_stats_wait makes
 * `stream` wait for the newest one.  NULL switches it off.  (Steps then run as one chain and with update_kernel.) */
int sgpmp_mode_stats(sgpmp_ctx* ctx, const void* means, double* out, void* stream);
int sgpmp_allreduce_f64(sgpmp_ctx* ctx, double* buf, int64_t count, void* stream);
int sgpmp_set_step_mode_stats(sgpmp_ctx* ctx, double* buf);
int sgpmp_mode_stats_wait(sgpmp_ctx* ctx, void* stream);
/* All ranks' particle means: local [P_local,T,d] -> all [P_global,T,d] on every rank (ncclAllGather on
 * `stream`; equal shards only). */
int sgpmp_allgather_means(sgpmp_ctx* ctx, const void* local_means, void* all_means, void* stream);

/* ---- standalone field / FK ops (the planner <-> cost seam) ----------------------- */
/* FK callable: q [B,n] -> link frames [B,L,4,4], L = 1 + n_joints (cost_functions.py:51-52). */
int sgpmp_fk(sgpmp_ctx* ctx, const void* q, int64_t batch, void* frames, void* stream);
/* ObstacleMap.compute_cost (obst_map.py:164-185): X [B,2] -> values [B]; uses cost term `term`. */
int sgpmp_grid_lookup(sgpmp_ctx* ctx, int term, const void* xy, int64_t batch, void* out,
                      void* stream);
/* LinkDistanceField / LinkSelfDistanceField.compute_cost on explicit frames [B,L,4,4] -> [B]
 * using cost term `term` (its field type, margin, interpolation). */
int sgpmp_field_eval(sgpmp_ctx* ctx, int term, const void* frames, int64_t batch, int n_links,
                     const void* spheres, int n_spheres, void* out, void* stream);

/* LinkDistanceField.distances / compute_collision / compute_distance (fields.py:40-61; spheres DEVICE [n_spheres,4]:
 * D[l][o] = |p_l - c_o| - r_o) and LinkSelfDistanceField's (fields.py:100-112; spheres NULL: D[i][j] = |p_i - p_j|)
 * on link frames [B,L,4,4] in ctx dtype.  mode 0: out [B,L,n_spheres or L] = D;  mode 1: out [B] = 1 where any
 * D < buffer (self: over link pairs i - j >= 2, torch.tril(.., diagonal=-2)), else 0;  mode 2: out [B] = sum D. */
int sgpmp_link_distances(sgpmp_ctx* ctx, const void* frames, int64_t batch, int n_links, const void* spheres,
                         int n_spheres, int mode, double buffer, void* out, void* stream);

/* FieldFactor.get_error(calc_jacobian=True) (factors/field_factor.py:28-38): value [B] (may be NULL) and
 * gradient d value / d q [B,n] of link-field term `term` at joint configurations q [B,n], with the
 * context's FK chain -- the analytic form of the reference's torch.autograd.grad through FK and the
 * field (the reference's H is MINUS this gradient).  SPHERES with the rbf type; SPHERES with the sdf type
 * (fields.py:79-83: value = max over (link point, sphere) of r - dist, optionally clamped at 0; gradient = that of
 * the arg-max pair, first maximum in (point, sphere) order as torch's max keeps it, zero where the clamp is
 * active -- what autograd returns through sdf.max(-1)[0].max(-1)[0]); SELF; EE_GOAL (end-effector SE(3) distance:
 * position part u . (z_j x (p - o_j)), rotation part z_j . axis; what CostGoal.get_linear_system needs,
 * cost_functions.py:323-337).  The occupancy count has no gradient -> SGPMP_EINVAL.   */
int sgpmp_field_grad(sgpmp_ctx* ctx, int term, const void* q, int64_t batch, const void* spheres,
                     int n_spheres, void* value, void* grad, void* stream);

/* ---- dense trajectories: GP interpolation between the support waypoints, and a check of ALL fine states ---- */
/* No reference counterpart: the reference evaluates every collision term at the T support waypoints only (cost_functions.py:
 * 247-261) and has no joint or velocity limits.  The interpolant is the one the planner's own prior implies: the posterior mean
 * of the constant-velocity GP between two support states, x(tau) = Lambda(tau) x_i + Psi(tau) x_{i+1} (the GPMP "GP
 * interpolation"); for this prior Q_c and the prior mean cancel and the result is the cubic Hermite spline on (q, q'), so only
 * `dt` is needed.  n_sub = k >= 0 points are inserted per interval: T_f = (T - 1)(k + 1) + 1 fine states, fine index
 * f = i (k + 1) + m at s = m / (k + 1) of interval i; support states (m = 0, and f = T_f - 1) are copied, not computed.  Both
 * entry points evaluate the fine states with the same device function (csrc/traj_dense.hip: hermite_state), bit for bit. */
#define SGPMP_MAX_SUBSTEPS 31

/* ---- signed-distance grid field (SGPMP_COST_GRID_SDF) -------------------------------------------
 * A smooth collision field for planar map scenes: the occupancy grid's exact Euclidean signed distance, interpolated
 * bilinearly, under the GPMP hinge.  No reference counterpart (its ObstacleMap is occupancy only).
 *
 * sgpmp_grid_sdf_build: occ [ny, nx] (DEVICE, ctx dtype; a cell is occupied when (double)occ > threshold) -> sdf [ny, nx]
 * (DEVICE, ctx dtype), the signed distance at cell centres in world units.  For a free cell a, D(a) = min over occupied cells b
 * of the Euclidean distance between the index pairs and sdf = (D - 0.5) * cell; for an occupied cell D is taken over the free
 * cells and sdf = -(D - 0.5) * cell: the zero level sits on cell edges.  Exact: squared distances are integers, one correctly
 * rounded square root in double, then the subtract and the multiply in that order, then the conversion to the ctx dtype.  A map
 * with no occupied cell gives +cap everywhere, one with no free cell -cap, cap = cell * (nx + ny); never infinite.
 * 1 <= nx, ny <= 4096 and cell > 0, else SGPMP_EINVAL (before any launch).  Stream-ordered, two launches, no host copy of the
 * map, no allocation; occ and sdf must not overlap.
 *
 * The term: sgpmp_cost_desc { kind = SGPMP_COST_GRID_SDF, data = sdf, dim0 = ny, dim1 = nx, p0 = cell, p1, p2 = the offsets
 * (ox, oy) of SGPMP_COST_GRID, sigma -> K = 1 / sigma^2, sigma2 = margin >= 0 }; needs n_dof >= 2, the point is (q[0], q[1]).
 *   u = x * (1 / cell) + ox - 0.5, v = y * (1 / cell) + oy - 0.5   (multiply and add rounded separately, as the GRID lookup)
 *   i0 = floor(u), fx = u - i0, j0 = floor(v), fy = v - j0; i0, i0 + 1 clamped to [0, nx - 1], j0, j0 + 1 to [0, ny - 1]
 *   d = (1 - fy) ((1 - fx) s00 + fx s10) + fy ((1 - fx) s01 + fx s11),  s[j][i] = sdf[j * nx + i]
 *   field h = margin - d where that is > 0, else 0;  dh/d(x, y) = -(dd/dx, dd/dy) where h > 0, exactly 0 elsewhere,
 *   dd/dx = ((1 - fy)(s10 - s00) + fy (s11 - s01)) * (1 / cell),  dd/dy = ((1 - fx)(s01 - s00) + fx (s11 - s10)) * (1 / cell)
 *   (the reciprocal the first operation multiplies by: not a division).
 * x is clamped by the x extent (dim1) and y by the y extent (dim0): the GRID lookup's reference-inherited clamp of x by dim0 is
 * NOT copied.  Outside the map the clamp makes the derivative in that direction zero.  A non-finite x or y gives NaN in the
 * value and in the gradient.
 * In a cost list the term is K * sum over t = 1 .. T-1 of h(q_t[0], q_t[1]) (SGPMP_COST_GRID's range) in sgpmp_cost_eval /
 * sgpmp_step (sampler + generic sweep + update: no fused launch takes it), one of the collision terms of sgpmp_dense_cost and
 * sgpmp_dense_cost_grad (differentiable; not together with link-field terms in the gradient: SGPMP_EINVAL), a field of
 * sgpmp_field_grad (no FK chain needed: q [B, n] -> value [B], grad [B, n], entries >= 2 zero; SGPMP_ESTATE in a build without
 * the kernel) and one of the four field slots of sgpmp_gpmp_linearize (one row per waypoint 1 .. T-1, error h, precision K,
 * A = -dh/dq on entries 0 and 1; with sgpmp_gpmp_set_dense on the fine states).  sgpmp_validate's occupancy column still needs
 * a SGPMP_COST_GRID term. */
int sgpmp_grid_sdf_build(sgpmp_ctx* ctx, const void* occ, int ny, int nx, double cell, double threshold, void* sdf,
                         void* stream);

/* ---- voxel signed-distance field (SGPMP_COST_VOXEL_SDF) -----------------------------------------
 * The 3-D counterpart of the grid field above, for arm scenes: an occupancy volume's exact Euclidean signed distance,
 * interpolated trilinearly, under the GPMP hinge, summed over the link points of the FK chain.  No reference counterpart.
 *
 * sgpmp_voxel_sdf_build: occ [nz, ny, nx] (x fastest; DEVICE, ctx dtype; a cell is occupied when (double)occ > threshold) ->
 * sdf [nz, ny, nx] (DEVICE, ctx dtype), the signed distance at cell centres in world units, by sgpmp_grid_sdf_build's
 * convention: for a free cell D^2 = min over occupied cells of the squared distance between the index triples and
 * sdf = (sqrt(D^2) - 0.5) * cell, for an occupied cell the same over the free cells, negated.  Exact: squared distances are
 * integers (<= 3 * 511^2, exact in fp32), one correctly rounded square root in double, then the subtract, the multiply, the
 * conversion to the ctx dtype.  No occupied cell: +cap everywhere; no free cell: -cap; cap = cell * (nx + ny + nz); never
 * infinite.  1 <= nx, ny, nz <= 512, cell > 0, a threshold that is not NaN, non-null occ != sdf: else SGPMP_EINVAL before any
 * launch.  Stream-ordered, three launches (along z, y, x), IN PLACE in sdf: no scratch volume, no allocation, no host copy
 * (the y pass stages a [ny][32] tile, <= 64 KiB, the x pass a row in LDS).
 *
 * The term: sgpmp_cost_desc { kind = SGPMP_COST_VOXEL_SDF, data = sdf, reserved = nz, dim0 = ny, dim1 = nx, p0 = cell,
 * p1 = ox, p2 = oy, dt = oz, sigma -> K = 1 / sigma^2, sigma2 = margin >= 0, num_interpolate / interp_lo / interp_hi / alpha as
 * for SGPMP_COST_SPHERES }.  (dt and reserved are fields no other link field uses: the struct's layout does not move.)  The
 * points p are those of SGPMP_COST_SPHERES: every link origin of the chain, then the interpolated points.  Per point
 *   u = px * (1 / cell) + ox - 0.5, v = py * (1 / cell) + oy - 0.5, w = pz * (1 / cell) + oz - 0.5   (multiply, add: rounded separately)
 *   i0 = floor(u), fx = u - i0; i0, i0 + 1 clamped to [0, nx - 1]; j0, fy from v and ny, k0, fz from w and nz likewise
 *   s[k][j][i] = sdf[(k * ny + j) * nx + i];  trilinear, x first, then y, then z:
 *   c_kj = (1 - fx) s[k][j][i0] + fx s[k][j][i1];  e_k = (1 - fy) c_k,j0 + fy c_k,j1;  d = (1 - fz) e_k0 + fz e_k1
 *   dd/dx = ((1 - fz) ((1 - fy) (s[k0][j0][i1] - s[k0][j0][i0]) + fy (s[k0][j1][i1] - s[k0][j1][i0]))
 *            + fz ((1 - fy) (s[k1][j0][i1] - s[k1][j0][i0]) + fy (s[k1][j1][i1] - s[k1][j1][i0]))) * (1 / cell)
 *   dd/dy = ((1 - fz) (c_k0,j1 - c_k0,j0) + fz (c_k1,j1 - c_k1,j0)) * (1 / cell),  dd/dz = (e_k1 - e_k0) * (1 / cell)
 *   h_p = margin - d where that is > 0, else 0;  dh_p/dp = -grad d where h_p > 0, exactly 0 elsewhere.
 * A clamped axis (outside the volume) has a zero derivative; a non-finite coordinate gives NaN in the value and the gradient.
 * The field is f(q) = sum over the points of h_p; in a cost list the term is K * sum over t = 1 .. T-1 of f(q_t).  It needs an
 * FK chain (SGPMP_ESTATE without one).  Consumers: sgpmp_cost_eval / sgpmp_step (sampler + generic sweep + update: no fused
 * launch takes it), sgpmp_field_eval on explicit frames, sgpmp_field_grad, and one of the four field slots of
 * sgpmp_gpmp_linearize (with and without sgpmp_gpmp_set_dense).  With SGPMP_FLAG_GRID_DISTANCE sgpmp_field_grad returns
 * min over the points of d and the gradient through the FIRST arg-min point (point order, strict comparison): a query, allowed
 * only as the cost list's single term (else SGPMP_EINVAL) and refused by GPMP.  sgpmp_dense_cost, sgpmp_dense_cost_grad and
 * sgpmp_validate refuse a cost list that holds the term (SGPMP_EINVAL): their kernels do not evaluate it. */
int sgpmp_voxel_sdf_build(sgpmp_ctx* ctx, const void* occ, int nz, int ny, int nx, double cell, double threshold, void* sdf,
                          void* stream);

/* ---- body collision spheres on the voxel field (SGPMP_COST_BODY_SDF) -----------------------------
 * The robot side of the voxel field above: instead of the link origins, the term evaluates a BODY, a table of M spheres fixed in
 * the link frames, 1 <= M <= SGPMP_MAX_BODY.  Sphere m has a link index l_m, a centre c_m in that link's frame and a radius
 * r_m >= 0.  Link frames are sgpmp_fk's: frame 0 is the base, frame j + 1 follows joint j, its rotation included, so
 * 0 <= l_m <= n_joints.  No reference counterpart.
 *
 * sgpmp_set_body: links HOST int32[n] in non-decreasing order, spheres HOST double[n][4] = (cx, cy, cz, r); uploaded in the ctx
 * dtype; one body per context; n = 0 clears it.  SGPMP_EINVAL: n outside [0, 64], a null table with n > 0, links not in
 * non-decreasing order, a negative or non-finite radius, a non-finite centre, a link index past the chain's last frame;
 * SGPMP_ESTATE: no FK chain.  A later sgpmp_set_fk clears the body.  Synchronous.
 *
 * The term: sgpmp_cost_desc packed exactly as SGPMP_COST_VOXEL_SDF's (data = sdf volume, reserved / dim0 / dim1 = nz / ny / nx,
 * p0 / p1 / p2 / dt = cell and the three offsets, sigma -> K = 1 / sigma^2, sigma2 = margin >= 0); num_interpolate must be 0
 * (SGPMP_EINVAL).  With (R_l, P_l) the frame of link l at configuration q and d(.) the trilinear signed distance of
 * SGPMP_COST_VOXEL_SDF (the same device function, the same clamping, the same NaN rule):
 *   p_m(q) = P_l + R_l c_m                       world centre
 *   s_m = d(p_m) - r_m                           clearance
 *   h_m = (margin + r_m) - d(p_m) where that is > 0, else 0      (the hinge on margin - s_m)
 *   f(q) = sum over m of h_m, in table order;  the term in a cost list is K * sum over t = 1 .. T-1 of f(q_t).
 * Gradient, with g_m = dh_m/dp (-grad d where h_m > 0, exactly 0 elsewhere): df/dq_j = sum over the spheres on links behind
 * revolute joint j of z_j . ((p_m - o_j) x g_m) -- sgpmp_field_grad's recurrence z_j . (M_j - o_j x F_j), which holds for any point
 * rigidly attached behind the joint.  Spheres on link 0 contribute to the value and never to the gradient.  A non-finite
 * coordinate of a sphere centre gives NaN in the value and in EVERY gradient entry.
 * A program that holds the term without a body fails with SGPMP_ESTATE and a message that names sgpmp_set_body, whatever the
 * call order (the body may be set before or after sgpmp_set_costs).
 * Consumers: sgpmp_cost_eval / sgpmp_step / sgpmp_optimize (sampler + generic sweep + body_cost_kernel + update: the sweep skips
 * the term, body_cost_kernel adds it to the costs behind it on the same stream -- one wave per trajectory, lane = waypoint, one
 * writer per cost element, no atomics; no fused launch takes the term), sgpmp_field_eval on explicit frames [B, L, 4, 4] (the
 * frames carry the rotations; L must exceed the body's last link index), sgpmp_field_grad, and one of the four field slots of
 * sgpmp_gpmp_linearize (with and without sgpmp_gpmp_set_dense).  With SGPMP_FLAG_GRID_DISTANCE sgpmp_field_grad returns
 * min over m of s_m and the gradient through the FIRST arg-min sphere (table order, strict comparison): a query, allowed only as
 * the cost list's single term (else SGPMP_EINVAL) and refused by GPMP.  sgpmp_dense_cost, sgpmp_dense_cost_grad and
 * sgpmp_validate refuse a cost list that holds the term (SGPMP_EINVAL): their kernels do not evaluate it.  SGPMP_ESTATE from
 * sgpmp_set_costs in a build without the kernels (csrc/body_sdf.hip). */
int sgpmp_set_body(sgpmp_ctx* ctx, const int32_t* links, const double* spheres, int n);

/* ---- body self-collision: sphere pairs with radii and an allowed-pair mask (SGPMP_COST_BODY_SELF) --
 * The other half of the body above: the body's spheres against each other.  The term uses the context's body of sgpmp_set_body,
 * p_m(q) = P_l + R_l c_m with radius r_m, and a set of COUNTED pairs -- which spheres can touch is the caller's knowledge (an
 * ignore list, as in GPMP2, CHOMP and cuRobo).  No reference counterpart (SGPMP_COST_SELF is a Gaussian of the distances between
 * link origins over all link pairs).
 *
 * sgpmp_set_body_pairs: rows HOST uint64[n]; bit j of rows[i] set means pair (i, j) is counted; only bits j > i are read.  n must
 * equal the body's sphere count; n = 0 clears the pairs.  SGPMP_EINVAL: n not equal to the body's count, a null table with n > 0,
 * a bit j >= n, a counted pair with both spheres on one link (a constant, almost certainly a mistake), no counted pair at all;
 * SGPMP_ESTATE: no body.  sgpmp_set_body and sgpmp_set_fk clear the pairs.  Synchronous: the rows are uploaded once to a device
 * table beside the body's, which the kernels read through the constant address space, wave-uniform.
 *
 * The term: sgpmp_cost_desc with sigma -> K = 1 / sigma^2, sigma2 = margin >= 0, data null; num_interpolate must be 0
 * (SGPMP_EINVAL).  For a counted pair (i, j), i < j in table order:
 *   D_ij = |p_i - p_j|
 *   s_ij = D_ij - r_i - r_j                         clearance
 *   h_ij = (margin + r_i + r_j) - D_ij  where that is > 0, else 0
 *   f(q) = sum of h_ij over the counted pairs, i ascending, then j ascending;
 *   the term in a cost list is K * sum over t = 1 .. T-1 of f(q_t).
 * Gradient: dh_ij/dp_i = -(p_i - p_j) / D_ij where h_ij > 0, and dh_ij/dp_j is its negative; exactly 0 where h_ij = 0, and exactly 0
 * where D_ij = 0 (the value there is margin + r_i + r_j: no NaN, no division).  df/dq follows by the body term's recurrence,
 * z_k . ((p - o_k) x g) for every joint k in front of the sphere's link; for a joint in front of both spheres the two forces cancel
 * (g is parallel to p_i - p_j), so only the joints between the two links act, and a pair behind fixed joints only has a gradient of
 * exactly 0.  A non-finite coordinate of any counted sphere centre gives NaN in the value and in EVERY gradient entry.
 * A program that holds the term without a chain, a body and pairs fails with SGPMP_ESTATE and a message that names
 * sgpmp_set_body_pairs, whatever the call order.
 * Consumers: sgpmp_cost_eval / sgpmp_step / sgpmp_optimize (sampler + generic sweep + body_self_cost_kernel + update: the sweep
 * skips the term, body_self_cost_kernel adds it to the costs behind it -- and behind body_cost_kernel where both terms are present,
 * in program order -- one wave per trajectory, lane = waypoint, one writer per cost element, no atomics, two calls give the same
 * bits; no fused launch takes the term), sgpmp_field_eval on explicit frames [B, L, 4, 4] (L must exceed the body's last link
 * index), sgpmp_field_grad, and one of the four field slots of sgpmp_gpmp_linearize (with and without sgpmp_gpmp_set_dense).  With
 * SGPMP_FLAG_GRID_DISTANCE sgpmp_field_grad returns min over the counted pairs of s_ij and the gradient through the FIRST arg-min
 * pair (summation order, strict comparison): a query, allowed only as the cost list's single term (else SGPMP_EINVAL) and refused
 * by GPMP.  sgpmp_dense_cost, sgpmp_dense_cost_grad and sgpmp_validate refuse a cost list that holds the term (SGPMP_EINVAL):
 * their kernels do not evaluate it.  SGPMP_ESTATE from sgpmp_set_costs in a build without the kernels (csrc/body_self.hip). */
int sgpmp_set_body_pairs(sgpmp_ctx* ctx, const uint64_t* rows, int n);

/* trajs [B,T,d] -> out [B,T_f,d], ctx dtype, T = dims.traj_len. */
int sgpmp_interpolate(sgpmp_ctx* ctx, const void* trajs, int64_t batch, int n_sub, double dt, void* out, void* stream);
/* Per trajectory, over ALL T_f fine states (never written to memory): values [B,4] ctx dtype, where [B,4] int32 = the first fine
 * index attaining each value (ties go to the lowest f).
 *   [0] c_obs   min over f, links l, spheres o of |p_l(q_f) - c_o| - r_o   (the D of sgpmp_link_distances; needs sgpmp_set_fk and spheres)
 *   [1] c_self  min over f and link pairs i - j >= 2 whose distance depends on q of |p_i - p_j|   (needs sgpmp_set_fk; rigid and
 *               coincident pairs are left out: with them the minimum is a constant of the chain)
 *   [2] e_lim   max over f, dof k of max(q_lo[k] - q, q - q_hi[k], |q'| - v_max[k]), over whichever limits are given
 *   [3] g_occ   max over f of the grid value of cost term `grid_term` at (q_f0, q_f1)   (sgpmp_grid_lookup's value)
 * A column whose inputs are absent reports +inf ([0], [1]) or -inf ([2], [3]) with where = -1.  A trajectory with any non-finite
 * fine state reports NaN in all four columns and the first non-finite fine index in all four `where`.
 * SGPMP_EINVAL: n_sub outside [0, SGPMP_MAX_SUBSTEPS], dt <= 0, a null buffer with batch > 0, grid_term >= 0 that is not a GRID
 * term; SGPMP_ESTATE: spheres without a chain. */
int sgpmp_validate(sgpmp_ctx* ctx, const void* trajs, int64_t batch, int n_sub, double dt,
                   const void* spheres, int n_spheres,      /* DEVICE [n,4] or NULL          */
                   int grid_term,                           /* index of a GRID cost term, -1 */
                   const double* q_lo, const double* q_hi,  /* HOST [n_dof] or NULL          */
                   const double* v_max,                     /* HOST [n_dof] or NULL          */
                   void* values, int32_t* where, void* stream);

/* Continuous-time collision and limit cost of trajs [B,T,d] on the fine states of sgpmp_interpolate (same device function, same
 * bits), per trajectory b:
 *   dense[b] = weight * sum over the INSERTED states (m = 1 .. n_sub of every interval) of sum over the GRID / SPHERES / SELF terms
 *                       of the cost program of K_term * field_term(x_f)
 *            + 1/sigma_limit^2 * sum over ALL fine states f and dof k of
 *                       max(0, q_lo[k] - q)^2 + max(0, q - q_hi[k])^2 + max(0, |q'| - v_max[k])^2
 * The support states' collision cost stays with the sweep: sgpmp_cost_eval + sgpmp_dense_cost counts every fine state once.  The
 * fields are the sweep's own (grid value at (q_0, q_1); rbf / sdf / clamped sdf / occupancy sphere fields with a term's
 * interpolated link points; the full L x L self field); GP, goal-prior and end-effector terms are ignored, and so is the option
 * f64_fields_f32.  A limit that is not given (NULL; one side of q_lo / q_hi alone is allowed) contributes nothing; a SPHERES term
 * with n_spheres = 0 contributes nothing; weight = 0 leaves the limit part.  A trajectory with any non-finite fine state reports
 * NaN.  accumulate = 0 writes, 1 adds to what the outputs hold (both given: costs64 is the accumulator, costs its rounding);
 * each lane sums its interval in the ctx dtype, the sum over the lanes and the add are in double.
 * Chains the library was built with (Panda, no interpolated link points) run register-resident generated code, every other
 * chain the generic forward kinematics through LDS; sgpmp_last_dense_kernel names the kernel of this thread's last launch.
 * SGPMP_EINVAL: n_sub outside [0, SGPMP_MAX_SUBSTEPS], dt <= 0, weight < 0, a limit with sigma_limit <= 0, and with batch > 0 a
 * null trajs or both outputs null; SGPMP_ESTATE: a SPHERES / SELF term without a chain, a SPHERES term with n_spheres > 0 and
 * spheres NULL.  batch = 0 is a no-op. */
int sgpmp_dense_cost(sgpmp_ctx* ctx, const void* trajs, int64_t batch, int n_sub, double dt,
                     const void* spheres, int n_spheres,          /* DEVICE [n,4] or NULL */
                     double weight,                               /* scales the collision part */
                     const double* q_lo, const double* q_hi,      /* HOST [n_dof] or NULL */
                     const double* v_max, double sigma_limit,     /* HOST [n_dof] or NULL; > 0 when any limit is given */
                     int accumulate,                              /* 0: write, 1: add to what is there */
                     void* costs, double* costs64,                /* [B] ctx dtype / double; either may be NULL */
                     void* stream);
const char* sgpmp_last_dense_kernel(void);   /* thread-local static name of the kernel the last call launched; "" before */

/* Value and gradient of the continuous-time cost with respect to the SUPPORT states, per trajectory b:
 *   J[b]    = sgpmp_dense_cost's dense[b] (weight x the GRID / SPHERES / SELF terms on the inserted states + the limit penalty on all
 *             fine states), and with support = 1 also weight x the SPHERES / SELF terms at the support waypoints 1 .. T-1 (the range
 *             of CostCollision and sgpmp_field_grad);
 *   grad[b] = d J[b] / d trajs[b], all T x 2n entries, velocities included.
 * The fine states are hermite_state's (the bits sgpmp_interpolate writes).  Per fine state: forward kinematics that keeps the joint
 * axes, the forces d field / d p_l on the link points (a term's interpolated points hand theirs to the two links they lie between),
 * sgpmp_field_grad's backward recurrence d f / d q_j = z_j . (M_j - o_j x F_j), the limit penalty's derivative 2/sigma_limit^2 x
 * the signed excess (C^1: zero where no limit is exceeded), and the transpose of the eight Hermite coefficients that formed the
 * state onto x_i and x_{i+1} (m = 0: the identity).  The rbf sphere field and the SELF field are smooth; the sdf field (clamped or
 * not) follows sgpmp_field_grad's rule: the gradient of the arg-max (point, sphere) pair, first maximum in point-major order,
 * exactly zero where the clamp is active.
 * Never a silently zero gradient: a GRID term (with n_sub > 0) or a SPHERES term of the occupancy type (n_spheres > 0, n_sub > 0 or
 * support) is piecewise constant; with weight > 0 the call is refused, SGPMP_EINVAL.  weight = 0 (the limit part alone) is always
 * allowed.  A trajectory with any non-finite fine state reports NaN in its value and in every element of grad[b], also under
 * accumulate.  accumulate = 0 writes grad, 1 adds to what it holds; the values are always written.  Every element of grad is written
 * once, by one lane, without atomics: two calls on the same inputs return the same bits.
 * Link points, forces and joint axes live in one LDS column per lane: the forces of the L links in double in either dtype (their
 * sums cancel), points and axes in the ctx dtype, L x 3 x 64 x 8 + (2 L - 1) x 3 x 64 x sizeof(real) bytes whatever the number of
 * interpolated points (Panda: 32 KB fp32, 48 KB fp64); a chain that needs more than 64 KB is refused, SGPMP_EINVAL, with
 * the computed bound in the message.  sgpmp_last_dense_kernel names the kernel: "dense_cost_grad_kernel<f32, 10 joints>" (chain
 * lengths 10 and 7 with n_dof 7 and no interpolated points are compiled in), "... generic>", "... no FK>".
 * SGPMP_EINVAL: sgpmp_dense_cost's argument errors, and a null grad with batch > 0; SGPMP_ESTATE as sgpmp_dense_cost.  batch = 0 is
 * a no-op. */
int sgpmp_dense_cost_grad(sgpmp_ctx* ctx, const void* trajs, int64_t batch, int n_sub, double dt,
                          const void* spheres, int n_spheres,          /* DEVICE [n,4] or NULL */
                          double weight,                               /* scales the collision part */
                          const double* q_lo, const double* q_hi,      /* HOST [n_dof] or NULL */
                          const double* v_max, double sigma_limit,     /* HOST [n_dof] or NULL; > 0 when any limit is given */
                          int support,                                 /* 1: the collision terms also on support waypoints 1 .. T-1 */
                          int accumulate,                              /* 0: write grad, 1: add to what grad holds */
                          void* grad,                                  /* [B,T,d] ctx dtype, required when batch > 0 */
                          void* costs, double* costs64,                /* [B] value, either or both may be NULL */
                          void* stream);

/* ---- GPMP: the reference's Gauss-Newton planner (planner.py:352-661) ------- */
/* First half of GPMP._step (planner.py:580-581, cost.get_linear_system): evaluates every smooth link
 * field of the cost list and its Jacobian at waypoints 1..T-1 of the particle means [P,T,d] (kept in
 * the context), and -- when `diag_sum` [T*d] is given -- the sum over THIS context's particles of the
 * field part of diag(A^T K A), which the trust-region damping averages over all particles
 * (planner.py:618-622; all-reduce it across ranks before sgpmp_gpmp_solve when particles are sharded).
 * The cost list may hold one CostGP, one CostGoalPrior and up to 4 rbf- or sdf-sphere / self-distance /
 * end-effector-goal fields (CostGoal: one row, on the last waypoint). */
int sgpmp_gpmp_linearize(sgpmp_ctx* ctx, const void* means, const void* spheres, int n_spheres,
                         double* diag_sum, void* stream);
/* Second half (planner.py:583-603): per particle, assemble the block-tridiagonal normal equations
 * (A^T K A + damping) d_theta = A^T K b, solve them by block Cholesky, means += step_size * d_theta.
 * diag_sum NULL: damping delta * I (trust_region=False); else delta * diag(mean_p A^T K A).
 * d_theta [P,T,d] and costs [P] (= b^T K b at the linearisation point, planner.py:642-644) may be NULL.
 * Synchronous; SGPMP_ENOTPD if a pivot is not positive (torch raises from cholesky in the reference). */
int sgpmp_gpmp_solve(sgpmp_ctx* ctx, void* means, const double* diag_sum, double delta, double step_size,
                     void* d_theta, void* costs, void* stream);

/* Continuous-time factors in that linear system (no reference counterpart: the reference's GPMP has rows at the T support
 * waypoints only).  With n_sub = k states inserted per interval by the interpolation of sgpmp_interpolate (fine state m of
 * interval i: x_f = Lambda[m] x_i + Psi[m] x_{i+1}), sgpmp_gpmp_linearize / sgpmp_gpmp_solve add, all as scalar rows
 * (A row = -d error / d x, b = error):
 *   - for every SPHERES (rbf, sdf, clamped sdf) and SELF term, at every inserted state m = 1 .. k of every interval, the row
 *     error = field_term(q_f), precision = weight x K_term, entries -(Lambda[m][0][0], Lambda[m][0][1]) g on (q_i, q'_i) and
 *     -(Psi[m][0][0], Psi[m][0][1]) g on (q_{i+1}, q'_{i+1}), g = d field / d q_f as sgpmp_field_grad returns it.  The support
 *     waypoints 1 .. T-1 keep their rows with K_term, an EE_GOAL term its one row on the last waypoint;
 *   - per degree of freedom at ALL fine states the limit rows max(0, q_lo - q), max(0, q - q_hi), max(0, |q'| - v_max) with
 *     precision 1/sigma_limit^2 (b^T K b of them is sgpmp_dense_cost's limit penalty); an inactive row is a zero row, a limit
 *     that is not given (NULL; one side alone is allowed) contributes nothing.
 * The normal matrix stays block-tridiagonal with a per-interval sub-diagonal block: sgpmp_gpmp_solve then runs
 * gpmp_dense_solve_kernel (csrc/gpmp_dense.hip), `costs` counts the new rows, and `diag_sum` of sgpmp_gpmp_linearize carries
 * their part of diag(A^T K A) -- velocity entries and waypoint 0 included.  q_lo, q_hi, v_max: HOST double[n_dof], copied.
 * n_sub = 0 or weight = 0 with no limit given switches the option OFF: linearize and solve are then those without it, bit for
 * bit.  A change of the setting takes effect at the next sgpmp_gpmp_linearize (a solve in between: SGPMP_ESTATE).
 * SGPMP_EINVAL: n_sub outside [0, SGPMP_MAX_SUBSTEPS], dt <= 0, weight < 0, a limit with sigma_limit <= 0. */
int sgpmp_gpmp_set_dense(sgpmp_ctx* ctx, int n_sub, double dt, double weight, const double* q_lo, const double* q_hi,
                         const double* v_max, double sigma_limit);
/* Name of the solve kernel of this thread's last sgpmp_gpmp_solve ("gpmp_thomas_kernel", "gpmp_solve_kernel",
 * "gpmp_dense_solve_kernel"; "" before): for the tests that must prove which kernel they exercised.  Static string. */
const char* sgpmp_last_gpmp_kernel(void);
/* Particles per wave of that solve: 4 or 2 after "gpmp_thomas_kernel" (four while 4 x 8 T (32 + 9 F) bytes of staging, F the number
 * of link-field terms, fit 150 KiB of LDS; else two), 0 after the other two kernels and before the first solve. */
int sgpmp_last_gpmp_ppw(void);
/* Kernel and launch parameters of the sampler launch this thread last enqueued (sgpmp_sample, and the sampler launch of a step
 * that is not fused): "sample_iso_kernel<VW=2>" or "<VW=4>" (store width in elements), "sample_iso_small_kernel<NC=7,spb=8,tc=64>"
 * (compiled-in dof count or 0, samples per workgroup, waypoints per chunk), "sample_dense_kernel", with "(per-mode)" appended
 * when each mode has factors of its own (sgpmp_set_prior_blocks); "" before the first.  For the tests that must prove which
 * branch of the dispatch they exercised.  Valid until this thread's next call of this function. */
const char* sgpmp_last_sample_kernel(void);

/* Kernel timing helper for bench.py: elapsed ms between two events recorded on `stream`
 * (HIP events on the stream the kernels run on). */
int sgpmp_event_create(void** ev);
int sgpmp_event_record(void* ev, void* stream);
int sgpmp_event_elapsed_ms(void* start, void* stop, float* ms);   /* synchronises on stop */
int sgpmp_event_destroy(void* ev);
/* Per-kernel accumulated device time (ms) measured with events inside sgpmp_step when enabled:
 * out double[4] = K5, K2, K3, K4; `launches` = steps accumulated.  Enabling inserts events only. */
int sgpmp_profile_enable(sgpmp_ctx* ctx, int on);
int sgpmp_profile_read(sgpmp_ctx* ctx, double* ms4, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* SGPMP_H */
