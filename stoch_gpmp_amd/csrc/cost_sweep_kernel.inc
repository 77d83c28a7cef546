// The cost-sweep kernel proper (included by cost_sweep.hip after the field helpers).
//
// Work item = (trajectory b, 64-waypoint pass c); each wave walks its items in a grid-stride loop.
// The kernel is VALU-bound (DESIGN.md), so the structure aims at few instructions and few exposed
// latencies per item:
//   * all per-lane data of an item -- the waypoint, its importance-sampling weights and, in FLAT
//     programs, the start state (lane 0) / goal state (lane T-1) -- is fetched by one batch of
//     vector loads at the top of the item; nothing is loaded under a divergent branch later;
//   * the goal block of the importance-sampling term is folded into the per-waypoint weights by
//     K5 (update.hip), so the sweep only needs one weight vector per lane;
//   * the 64-lane cost reduction runs on DPP row rotations + four readlanes, not LDS permutes;
//   * obstacle spheres are staged once per workgroup in LDS in the expanded-exponent form
//     (-2 k c, k, k |c|^2) with k = -log2(e)/(2 r^2), and read one sphere ahead of their use;
//   * FLAT programs (at most one term of each kind -- every cost list of the reference examples)
//     carry their constants in named kernel-argument fields that the compiler keeps in SGPRs for the
//     whole kernel, instead of re-loading a term record inside a loop over the term list.

// x_{t-1} from the neighbour lane: DPP wave_shr:1.  Lane 0 has no source lane and keeps `old`, which
// is the carried last waypoint of the previous 64-waypoint pass -- no select needed (v_cndmask on
// VCC measured ~10 ns per wave on gfx950, see tools/valu_bench2.hip).
__device__ __forceinline__ float lane_shr1(float v, float old) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ double lane_shr1(double v, double old) {
    const long long b = __double_as_longlong(v), o = __double_as_longlong(old);
    const int lo = __builtin_amdgcn_update_dpp((int)(o & 0xffffffffll), (int)(b & 0xffffffffll), 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(o >> 32), (int)(b >> 32), 0x138, 0xf, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ float lane_read(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ double lane_read(double v, int l) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), l);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// Sum over the 64 lanes without touching LDS: rotate-and-add inside each row of 16 (DPP row_ror),
// then add the four row sums through scalar reads.  Every lane returns the total.
template <int CTRL>
__device__ __forceinline__ double row_ror_add(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xf, 0xf, false);
    return v + __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double wave_sum_dpp(double v) {
    v = row_ror_add<0x128>(v);        // row_ror:8
    v = row_ror_add<0x124>(v);        // row_ror:4
    v = row_ror_add<0x122>(v);        // row_ror:2
    v = row_ror_add<0x121>(v);        // row_ror:1  -> every lane holds its row's sum
    return (lane_read(v, 0) + lane_read(v, 16)) + (lane_read(v, 32) + lane_read(v, 48));
}

// ---- per-waypoint terms that need no FK ----------------------------------------------------------
// CostGP / CostGPTrajectory (cost_functions.py:128-146, 202-215)
template <typename real, int N>
__device__ __forceinline__ double gp_term(const TermK<real>& tm, int t, bool valid, const real (&x)[2 * N],
                                          const real (&xp)[2 * N]) {
    constexpr int D = 2 * N;
    double out = 0.;
    if (t == 0 && (tm.flags & SGPMP_FLAG_GP_START)) {
        const SGPMP_CONST real* st = as_const((const real*)tm.dev_data);     // uniform: scalar loads
        real sq = 0;
#pragma unroll
        for (int i = 0; i < D; ++i) { const real dd = st[i] - x[i]; sq += dd * dd; }
        out += (double)(sq * tm.K2);
    }
    if (valid && t >= 1) {                          // e_{t-1} = x_t - Phi x_{t-1} (gp_factor.py:54-58)
        const real dt = tm.dt;
        real pp = 0, pv = 0, vv = 0;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const real ep = x[k] - (xp[k] + dt * xp[N + k]);
            const real ev = x[N + k] - xp[N + k];
            pp += ep * ep; pv += ep * ev; vv += ev * ev;
        }
        out += (double)(tm.K * (tm.c11 * pp + (real)2 * tm.c12 * pv + tm.c22 * vv));
    }
    return out;
}

// CostGoalPrior (cost_functions.py:376-388); `row` is the global row index of this trajectory
template <typename real, int N>
__device__ __forceinline__ double goal_term(const TermK<real>& tm, int t, int T, unsigned row,
                                            const real (&x)[2 * N]) {
    constexpr int D = 2 * N;
    if (t != T - 1) return 0.;
    const unsigned g = row / (unsigned)tm.rows_per_goal;
    const SGPMP_CONST real* gl = as_const((const real*)tm.dev_data + (size_t)g * D);
    real sq = 0;
#pragma unroll
    for (int i = 0; i < D; ++i) { const real dd = gl[i] - x[i]; sq += dd * dd; }
    return (double)(sq * tm.K);
}

// ---- sphere fields reading the LDS-staged spheres, one sphere ahead -------------------------------
#define SGPMP_SPH_LDS 128

// rbf exponent in expanded form: k |p - c|^2 = k |p|^2 + p . (-2 k c) + k |c|^2 -- 4 FMAs per
// (link, sphere) instead of 3 subtractions + 4 multiply-adds; |p|^2 is shared by all spheres.  The
// rounding error of the expansion is ~3e-6 relative on the exponential, far inside the fp32 budget.
// staged record: [-2 k c_x, -2 k c_y, -2 k c_z, k, k |c|^2, r, -, -]
// Two links per instruction: on gfx950 a VALU op with 2-3 VGPR sources issues at about half the rate
// of one with scalar sources, while the PACKED fp32 forms (v_pk_fma_f32 ...) take the same time for
// two lanes' worth of work (tools/valu_bench.hip), so the link loop is written on 2-vectors.
template <typename real, class CC>
__device__ __forceinline__ real spheres_rbf_cg(const real (&Pq)[CC::NREP][3], const real* sl, int n_sph,
                                               real acc) {
    using O = RealOps<real>;
    typedef real vec2 __attribute__((ext_vector_type(2)));
    constexpr int ND = CC::NDYN, NP = (ND + 1) / 2;
    vec2 X[NP], Y[NP], Z[NP], PP[NP], W[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int la = CC::dyn_link(2 * j), lb = CC::dyn_link(2 * j + 1 < ND ? 2 * j + 1 : 2 * j);
        X[j] = vec2{Pq[la][0], Pq[lb][0]};
        Y[j] = vec2{Pq[la][1], Pq[lb][1]};
        Z[j] = vec2{Pq[la][2], Pq[lb][2]};
        PP[j] = X[j] * X[j] + Y[j] * Y[j] + Z[j] * Z[j];
        W[j] = vec2{(real)CC::mult(la), 2 * j + 1 < ND ? (real)CC::mult(lb) : (real)0};
    }
    vec2 acc2 = {acc, (real)0};
    real ax = sl[0], ay = sl[1], az = sl[2], k = sl[3], b = sl[4];
    for (int o = 0; o < n_sph; ++o) {
        const real* nx = sl + (size_t)(o + 1 < n_sph ? o + 1 : o) * 8;
        const real nax = nx[0], nay = nx[1], naz = nx[2], nk = nx[3], nb = nx[4];   // next sphere, in flight
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const vec2 arg = PP[j] * k + (X[j] * ax + (Y[j] * ay + (Z[j] * az + b)));
            acc2 += W[j] * vec2{O::exp2_(arg.x), O::exp2_(arg.y)};
        }
        ax = nax; ay = nay; az = naz; k = nk; b = nb;
    }
    return acc2.x + acc2.y;
}

// ---- GEN: the sampler INSIDE the sweep (fp64 contexts; round 6) ------------------------------------------------------------
// The fp32 steps fuse K2 and K3 through an LDS tile (fused_step.inc: lane = (sample, dof) for the recurrence, lane = (row pair,
// waypoint) for the costs).  An fp64 step keeps THIS kernel's mapping -- one wave per trajectory, lane = waypoint -- and produces
// the lane's waypoint in place: its noise (the fp64 stream of rng.h, keyed on the waypoint), the noise terms b_t = G_t eps_t,
// and the recurrence y_t = H_t y_{t-1} + b_t of all 64 waypoints of a pass at once as a Kogge-Stone scan over the lanes -- six
// rounds of  y_t += A_t^(r) y_{t - 2^r}  with the 2 x 2 products A_t^(r) = H_t ... H_{t - 2^r + 1} (zero where t - 2^r lies before
// the pass) from a table the host builds once per factorisation (api.hip: upload_scan64; the propagators of an isotropic prior
// are the same for every dof, particle and sample) -- plus C_t y_carry for passes after the first.  x = mu + y is stored (the
// step's state_samples) and handed to the cost terms in registers: the 0.94 GB that sample_iso_kernel<double> wrote and this
// kernel re-read at config 3's shape never make the round trip.
struct GenArgs64 {
    const double* coef;          // PriorDev::iso64 [T][8]: g11 g21 g22 h11 h12 h21 h22 -
    const double* scan;          // [T][7][4]: A^(0) .. A^(5), C   (row-major 2 x 2)
    const double* means;         // [P][T][D]
    double* samples;             // [P][S][T][D]
    uint64_t seed, draw;
    int mode_offset, S;
    double* zero_stats;          // the step's statistics shards, zeroed by workgroup 0 (or null)
};
#define SGPMP_SCAN64_ROW 28      // doubles per waypoint of the scan table

// the value of lane (addr / 4) mod 64: two ds_bpermute_b32, no range check (the scan multiplies what a lane without a source reads by zero)
__device__ __forceinline__ double lane_from(double v, int addr) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_ds_bpermute(addr, (int)(b & 0xffffffffll));
    const int hi = __builtin_amdgcn_ds_bpermute(addr, (int)(b >> 32));
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// ... of the neighbour lane (lane ^ 1): DPP quad_perm [1, 0, 3, 2]
__device__ __forceinline__ float lane_swap1(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xb1, 0xf, 0xf, false));
}

// FKMODE: 0 = no link fields; -1 = generic chain (LDS); 1..999 = register path with that many
// joints; >= 1000 = build-time generated chain code.  FLAT: program has at most one term per kind.
template <typename real, int N, int FKMODE, bool FLAT, bool GEN, bool MIXED = false, int SCAN = 0>
__device__ __forceinline__ void cost_sweep_body(const CostArgs<real>& a, const ProgK<real>& P, const FlatProg<real>& F,
                                                const GenArgs64& g) {
    constexpr int D = 2 * N;
    typedef real real2 __attribute__((ext_vector_type(2)));
    extern __shared__ __align__(16) unsigned char lds_raw[];
    real* lds = reinterpret_cast<real*>(lds_raw);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // scalar
    const int waves_per_block = blockDim.x >> 6;
    const int stride = blockDim.x;
    real* col = lds + threadIdx.x;
    const int T = a.T;
    const int nchunks = (T + 63) >> 6;
    if constexpr (GEN) {
        if (g.zero_stats && blockIdx.x == 0)
            for (int e = threadIdx.x; e < SGPMP_STAT_SHARDS * 4; e += blockDim.x) g.zero_stats[e] = 0.;
        if constexpr (SCAN != 0) {
            for (int e = threadIdx.x; e < T * SGPMP_SCAN64_ROW; e += blockDim.x) reinterpret_cast<double*>(lds_raw)[e] = g.scan[e];
            if constexpr (FKMODE < 1000) __syncthreads();        // (the generated-chain prologue below ends with a barrier)
        }
    }

    __shared__ double stat[4 * SGPMP_MAX_TERMS];         // per wave: sphere terms of the static links
    __shared__ __align__(16) real sphl[(FKMODE >= 1000 && !MIXED ? SGPMP_SPH_LDS : 1) * 8];   // (MIXED reads the fp32 tables below)
    __shared__ __align__(16) float sphl32[(FKMODE >= 1000 && MIXED ? SGPMP_SPH_LDS : 1) * 8], sph32[(FKMODE >= 1000 && MIXED ? SGPMP_SPH_LDS : 1) * 4];
    if constexpr (FKMODE >= 1000) {
        using CC = typename ChainOf<FKMODE>::type;
        const bool staged = a.n_spheres <= SGPMP_SPH_LDS;
        if (staged && !MIXED) {
            for (int o = threadIdx.x; o < a.n_spheres; o += blockDim.x) {
                const real cx = a.spheres[o * 4 + 0], cy = a.spheres[o * 4 + 1], cz = a.spheres[o * 4 + 2];
                const real r = a.spheres[o * 4 + 3];
                const real k = (real)(-0.5 * SGPMP_LOG2E) / (r * r);
                sphl[o * 8 + 0] = (real)-2 * k * cx;
                sphl[o * 8 + 1] = (real)-2 * k * cy;
                sphl[o * 8 + 2] = (real)-2 * k * cz;
                sphl[o * 8 + 3] = k;
                sphl[o * 8 + 4] = k * (cx * cx + cy * cy + cz * cz);
                sphl[o * 8 + 5] = r;
            }
        }
        if constexpr (MIXED) {
            // the same tables in fp32 for the packed-fp32 field code (expanded rbf form / raw spheres)
            for (int o = threadIdx.x; o < a.n_spheres && staged; o += blockDim.x) {
                const float cx = (float)a.spheres[o * 4 + 0], cy = (float)a.spheres[o * 4 + 1], cz = (float)a.spheres[o * 4 + 2];
                const float r = (float)a.spheres[o * 4 + 3];
                const float k = (float)(-0.5 * SGPMP_LOG2E) / (r * r);
                sphl32[o * 8 + 0] = -2.f * k * cx; sphl32[o * 8 + 1] = -2.f * k * cy; sphl32[o * 8 + 2] = -2.f * k * cz;
                sphl32[o * 8 + 3] = k; sphl32[o * 8 + 4] = k * (cx * cx + cy * cy + cz * cz); sphl32[o * 8 + 5] = r;
                sph32[o * 4 + 0] = cx; sph32[o * 4 + 1] = cy; sph32[o * 4 + 2] = cz; sph32[o * 4 + 3] = r;
            }
        }
        real q0[N], P0[CC::NREP][3];
#pragma unroll
        for (int k = 0; k < N; ++k) q0[k] = 0;
        fk_cg<real, CC>(q0, P0);                         // static links do not depend on q
        for (int ti = 0; ti < P.n_terms; ++ti) {
            const TermK<real>& tm = P.t[ti];
            if (tm.kind != SGPMP_COST_SPHERES) continue;
            const real init = ((tm.flags & 15) == SGPMP_FIELD_SDF) ? (real)-1e30 : (real)0;
            const real v = spheres_field_cg<real, CC, true>(tm, P0, a.spheres, a.n_spheres, init);
            if (lane == 0) stat[wave * SGPMP_MAX_TERMS + ti] = (double)v;
        }
        __syncthreads();
    }

    const long long wstride = (long long)gridDim.x * waves_per_block;
    long long b = (long long)blockIdx.x * waves_per_block + wave;
    int c = 0;
    const bool use_is = a.isw != nullptr;

    // loads of one item: the lane's waypoint (index clamped: lanes past T re-read the last waypoint
    // and are masked when accumulating) and its block of importance-sampling weights
    auto load_item = [&](long long bb, int cc, real (&x)[D], real (&w)[D]) {
        const int t = min((cc << 6) + lane, T - 1);
        const real2* r2 = reinterpret_cast<const real2*>(a.trajs + ((size_t)bb * T + t) * D);
#pragma unroll
        for (int i = 0; i < N; ++i) { const real2 v = r2[i]; x[2 * i] = v.x; x[2 * i + 1] = v.y; }
        if (use_is) {
            const unsigned p = (unsigned)bb / (unsigned)a.rows_per_particle;   // host checks rows < 2^31
            const real2* w2 = reinterpret_cast<const real2*>(a.isw + ((size_t)p * (T + 1) + t) * D);
#pragma unroll
            for (int i = 0; i < N; ++i) { const real2 v = w2[i]; w[2 * i] = v.x; w[2 * i + 1] = v.y; }
        } else {
#pragma unroll
            for (int i = 0; i < D; ++i) w[i] = 0;
        }
    };

    // GEN: the lane's waypoint of trajectory bb produced in place (see GenArgs64); y_carry: the state at the end of the previous
    // pass of the same trajectory (zero in pass 0)
    real ycar[D];
#pragma unroll
    for (int i = 0; i < D; ++i) ycar[i] = 0;
    auto gen_item = [&](long long bb, int cc, real (&x)[D], real (&w)[D]) {
        if constexpr (GEN) {
            const int tt = (cc << 6) + lane;
            const int t = min(tt, T - 1);                // lanes past T repeat the last waypoint's inputs; nothing of theirs is kept
            const unsigned p = (unsigned)bb / (unsigned)g.S;
            const unsigned sidx = (unsigned)bb - p * (unsigned)g.S;
            const double* cf = g.coef + (size_t)t * 8;
            // the lane's row of the scan table.  SCAN 0 (small launches): from memory, one batch at the top -- one round trip.
            // SCAN 1: staged per workgroup in LDS, read in one batch at the top.  SCAN 2: staged, read ROUND BY ROUND -- 56 registers
            // less at the scan's peak: what lets the fp32-link-fields launch hold three waves per SIMD without spilling; the all-fp64
            // launch sits at two waves either way and measured 3.6 % slower with a read inside every round (823 against 794 us).
            constexpr bool SCAN_LDS = SCAN == 2;
            double A[SCAN_LDS ? 1 : SGPMP_SCAN64_ROW];
            const double2* const sl = reinterpret_cast<const double2*>(reinterpret_cast<const double*>(lds_raw) + (size_t)t * SGPMP_SCAN64_ROW);
            if constexpr (!SCAN_LDS) {
                const double2* sg = SCAN == 1 ? sl : reinterpret_cast<const double2*>(g.scan + (size_t)t * SGPMP_SCAN64_ROW);
#pragma unroll
                for (int j = 0; j < SGPMP_SCAN64_ROW / 2; ++j) { const double2 v = sg[j]; A[2 * j] = v.x; A[2 * j + 1] = v.y; }
            }
            // means of this waypoint (independent of everything below: issued first)
            const real2* m2 = reinterpret_cast<const real2*>(g.means + ((size_t)p * T + t) * D);
            real mu[D];
#pragma unroll
            for (int i = 0; i < N; ++i) { const real2 v = m2[i]; mu[2 * i] = v.x; mu[2 * i + 1] = v.y; }
            if (use_is) {
                const real2* w2 = reinterpret_cast<const real2*>(a.isw + ((size_t)p * (T + 1) + t) * D);
#pragma unroll
                for (int i = 0; i < N; ++i) { const real2 v = w2[i]; w[2 * i] = v.x; w[2 * i + 1] = v.y; }
            } else {
#pragma unroll
                for (int i = 0; i < D; ++i) w[i] = 0;
            }
            // the noise: a Philox block carries the four normals of one dof at the waypoints (2b, 2b + 1) -- the lanes of a pair
            // share the blocks: the even lane forms those of the even dofs, the odd lane those of the odd dofs, each keeps its own
            // waypoint's half and hands the other half to its neighbour (DPP quad_perm).  Same values as NoiseGen<float>::get4.
            double yp[N], yv[N];
            {
                const bool odd = (lane & 1) != 0;
                NoiseGen<float> gen;
#pragma unroll
                for (int j = 0; j < (N + 1) / 2; ++j) {
                    const int kmine = 2 * j + (odd ? 1 : 0);
                    gen.init(g.seed, g.draw, (uint32_t)(g.mode_offset + (int)p), sidx, (uint32_t)(kmine < N ? kmine : 0));
                    float e[4];
                    gen.get4(tt & ~1, e);                                    // (past T: a block nobody uses)
                    const float keep_p = odd ? e[2] : e[0], keep_v = odd ? e[3] : e[1];
                    const float recv_p = lane_swap1(odd ? e[0] : e[2]), recv_v = lane_swap1(odd ? e[1] : e[3]);
                    const double p0 = (double)(odd ? recv_p : keep_p), v0 = (double)(odd ? recv_v : keep_v);     // dof 2j
                    scan_step_noise<double>(cf, p0, v0, yp[2 * j], yv[2 * j]);      // b_t = G_t eps_t (rng.h: the sampler's own expression)
                    if (2 * j + 1 < N) {
                        const double p1 = (double)(odd ? keep_p : recv_p), v1 = (double)(odd ? keep_v : recv_v); // dof 2j + 1
                        scan_step_noise<double>(cf, p1, v1, yp[2 * j + 1], yv[2 * j + 1]);
                    }
                }
            }
            // Kogge-Stone over the lanes: round r adds A^(r) y_{t - 2^r}
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                double a00, a01, a10, a11;
                if constexpr (SCAN_LDS) { const double2 u = sl[2 * r], v = sl[2 * r + 1]; a00 = u.x; a01 = u.y; a10 = v.x; a11 = v.y; }
                else { a00 = A[4 * r]; a01 = A[4 * r + 1]; a10 = A[4 * r + 2]; a11 = A[4 * r + 3]; }
                const int src = (lane - (1 << r)) * 4;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const double sp = r == 0 ? lane_shr1(yp[k], 0.) : lane_from(yp[k], src);
                    const double sv = r == 0 ? lane_shr1(yv[k], 0.) : lane_from(yv[k], src);
                    yp[k] = __builtin_fma(a01, sv, __builtin_fma(a00, sp, yp[k]));
                    yv[k] = __builtin_fma(a11, sv, __builtin_fma(a10, sp, yv[k]));
                }
            }
            if (nchunks > 1) {
                double c00, c01, c10, c11;
                if constexpr (SCAN_LDS) { const double2 u = sl[12], v = sl[13]; c00 = u.x; c01 = u.y; c10 = v.x; c11 = v.y; }
                else { c00 = A[24]; c01 = A[25]; c10 = A[26]; c11 = A[27]; }
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    yp[k] = __builtin_fma(c01, ycar[N + k], __builtin_fma(c00, ycar[k], yp[k]));
                    yv[k] = __builtin_fma(c11, ycar[N + k], __builtin_fma(c10, ycar[k], yv[k]));
                }
#pragma unroll
                for (int k = 0; k < N; ++k) { ycar[k] = lane_read(yp[k], 63); ycar[N + k] = lane_read(yv[k], 63); }
                if (cc == nchunks - 1) {
#pragma unroll
                    for (int i = 0; i < D; ++i) ycar[i] = 0;
                }
            }
#pragma unroll
            for (int k = 0; k < N; ++k) { x[k] = mu[k] + yp[k]; x[N + k] = mu[N + k] + yv[k]; }
            if constexpr (SCAN == 1 || (MIXED && SCAN == 2)) {
                // (the chain launches) the pass's 64 waypoints x D doubles through a wave-private LDS tile, so that every store
                // instruction writes 1 KB of consecutive bytes (64 lanes x 16) instead of 64 pieces 112 bytes apart: all-fp64 794 ->
                // 766 us at config 3's shape; link fields in fp32 478 -> 455 us once the fp64 sphere table it never reads left its
                // LDS (with it the tile's 28 KB cost the launch its third workgroup per CU: -7 %).  The planar launches lose a
                // workgroup per CU to the tile and ran 7 % slower with it (profiles/r06/store_policy_ab.txt)
                double* tile = reinterpret_cast<double*>(lds_raw) + (size_t)T * SGPMP_SCAN64_ROW + (size_t)wave * 64 * D;
                real2* t2 = reinterpret_cast<real2*>(tile + (size_t)lane * D);
#pragma unroll
                for (int i = 0; i < N; ++i) t2[i] = real2{x[2 * i], x[2 * i + 1]};
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const int t0p = cc << 6;
                const int nvalid = min(64, T - t0p) * (D / 2);                    // 16-byte pieces of this pass that exist
                real2* ob = reinterpret_cast<real2*>(g.samples + ((size_t)bb * T + t0p) * D);
                const real2* tb = reinterpret_cast<const real2*>(tile);
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    const int q = j * 64 + lane;
                    if (q < nvalid) ob[q] = tb[q];
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
            } else if (tt < T) {
                real2* o2 = reinterpret_cast<real2*>(g.samples + ((size_t)bb * T + t) * D);
                // (plain stores: a lane writes its waypoint's 112 bytes in 16-byte pieces that L2 merges into full lines -- as
                // non-temporal stores they reached HBM piecemeal: 0.81 -> 1.21 ms per iteration at config 3's shape, round 6)
#pragma unroll
                for (int i = 0; i < N; ++i) o2[i] = real2{x[2 * i], x[2 * i + 1]};
            }
        }
    };

    real x[D], w[D];
    bool have = b < a.batch;
    double acc = 0.;
    real carry[D];
#pragma unroll
    for (int i = 0; i < D; ++i) carry[i] = 0;

    while (have) {
        long long nb = b;
        int nc = c + 1;
        if (nc == nchunks) { nb = b + wstride; nc = 0; }
        const bool have_next = nb < a.batch;

        const int t = (c << 6) + lane;
        const bool valid = t < T;
        const bool inner = valid && t >= 1;              // waypoints 1..T-1 carry the field costs
        const unsigned row = (unsigned)(a.batch_offset + b);
        if constexpr (GEN) gen_item(b, c, x, w);
        else load_item(b, c, x, w);
        // FLAT: start state for lane 0 / this trajectory's goal state for lane T-1, as one more
        // per-lane vector load in the same batch (other lanes read the goal row and ignore it)
        real aux[D];
        if constexpr (FLAT) {
            const real* gp = F.has_goal ? (const real*)F.goal.dev_data + (size_t)(row / (unsigned)F.goal.rows_per_goal) * D
                                        : a.trajs;
            const real* sp = (F.has_gp && (F.gp.flags & SGPMP_FLAG_GP_START)) ? (const real*)F.gp.dev_data : gp;
            const real2* a2 = reinterpret_cast<const real2*>(t == 0 ? sp : gp);
#pragma unroll
            for (int i = 0; i < N; ++i) { const real2 v = a2[i]; aux[2 * i] = v.x; aux[2 * i + 1] = v.y; }
        }
        real xp[D];
#pragma unroll
        for (int i = 0; i < D; ++i) xp[i] = lane_shr1(x[i], carry[i]);
        if (nchunks > 1) {
#pragma unroll
            for (int i = 0; i < D; ++i) carry[i] = lane_read(x[i], 63);
        }
        real part = 0;                                   // this waypoint's cost, in `real`
        double part64 = 0.;

        // ---- terms without FK
        if constexpr (FLAT) {
            // start-state unary factor on lane 0, goal prior on lane T-1 (unary_factor.py:21-22)
            real sq = 0;
#pragma unroll
            for (int i = 0; i < D; ++i) { const real dd = aux[i] - x[i]; sq += dd * dd; }
            const real ku = (t == 0) ? ((F.has_gp && (F.gp.flags & SGPMP_FLAG_GP_START)) ? F.gp.K2 : (real)0)
                                     : ((t == T - 1 && F.has_goal) ? F.goal.K : (real)0);
            part64 += (double)(sq * ku);
            if (F.has_gp && inner) {                 // e_{t-1} = x_t - Phi x_{t-1} (gp_factor.py:54-58)
                const real dt = F.gp.dt;
                real pp = 0, pv = 0, vv = 0;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const real ep = x[k] - (xp[k] + dt * xp[N + k]);
                    const real ev = x[N + k] - xp[N + k];
                    pp += ep * ep; pv += ep * ev; vv += ev * ev;
                }
                part64 += (double)(F.gp.K * (F.gp.c11 * pp + (real)2 * F.gp.c12 * pv + F.gp.c22 * vv));
            }
            if (F.has_grid) {
                const real gv = grid_value<real>(F.grid, x[0], x[N > 1 ? 1 : 0]);
                if (inner) part += F.grid.K * gv;
            }
        } else {
            for (int ti = 0; ti < P.n_terms; ++ti) {
                const TermK<real>& tm = P.t[ti];
                if (tm.kind == SGPMP_COST_GP) {
                    part64 += gp_term<real, N>(tm, t, valid, x, xp);
                } else if (tm.kind == SGPMP_COST_GOAL_PRIOR) {
                    part64 += goal_term<real, N>(tm, t, T, row, x);
                } else if (tm.kind == SGPMP_COST_GRID) {
                    const real gv = grid_value<real>(tm, x[0], x[N > 1 ? 1 : 0]);
                    if (inner) part += tm.K * gv;
                } else if (tm.kind == SGPMP_COST_GRID_SDF) {
                    const real h = grid_sdf_field<real, false>(tm, x[0], x[N > 1 ? 1 : 0], nullptr, nullptr);
                    if (inner) part += tm.K * h;
                }
            }
        }
        // ---- link fields
        if constexpr (FKMODE != 0) {
            if (P.needs_fk) {
                // every lane runs FK (uniform control flow); lanes past T repeat the last waypoint
                real q[N];
#pragma unroll
                for (int k = 0; k < N; ++k) q[k] = x[k];
                if constexpr (FKMODE >= 1000 && MIXED && FLAT) {
                    // option f64_fields_f32: the link fields of the fp64 waypoint on the fp32 launches' packed code (the q-independent
                    // parts -- static links, rigid pairs -- stay the fp64 values of the prologue / the host)
                    using CC = typename ChainOf<FKMODE>::type;
                    float q32[N], Pq[CC::NREP][3];
#pragma unroll
                    for (int k = 0; k < N; ++k) q32[k] = (float)q[k];
                    fk_cg<float, CC>(q32, Pq);
                    if (F.has_self) {
                        TermK<float> ts;
                        ts.flags = F.self.flags; ts.K2 = (float)F.self.K2; ts.selfc = 0.f;
                        const real f = (real)self_field_cg<float, CC>(ts, Pq) + F.self.selfc;
                        if (inner) part += F.self.K * f;
                    }
                    if (F.has_sph) {
                        const real st = (real)stat[wave * SGPMP_MAX_TERMS + F.sph_index];
                        const int type = F.sph.flags & 15;
                        real f;
                        if (type == SGPMP_FIELD_RBF && a.n_spheres <= SGPMP_SPH_LDS)
                            f = st + (real)spheres_rbf_cg<float, CC>(Pq, sphl32, a.n_spheres, 0.f);
                        else {                       // (the launcher takes this instantiation for <= SGPMP_SPH_LDS spheres only)
                            TermK<float> tsp;
                            tsp.flags = F.sph.flags;
                            const float init = type == SGPMP_FIELD_SDF ? (float)st : 0.f;
                            const float v = spheres_field_cg<float, CC, false>(tsp, Pq, sph32, a.n_spheres, init);
                            f = type == SGPMP_FIELD_SDF ? (real)v : st + (real)v;
                        }
                        if (inner) part += F.sph.K * f;
                    }
                } else if constexpr (FKMODE >= 1000) {
                    using CC = typename ChainOf<FKMODE>::type;
                    real Pq[CC::NREP][3];
                    fk_cg<real, CC>(q, Pq);
                    if constexpr (FLAT) {
                        if (F.has_self) {
                            const real f = self_field_cg<real, CC>(F.self, Pq);
                            if (inner) part += F.self.K * f;
                        }
                        if (F.has_sph) {
                            const real st = (real)stat[wave * SGPMP_MAX_TERMS + F.sph_index];
                            real f;
                            if ((F.sph.flags & 15) == SGPMP_FIELD_RBF && a.n_spheres <= SGPMP_SPH_LDS)
                                f = spheres_rbf_cg<real, CC>(Pq, sphl, a.n_spheres, st);
                            else
                                f = spheres_field_cg<real, CC, false>(F.sph, Pq, a.spheres, a.n_spheres, st);
                            if (inner) part += F.sph.K * f;
                        }
                    } else {
                        for (int ti = 0; ti < P.n_terms; ++ti) {
                            const TermK<real>& tm = P.t[ti];
                            real f;
                            if (tm.kind == SGPMP_COST_SPHERES)
                                f = spheres_field_cg<real, CC, false>(tm, Pq, a.spheres, a.n_spheres,
                                                                      (real)stat[wave * SGPMP_MAX_TERMS + ti]);
                            else if (tm.kind == SGPMP_COST_SELF)
                                f = self_field_cg<real, CC>(tm, Pq);
                            else if (tm.kind == SGPMP_COST_VOXEL_SDF)
                                f = voxel_field_cg<real, CC>(tm, Pq);
                            else
                                continue;
                            if (inner) part += tm.K * f;
                        }
                    }
                } else if constexpr (FKMODE > 0) {
                    real PX[FKMODE + 1], PY[FKMODE + 1], PZ[FKMODE + 1];
                    ChainC chain = as_const(a.chain);
                    fk_points_reg<real, N, FKMODE>(chain, q, PX, PY, PZ);
                    for (int ti = 0; ti < P.n_terms; ++ti) {
                        const TermK<real>& tm = P.t[ti];
                        real f;
                        if (tm.kind == SGPMP_COST_SPHERES)
                            f = spheres_field_reg<real, FKMODE>(tm, chain, PX, PY, PZ, a.spheres, a.n_spheres);
                        else if (tm.kind == SGPMP_COST_SELF)
                            f = self_field_reg<real, FKMODE>(tm, chain, PX, PY, PZ);
                        else if (tm.kind == SGPMP_COST_VOXEL_SDF)
                            f = voxel_field_reg<real, FKMODE>(tm, chain, PX, PY, PZ);
                        else
                            continue;
                        if (inner) part += tm.K * f;
                    }
                } else {
                    fk_points<real, N>(a.chain, q, col, stride);
                    for (int ti = 0; ti < P.n_terms; ++ti) {
                        const TermK<real>& tm = P.t[ti];
                        if (tm.kind != SGPMP_COST_SPHERES && tm.kind != SGPMP_COST_SELF && tm.kind != SGPMP_COST_VOXEL_SDF) continue;
                        if (tm.n_interp > 0) add_interp_points<real>(tm, a.n_links, col, stride);
                        real f;
                        if (tm.kind == SGPMP_COST_SPHERES)
                            f = spheres_field<real>(tm, tm.n_points, col, stride, a.spheres, a.n_spheres);
                        else if (tm.kind == SGPMP_COST_VOXEL_SDF)
                            f = voxel_field<real>(tm, tm.n_points, col, stride);
                        else
                            f = self_field<real>(tm, tm.n_points, col, stride);
                        if (inner) part += tm.K * f;
                    }
                }
            }
        }
        // ---- importance-sampling term with the sampling prior's (A x)_t
        if (use_is) {
            real dot = 0;
            if (t == 0) {
#pragma unroll
                for (int i = 0; i < D; ++i) dot += x[i] * w[i];
            } else {
                const real dt = a.is_dt;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const real ep = x[k] - (xp[k] + dt * xp[N + k]);
                    const real ev = x[N + k] - xp[N + k];
                    dot += ep * w[k] + ev * w[N + k];
                }
            }
            if (valid) part64 += (double)dot;            // (goal block already folded into w by K5)
        }
        acc += part64 + (double)part;

        if (c == nchunks - 1) {
            acc = wave_sum_dpp(acc);
            if (lane == 0) {
                if (a.costs) a.costs[b] = (real)acc;
                if (a.costs64) a.costs64[b] = acc;
            }
            acc = 0.;
#pragma unroll
            for (int i = 0; i < D; ++i) carry[i] = 0;
        }
        b = nb; c = nc; have = have_next;
    }
}

template <typename real, int N, int FKMODE, bool FLAT>
__global__ void __launch_bounds__(256)
cost_sweep_kernel(const CostArgs<real> a, const ProgK<real> P, const FlatProg<real> F) {
    const GenArgs64 none = {};
    cost_sweep_body<real, N, FKMODE, FLAT, false>(a, P, F, none);
}

// K2 + K3 of an fp64 step in one launch (FLAT programs; FKMODE 0: no link fields, 1000: the built-in chain code)
template <int N, int FKMODE, int SCAN>
__global__ void __launch_bounds__(256)
fused_step_f64_kernel(const CostArgs<double> a, const ProgK<double> P, const FlatProg<double> F, const GenArgs64 g) {
    cost_sweep_body<double, N, FKMODE, true, true, false, SCAN>(a, P, F, g);
}
// option f64_fields_f32: the link fields on the packed-fp32 code, everything else fp64 (three waves per SIMD: the fp32 field
// code needs fewer registers than the fp64 one, and the scan's ds_bpermute round trips want the third wave to hide behind)
template <int N, int FKMODE, int SCAN>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3)))
fused_step_f64_mixed_kernel(const CostArgs<double> a, const ProgK<double> P, const FlatProg<double> F, const GenArgs64 g) {
    cost_sweep_body<double, N, FKMODE, true, true, true, SCAN>(a, P, F, g);
}
