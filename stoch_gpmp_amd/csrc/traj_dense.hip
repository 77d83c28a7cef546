// Dense trajectories: GP interpolation between the support waypoints (sgpmp_interpolate) and a collision / limit check over ALL
// fine states (sgpmp_validate).  No reference counterpart: the reference looks at the T support waypoints only.
//
// The interpolant is the posterior mean of the planner's own constant-velocity GP prior between two support states,
//   x(tau) = Lambda(tau) x_i + Psi(tau) x_{i+1},   Psi = Q(tau) Phi(dt - tau)^T Q(dt)^-1,   Lambda = Phi(tau) - Psi Phi(dt),
// in which Q_c and the prior mean cancel: the cubic Hermite spline on (q, q').  With k = n_sub points inserted per interval,
// fine index f = i (k + 1) + m is the state at s = m / (k + 1) of interval i; the eight weights of a sub-step m are formed by
// the host in fp64 and rounded once (hermite_coefs), and the state is evaluated in ONE explicit-fma order by ONE device function
// (hermite_state) that both kernels call -- the same discipline as rng.h's scan recurrence: the fine states of sgpmp_interpolate
// and the ones sgpmp_validate looks at are the same bits.
//
// Mapping: ONE WAVE PER TRAJECTORY, ONE LANE PER SUPPORT WAYPOINT i (64 per pass).  Lane i loads waypoint i (consecutive lanes read
// consecutive rows), takes waypoint i + 1 from its neighbour lane, and walks the k + 1 fine states of interval i (the last
// waypoint's lane: that waypoint alone).  sgpmp_validate keeps four running (value, fine index) pairs per lane, reduces them
// across the wave once with ties to the lower index, and one lane stores the 4 + 4 results; the fine states and their link
// positions (generic forward kinematics, any chain, one LDS column per lane) never reach memory.  Composed from
// the stand-alone ops (interpolate -> sgpmp_fk -> sgpmp_link_distances) the same check moves B T_f L 16 reals of frames.
//
// The two entry points live here, next to their launchers, and reach the context through SgpmpCtxView (sgpmp_internal.h).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "chain_code_generated.h"
#include "sgpmp_internal.h"
#include "cost_device.h"
#include "cost_host.h"

// ---------------------------------------------------------------------------------- shared Hermite evaluation
template <typename real>
struct HermiteK {                // per sub-step m = 1 .. k: q = c0 q_i + c1 v_i + c2 q_{i+1} + c3 v_{i+1}, v = c4 .. c7 likewise
    real c[SGPMP_MAX_SUBSTEPS][8];
};

// h00 h10 dt h01 h11 dt | h00'/dt h10' h01'/dt h11'  at s = m / (k + 1), in fp64, rounded once to the compute type
template <typename real>
static HermiteK<real> hermite_coefs(int n_sub, double dt) {
    HermiteK<real> K;
    std::memset(&K, 0, sizeof(K));
    for (int m = 1; m <= n_sub; ++m) {
        const double s = (double)m / (double)(n_sub + 1), s2 = s * s, s3 = s2 * s;
        const double h00 = 2. * s3 - 3. * s2 + 1., h10 = s3 - 2. * s2 + s, h01 = -2. * s3 + 3. * s2, h11 = s3 - s2;
        const double g00 = 6. * s2 - 6. * s, g10 = 3. * s2 - 4. * s + 1., g01 = -g00, g11 = 3. * s2 - 2. * s;
        real* c = K.c[m - 1];
        c[0] = (real)h00; c[1] = (real)(h10 * dt); c[2] = (real)h01; c[3] = (real)(h11 * dt);
        c[4] = (real)(g00 / dt); c[5] = (real)g10; c[6] = (real)(g01 / dt); c[7] = (real)g11;
    }
    return K;
}

// State m >= 1 of the interval (a, b), a = (q_i, v_i), b = (q_{i+1}, v_{i+1}); x = (q, v).  One multiply and three fmas per
// coordinate, in this order, nowhere else (m = 0 is a copy of `a`, made by the caller).
template <typename real, int N>
__device__ __forceinline__ void hermite_state(const real (&a)[2 * N], const real (&b)[2 * N], const real* __restrict__ c,
                                              real (&x)[2 * N]) {
    using O = RealOps<real>;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        x[k] = __builtin_fma(c[3], b[N + k], __builtin_fma(c[2], b[k], __builtin_fma(c[1], a[N + k], O::mul_rn(c[0], a[k]))));
        x[N + k] = __builtin_fma(c[7], b[N + k], __builtin_fma(c[6], b[k], __builtin_fma(c[5], a[N + k], O::mul_rn(c[4], a[k]))));
    }
}

// Waypoints i (own row) and i + 1 (the neighbour lane's row; lane 63 loads it itself) of trajectory `tr`, for i < T.
template <typename real, int N>
__device__ __forceinline__ void load_interval(const real* __restrict__ tr, int T, int i, int lane, real (&a)[2 * N],
                                              real (&b)[2 * N]) {
    const real* row = tr + (size_t)(i < T ? i : T - 1) * (2 * N);
#pragma unroll
    for (int k = 0; k < 2 * N; ++k) a[k] = row[k];
#pragma unroll
    for (int k = 0; k < 2 * N; ++k) b[k] = __shfl_down(a[k], 1, 64);
    if (lane == 63) {
        const real* nxt = tr + (size_t)(i + 1 < T ? i + 1 : T - 1) * (2 * N);
#pragma unroll
        for (int k = 0; k < 2 * N; ++k) b[k] = nxt[k];
    }
}

// ---------------------------------------------------------------------------------- sgpmp_interpolate
template <typename real, int N>
__global__ void __launch_bounds__(64)
interpolate_kernel(const real* __restrict__ trajs, long long batch, int T, int n_sub, HermiteK<real> H, real* __restrict__ out) {
    const int lane = threadIdx.x;
    const int k1 = n_sub + 1;
    const long long Tf = (long long)(T - 1) * k1 + 1;
    for (long long b = blockIdx.x; b < batch; b += gridDim.x) {
        const real* tr = trajs + (size_t)b * T * (2 * N);
        real* ob = out + (size_t)b * Tf * (2 * N);
        for (int base = 0; base < T; base += 64) {
            const int i = base + lane;
            real a[2 * N], nb[2 * N], x[2 * N];
            load_interval<real, N>(tr, T, i, lane, a, nb);
            const int nm = i < T - 1 ? k1 : (i == T - 1 ? 1 : 0);
            for (int m = 0; m < nm; ++m) {
                if (m == 0) {
#pragma unroll
                    for (int k = 0; k < 2 * N; ++k) x[k] = a[k];
                } else {
                    hermite_state<real, N>(a, nb, H.c[m - 1], x);
                }
                real* o = ob + ((size_t)i * k1 + m) * (2 * N);
#pragma unroll
                for (int k = 0; k < 2 * N; ++k) o[k] = x[k];
            }
        }
    }
}

// ---------------------------------------------------------------------------------- sgpmp_validate
// cost_device.h's generic fk_points (any chain, link positions into this lane's LDS column, stride 64) -- the same operations in
// the same order -- with the joint constants read through the CONSTANT address space (scalar loads: every lane of the wave
// wants the same 12 numbers per joint) and, in fp32, from the chain's fp32 copies instead of converting the doubles per state.
// Measured against the plain-pointer form at 131 072 x 64 waypoints, n_sub = 4: 5.68 against 5.86 ms -- the kernel is bound by
// its vector arithmetic (library sincos, sqrt, the 55 + 30 distances per fine state), not by these loads.
template <typename real, int N>
__device__ __forceinline__ void fk_points_const(ChainC chain, int n_links, const real (&q)[N], real* col) {
    using O = RealOps<real>;
    real R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    real p[3] = {0, 0, 0};
    col[0] = 0; col[64] = 0; col[128] = 0;
    for (int j = 0; j + 1 < n_links; ++j) {
        ChainC ch = opaque(chain);                         // this joint's constants: loaded here, not hoisted and spilled
        real F[9], tt[3];
#pragma unroll
        for (int i = 0; i < 9; ++i) F[i] = JointK<real>::R(ch, j, i);
#pragma unroll
        for (int i = 0; i < 3; ++i) tt[i] = JointK<real>::t(ch, j, i);
#pragma unroll
        for (int r = 0; r < 3; ++r) p[r] += R[r * 3 + 0] * tt[0] + R[r * 3 + 1] * tt[1] + R[r * 3 + 2] * tt[2];
        real Rn[9];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                Rn[r * 3 + c] = R[r * 3 + 0] * F[c] + R[r * 3 + 1] * F[3 + c] + R[r * 3 + 2] * F[6 + c];
        if (ch->j[j].revolute) {
            const int qidx = ch->j[j].qidx;
            real qv = 0;
#pragma unroll
            for (int i = 0; i < N; ++i) qv = (qidx == i) ? q[i] : qv;
            real s, c;
            O::sincos_(qv, &s, &c);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const real a = Rn[r * 3 + 0], b = Rn[r * 3 + 1];
                Rn[r * 3 + 0] = a * c + b * s;
                Rn[r * 3 + 1] = b * c - a * s;
            }
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = Rn[i];
        real* o = col + (size_t)(j + 1) * 3 * 64;
        o[0] = p[0]; o[64] = p[1]; o[128] = p[2];
    }
}

template <typename real>
struct ValidateK {
    int T, n_sub;
    const ChainDev* chain;            // DEVICE, or null: no link columns
    int n_links;
    const real* spheres;              // DEVICE [n_spheres][4], or null
    int n_spheres;
    unsigned pair_mask[SGPMP_MAX_LINKS];   // bit j of word i: pair (i, j) counts for the self-clearance
    int has_qlim, has_vlim, has_grid;
    real q_lo[SGPMP_MAX_DOF], q_hi[SGPMP_MAX_DOF], v_max[SGPMP_MAX_DOF];
    TermK<real> grid;
};

// (value, fine index) candidates: smaller (MIN) or larger value wins, equal values go to the lower index; index -1 = none yet
template <bool MIN, typename real>
__device__ __forceinline__ void take(real& v, int& f, real cv, int cf) {
    const bool better = MIN ? (cv < v) : (cv > v);
    if (better || (cv == v && (unsigned)cf < (unsigned)f)) { v = cv; f = cf; }
}
template <bool MIN, typename real>
__device__ __forceinline__ void wave_take(real& v, int& f) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const real ov = __shfl_xor(v, off, 64);
        const int of = __shfl_xor(f, off, 64);
        take<MIN, real>(v, f, ov, of);
    }
}

template <typename real, int N>
__global__ void __launch_bounds__(64)
validate_kernel(const real* __restrict__ trajs, long long batch, ValidateK<real> A, HermiteK<real> H, real* __restrict__ values,
                int* __restrict__ where) {
    using O = RealOps<real>;
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int lane = threadIdx.x;
    real* col = reinterpret_cast<real*>(lds_raw) + lane;      // this lane's column of link positions (SoA, stride 64)
    const int T = A.T, k1 = A.n_sub + 1;
    const real inf = std::numeric_limits<real>::infinity(), big = std::numeric_limits<real>::max();
    for (long long b = blockIdx.x; b < batch; b += gridDim.x) {
        const real* tr = trajs + (size_t)b * T * (2 * N);
        real v_obs = inf, v_self = inf, v_lim = -inf, v_occ = -inf;
        int f_obs = -1, f_self = -1, f_lim = -1, f_occ = -1;
        int f_bad = 0x7fffffff;                                // first non-finite fine state of this lane
        for (int base = 0; base < T; base += 64) {
            const int i = base + lane;
            real a[2 * N], nb[2 * N], x[2 * N];
            load_interval<real, N>(tr, T, i, lane, a, nb);
            const int nm = i < T - 1 ? k1 : (i == T - 1 ? 1 : 0);
            for (int m = 0; m < nm; ++m) {
                if (m == 0) {
#pragma unroll
                    for (int k = 0; k < 2 * N; ++k) x[k] = a[k];
                } else {
                    hermite_state<real, N>(a, nb, H.c[m - 1], x);
                }
                const int f = i * k1 + m;
                // explicit tests: fmin / fmax drop a NaN, comparisons with one are all false
                bool finite = true;
#pragma unroll
                for (int k = 0; k < 2 * N; ++k) finite = finite && (fabs(x[k]) <= big);
                if (!finite) { f_bad = f < f_bad ? f : f_bad; continue; }
                if (A.has_qlim | A.has_vlim) {
                    real e = -inf;
#pragma unroll
                    for (int k = 0; k < N; ++k) {
                        if (A.has_qlim) {
                            const real lo = A.q_lo[k] - x[k], hi = x[k] - A.q_hi[k];
                            e = lo > e ? lo : e;
                            e = hi > e ? hi : e;
                        }
                        if (A.has_vlim) {
                            const real ve = fabs(x[N + k]) - A.v_max[k];
                            e = ve > e ? ve : e;
                        }
                    }
                    take<false, real>(v_lim, f_lim, e, f);
                }
                if (A.has_grid) take<false, real>(v_occ, f_occ, grid_value<real>(A.grid, x[0], x[N > 1 ? 1 : 0]), f);
                if (A.chain) {
                    const int L = A.n_links;
                    real q[N];
#pragma unroll
                    for (int k = 0; k < N; ++k) q[k] = x[k];
                    fk_points_const<real, N>(as_const(A.chain), L, q, col);
                    // sqrt and "- r" are monotone and correctly rounded, so the minimum is taken on the SQUARED distances and
                    // the root once per sphere / once for all pairs: the same bits as min over sqrt(d2) - r, 50 + 29 roots less
                    if (A.spheres) {
                        const SGPMP_CONST real* sph = as_const(A.spheres);       // uniform addresses: scalar loads
                        real dmin = inf;
                        for (int o = 0; o < A.n_spheres; ++o) {
                            const real cx = sph[o * 4 + 0], cy = sph[o * 4 + 1], cz = sph[o * 4 + 2], r = sph[o * 4 + 3];
                            real d2min = inf;
                            for (int l = 0; l < L; ++l) {
                                const real dx = col[(l * 3 + 0) * 64] - cx, dy = col[(l * 3 + 1) * 64] - cy,
                                           dz = col[(l * 3 + 2) * 64] - cz;
                                const real d2 = dx * dx + dy * dy + dz * dz;
                                d2min = d2 < d2min ? d2 : d2min;
                            }
                            const real dist = O::sqrt_(d2min) - r;
                            dmin = dist < dmin ? dist : dmin;
                        }
                        if (A.n_spheres > 0) take<true, real>(v_obs, f_obs, dmin, f);
                    }
                    real smin = inf;
                    bool any = false;
                    for (int li = 2; li < L; ++li) {
                        const unsigned row = A.pair_mask[li];
                        if (!row) continue;
                        const real ax = col[(li * 3 + 0) * 64], ay = col[(li * 3 + 1) * 64], az = col[(li * 3 + 2) * 64];
                        for (int lj = 0; lj + 2 <= li; ++lj) {
                            if (!((row >> lj) & 1u)) continue;
                            const real dx = ax - col[(lj * 3 + 0) * 64], dy = ay - col[(lj * 3 + 1) * 64],
                                       dz = az - col[(lj * 3 + 2) * 64];
                            const real d2 = dx * dx + dy * dy + dz * dz;
                            smin = d2 < smin ? d2 : smin;
                            any = true;
                        }
                    }
                    if (any) smin = O::sqrt_(smin);
                    if (any) take<true, real>(v_self, f_self, smin, f);
                }
            }
        }
        wave_take<true, real>(v_obs, f_obs);
        wave_take<true, real>(v_self, f_self);
        wave_take<false, real>(v_lim, f_lim);
        wave_take<false, real>(v_occ, f_occ);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const int o = __shfl_xor(f_bad, off, 64);
            f_bad = o < f_bad ? o : f_bad;
        }
        if (lane == 0) {
            real* vo = values + (size_t)b * 4;
            int* wo = where + (size_t)b * 4;
            if (f_bad != 0x7fffffff) {
                const real nan = std::numeric_limits<real>::quiet_NaN();
                vo[0] = nan; vo[1] = nan; vo[2] = nan; vo[3] = nan;
                wo[0] = f_bad; wo[1] = f_bad; wo[2] = f_bad; wo[3] = f_bad;
            } else {
                vo[0] = v_obs; vo[1] = v_self; vo[2] = v_lim; vo[3] = v_occ;
                wo[0] = f_obs; wo[1] = f_self; wo[2] = f_lim; wo[3] = f_occ;
            }
        }
    }
}

// ---------------------------------------------------------------------------------- launchers
static unsigned dense_blocks(long long batch) {               // one wave per trajectory; beyond 2^20 waves a block takes several
    return (unsigned)(batch < (1ll << 20) ? batch : (1ll << 20));
}

template <typename real>
static hipError_t launch_interpolate(int n, int T, const void* trajs, long long batch, int n_sub, double dt, void* out,
                                     hipStream_t stream) {
    const HermiteK<real> H = hermite_coefs<real>(n_sub, dt);
#define DENSE_CASE(NN)                                                                                               \
    case NN:                                                                                                         \
        hipLaunchKernelGGL((interpolate_kernel<real, NN>), dim3(dense_blocks(batch)), dim3(64), 0, stream,           \
                           (const real*)trajs, batch, T, n_sub, H, (real*)out);                                      \
        break;
    switch (n) {
        DENSE_CASE(1) DENSE_CASE(2) DENSE_CASE(3) DENSE_CASE(4) DENSE_CASE(5) DENSE_CASE(6) DENSE_CASE(7) DENSE_CASE(8)
        default: return hipErrorInvalidValue;
    }
#undef DENSE_CASE
    return hipGetLastError();
}

template <typename real>
static TermK<real> grid_termk(const CostTerm& s) {             // the fields grid_value reads
    TermK<real> k;
    std::memset(&k, 0, sizeof(k));
    k.kind = s.kind; k.flags = s.flags;
    k.inv_cell = (real)s.inv_cell; k.off_x = (real)s.off_x; k.off_y = (real)s.off_y;
    k.dev_data = s.dev_data; k.dim0 = s.dim0; k.dim1 = s.dim1;
    return k;
}

template <typename real>
static hipError_t launch_validate(const SgpmpCtxView& v, const void* trajs, long long batch, int n_sub, double dt,
                                  const void* spheres, int n_spheres, const CostTerm* grid, const double* q_lo,
                                  const double* q_hi, const double* v_max, void* values, int32_t* where, hipStream_t stream) {
    const int n = v.dims.n_dof;
    ValidateK<real> A;
    std::memset(&A, 0, sizeof(A));
    A.T = v.dims.traj_len; A.n_sub = n_sub;
    size_t lds = 0;
    if (v.have_chain) {
        A.chain = v.d_chain;
        A.n_links = v.h_chain->n_links;
        for (int i = 0; i < SGPMP_MAX_LINKS; ++i) A.pair_mask[i] = v.pair_mask[i];
        if (spheres && n_spheres > 0) { A.spheres = (const real*)spheres; A.n_spheres = n_spheres; }
        lds = (size_t)A.n_links * 3 * 64 * sizeof(real);
    }
    const real inf = std::numeric_limits<real>::infinity();
    A.has_qlim = (q_lo || q_hi) ? 1 : 0;
    A.has_vlim = v_max ? 1 : 0;
    for (int k = 0; k < SGPMP_MAX_DOF; ++k) {                  // a one-sided position limit: the other side never binds
        A.q_lo[k] = (q_lo && k < n) ? (real)q_lo[k] : -inf;
        A.q_hi[k] = (q_hi && k < n) ? (real)q_hi[k] : inf;
        A.v_max[k] = (v_max && k < n) ? (real)v_max[k] : inf;
    }
    if (grid) { A.has_grid = 1; A.grid = grid_termk<real>(*grid); }
    const HermiteK<real> H = hermite_coefs<real>(n_sub, dt);
#define DENSE_CASE(NN)                                                                                               \
    case NN:                                                                                                         \
        hipLaunchKernelGGL((validate_kernel<real, NN>), dim3(dense_blocks(batch)), dim3(64), lds, stream,            \
                           (const real*)trajs, batch, A, H, (real*)values, (int*)where);                             \
        break;
    switch (n) {
        DENSE_CASE(1) DENSE_CASE(2) DENSE_CASE(3) DENSE_CASE(4) DENSE_CASE(5) DENSE_CASE(6) DENSE_CASE(7) DENSE_CASE(8)
        default: return hipErrorInvalidValue;
    }
#undef DENSE_CASE
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------- entry points
static int dense_hip_error(const char* what, hipError_t e) {
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", what, hipGetErrorString(e));
    return sgpmp_set_error(SGPMP_EHIP, msg);
}

extern "C" int sgpmp_interpolate(sgpmp_ctx* c, const void* trajs, int64_t batch, int n_sub, double dt, void* out,
                                 void* stream) {
    if (!c || batch < 0 || n_sub < 0 || n_sub > SGPMP_MAX_SUBSTEPS || !(dt > 0.) || (batch > 0 && (!trajs || !out)))
        return sgpmp_set_error(SGPMP_EINVAL, "sgpmp_interpolate: bad argument (n_sub in [0, 31], dt > 0, non-null buffers)");
    if (batch == 0) return SGPMP_OK;
    SgpmpCtxView v;
    sgpmp_ctx_view(c, &v);                                     // (dims only: the state of the cost program does not matter here)
    const hipError_t e = v.dims.dtype == SGPMP_F64
        ? launch_interpolate<double>(v.dims.n_dof, v.dims.traj_len, trajs, batch, n_sub, dt, out, (hipStream_t)stream)
        : launch_interpolate<float>(v.dims.n_dof, v.dims.traj_len, trajs, batch, n_sub, dt, out, (hipStream_t)stream);
    return e == hipSuccess ? SGPMP_OK : dense_hip_error("sgpmp_interpolate", e);
}

extern "C" int sgpmp_validate(sgpmp_ctx* c, const void* trajs, int64_t batch, int n_sub, double dt, const void* spheres,
                              int n_spheres, int grid_term, const double* q_lo, const double* q_hi, const double* v_max,
                              void* values, int32_t* where, void* stream) {
    if (!c || batch < 0 || n_sub < 0 || n_sub > SGPMP_MAX_SUBSTEPS || !(dt > 0.) || n_spheres < 0 ||
        (batch > 0 && (!trajs || !values || !where)))
        return sgpmp_set_error(SGPMP_EINVAL, "sgpmp_validate: bad argument (n_sub in [0, 31], dt > 0, non-null buffers)");
    SgpmpCtxView v;
    const int view_rc = sgpmp_ctx_view(c, &v);
    const CostTerm* grid = nullptr;
    if (grid_term >= 0) {
        if (!v.prog && view_rc != SGPMP_OK) return view_rc;    // (finalize_program said why)
        if (!v.prog || grid_term >= v.prog->n_terms || v.prog->terms[grid_term].kind != SGPMP_COST_GRID)
            return sgpmp_set_error(SGPMP_EINVAL, "sgpmp_validate: grid_term is not a grid term");
        grid = &v.prog->terms[grid_term];
    } else if (grid_term != -1) {
        return sgpmp_set_error(SGPMP_EINVAL, "sgpmp_validate: grid_term is not a grid term");
    }
    if (spheres && n_spheres > 0 && !v.have_chain)
        return sgpmp_set_error(SGPMP_ESTATE, "sgpmp_validate: obstacle spheres need an FK chain (sgpmp_set_fk)");
    if (batch == 0) return SGPMP_OK;
    const hipError_t e = v.dims.dtype == SGPMP_F64
        ? launch_validate<double>(v, trajs, batch, n_sub, dt, spheres, n_spheres, grid, q_lo, q_hi, v_max, values, where,
                                  (hipStream_t)stream)
        : launch_validate<float>(v, trajs, batch, n_sub, dt, spheres, n_spheres, grid, q_lo, q_hi, v_max, values, where,
                                 (hipStream_t)stream);
    return e == hipSuccess ? SGPMP_OK : dense_hip_error("sgpmp_validate", e);
}

// ---------------------------------------------------------------------------------- sgpmp_dense_cost
// The collision terms of the cost program on the INSERTED fine states (the support states stay with the sweep) and a quadratic
// joint / velocity limit penalty on ALL fine states, summed per trajectory.  validate_kernel's mapping -- one wave per
// trajectory, one lane per support waypoint, the lane walks its interval -- and the same hermite_state; each lane sums its
// states in the compute type, the wave sum and the add into what `costs64` holds are in double.  Three instantiations:
//   MODE 2  built-in Panda code: fk_cg / spheres_field_cg / self_field_cg in registers, the sphere terms of the links that
//           never move once per wave (an LDS word per term) -- the sweep's FKMODE 1000 code, picked by launch_cost's conditions;
//   MODE 1  generic: any chain, interpolated points; link positions in one LDS column per lane (fk_points_const, add_interp_points,
//           spheres_field, self_field), as in validate_kernel;
//   MODE 0  no link field (planar GRID programs, limits only): no LDS.
template <typename real>
struct DenseCostK {
    int T, n_sub;
    const ChainDev* chain;            // DEVICE (MODE 1), or null
    int n_links;
    const real* spheres;              // DEVICE [n_spheres][4], or null
    int n_spheres;
    int n_terms;                      // GRID / SPHERES / SELF terms of the cost program, in program order
    int has_qlim, has_vlim, accumulate;
    real weight, inv_sigma2;
    real q_lo[SGPMP_MAX_DOF], q_hi[SGPMP_MAX_DOF], v_max[SGPMP_MAX_DOF];
    TermK<real> t[SGPMP_MAX_TERMS];
};
// (HIP passes at most 4 KiB of kernel arguments)
static_assert(sizeof(DenseCostK<double>) + sizeof(HermiteK<double>) + 4 * sizeof(void*) <= 4096, "dense_cost_kernel: kernel arguments");

template <typename real, int N, int MODE>
__global__ void __launch_bounds__(64)
dense_cost_kernel(const real* __restrict__ trajs, long long batch, DenseCostK<real> A, HermiteK<real> H, real* __restrict__ costs,
                  double* __restrict__ costs64) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int lane = threadIdx.x;
    const int T = A.T, k1 = A.n_sub + 1;
    const real big = std::numeric_limits<real>::max();
    __shared__ real stat[MODE == 2 ? SGPMP_MAX_TERMS : 1];     // MODE 2: sphere terms of the static links
    // Once per BLOCK, outside the trajectory loop: the static links and their sphere terms do not depend on the trajectory.  The
    // cost (one forward kinematics and the spheres x static links on all 64 lanes) is amortised only over the trajectories
    // this block serves -- ONE while dense_blocks hands out a block per trajectory (batch < 2^20); it is part of the call's
    // fixed time.  Whoever gives a block several trajectories gets it cheaper, not wrong.
    if constexpr (MODE == 2) {
        using CC = ChainCode_panda;
        real q0[CC::N], P0[CC::NREP][3];
#pragma unroll
        for (int k = 0; k < CC::N; ++k) q0[k] = 0;
        fk_cg<real, CC>(q0, P0);                               // static links do not depend on q
        for (int ti = 0; ti < A.n_terms; ++ti) {
            const TermK<real>& tm = A.t[ti];
            if (tm.kind != SGPMP_COST_SPHERES) continue;
            const real init = ((tm.flags & 15) == SGPMP_FIELD_SDF) ? (real)-1e30 : (real)0;
            const real v = spheres_field_cg<real, CC, true>(tm, P0, A.spheres, A.n_spheres, init);
            if (lane == 0) stat[ti] = v;
        }
        __syncthreads();
    }
    for (long long b = blockIdx.x; b < batch; b += gridDim.x) {
        const real* tr = trajs + (size_t)b * T * (2 * N);
        real part = 0, lim = 0;
        bool bad = false;
        for (int base = 0; base < T; base += 64) {
            const int i = base + lane;
            real a[2 * N], nb[2 * N], x[2 * N];
            load_interval<real, N>(tr, T, i, lane, a, nb);
            const int nm = i < T - 1 ? k1 : (i == T - 1 ? 1 : 0);
            for (int m = 0; m < nm; ++m) {
                if (m == 0) {
#pragma unroll
                    for (int k = 0; k < 2 * N; ++k) x[k] = a[k];
                } else {
                    hermite_state<real, N>(a, nb, H.c[m - 1], x);
                }
                // explicit test: fmin / fmax drop a NaN, comparisons with one are all false
                bool finite = true;
#pragma unroll
                for (int k = 0; k < 2 * N; ++k) finite = finite && (fabs(x[k]) <= big);
                if (!finite) { bad = true; continue; }
                if (A.has_qlim | A.has_vlim) {
#pragma unroll
                    for (int k = 0; k < N; ++k) {
                        if (A.has_qlim) {
                            const real lo = A.q_lo[k] - x[k], hi = x[k] - A.q_hi[k];
                            if (lo > 0) lim += lo * lo;
                            if (hi > 0) lim += hi * hi;
                        }
                        if (A.has_vlim) {
                            const real ve = fabs(x[N + k]) - A.v_max[k];
                            if (ve > 0) lim += ve * ve;
                        }
                    }
                }
                if (m == 0) continue;                          // a support state: its collision cost is the sweep's
                if constexpr (MODE == 2) {
                    using CC = ChainCode_panda;
                    real q[N], Pq[CC::NREP][3];
#pragma unroll
                    for (int k = 0; k < N; ++k) q[k] = x[k];
                    fk_cg<real, CC>(q, Pq);
                    for (int ti = 0; ti < A.n_terms; ++ti) {
                        const TermK<real>& tm = A.t[ti];
                        real f;
                        if (tm.kind == SGPMP_COST_SPHERES)
                            f = spheres_field_cg<real, CC, false>(tm, Pq, A.spheres, A.n_spheres, stat[ti]);
                        else if (tm.kind == SGPMP_COST_SELF)
                            f = self_field_cg<real, CC>(tm, Pq);
                        else
                            f = grid_value<real>(tm, x[0], x[N > 1 ? 1 : 0]);
                        part += tm.K * f;
                    }
                } else {
                    if constexpr (MODE == 1) {
                        real* col = reinterpret_cast<real*>(lds_raw) + lane;   // this lane's column of points (SoA, stride 64)
                        real q[N];
#pragma unroll
                        for (int k = 0; k < N; ++k) q[k] = x[k];
                        fk_points_const<real, N>(as_const(A.chain), A.n_links, q, col);
                        for (int ti = 0; ti < A.n_terms; ++ti) {
                            const TermK<real>& tm = A.t[ti];
                            if (tm.kind == SGPMP_COST_GRID) continue;
                            if (tm.n_interp > 0) add_interp_points<real>(tm, A.n_links, col, 64);
                            const real f = tm.kind == SGPMP_COST_SPHERES
                                ? spheres_field<real>(tm, tm.n_points, col, 64, A.spheres, A.n_spheres)
                                : self_field<real>(tm, tm.n_points, col, 64);
                            part += tm.K * f;
                        }
                    }
                    for (int ti = 0; ti < A.n_terms; ++ti) {
                        const TermK<real>& tm = A.t[ti];
                        if (tm.kind == SGPMP_COST_GRID) part += tm.K * grid_value<real>(tm, x[0], x[N > 1 ? 1 : 0]);
                    }
                }
            }
        }
        double acc = wave_sum((double)(A.weight * part) + (double)(A.inv_sigma2 * lim));
        const bool any_bad = __any(bad ? 1 : 0) != 0;
        if (lane == 0) {
            if (any_bad) acc = std::numeric_limits<double>::quiet_NaN();
            if (A.accumulate) acc += costs64 ? costs64[b] : (double)costs[b];   // (both given: costs64 is the accumulator, costs its rounding)
            if (costs64) costs64[b] = acc;
            if (costs) costs[b] = (real)acc;
        }
    }
}

static thread_local const char* g_last_dense_kernel = "";
extern "C" const char* sgpmp_last_dense_kernel(void) { return g_last_dense_kernel; }

template <typename real>
static hipError_t launch_dense_cost(const SgpmpCtxView& v, const void* trajs, long long batch, int n_sub, double dt,
                                    const void* spheres, int n_spheres, double weight, const double* q_lo, const double* q_hi,
                                    const double* v_max, double sigma_limit, int accumulate, void* costs, double* costs64,
                                    hipStream_t stream) {
    constexpr bool f64 = sizeof(real) == 8;
    const char* name = "";
    // the name is published only once the launch has been accepted
    auto launched = [&]() { const hipError_t e = hipGetLastError(); if (e == hipSuccess) g_last_dense_kernel = name; return e; };
    const int n = v.dims.n_dof;
    DenseCostK<real> A;
    std::memset(&A, 0, sizeof(A));
    A.T = v.dims.traj_len; A.n_sub = n_sub; A.accumulate = accumulate ? 1 : 0;
    A.weight = (real)weight;
    bool fk = false, interp = false;
    int max_pts = 0;
    // weight 0 (the limit part alone) and n_sub 0 (no inserted state) evaluate no field at all
    for (int i = 0; v.prog && weight > 0. && n_sub > 0 && i < v.prog->n_terms; ++i) {
        const CostTerm& s = v.prog->terms[i];
        if (s.kind == SGPMP_COST_SPHERES && n_spheres < 1) continue;       // no obstacle: the term adds nothing
        if (s.kind != SGPMP_COST_GRID && s.kind != SGPMP_COST_SPHERES && s.kind != SGPMP_COST_SELF) continue;
        A.t[A.n_terms++] = make_termk<real>(s);
        if (s.kind != SGPMP_COST_GRID) {
            fk = true;
            interp = interp || s.n_interp > 0;
            max_pts = s.n_points > max_pts ? s.n_points : max_pts;
        }
    }
    const real inf = std::numeric_limits<real>::infinity();
    A.has_qlim = (q_lo || q_hi) ? 1 : 0;
    A.has_vlim = v_max ? 1 : 0;
    A.inv_sigma2 = (A.has_qlim | A.has_vlim) ? (real)(1. / (sigma_limit * sigma_limit)) : (real)0;
    for (int k = 0; k < SGPMP_MAX_DOF; ++k) {                  // a one-sided position limit: the other side never binds
        A.q_lo[k] = (q_lo && k < n) ? (real)q_lo[k] : -inf;
        A.q_hi[k] = (q_hi && k < n) ? (real)q_hi[k] : inf;
        A.v_max[k] = (v_max && k < n) ? (real)v_max[k] : inf;
    }
    const HermiteK<real> H = hermite_coefs<real>(n_sub, dt);
    const dim3 grid(dense_blocks(batch)), block(64);
    if (fk) {
        A.spheres = n_spheres > 0 ? (const real*)spheres : nullptr;
        A.n_spheres = A.spheres ? n_spheres : 0;
        A.n_links = v.h_chain->n_links;
        // launch_cost's conditions for the code built with the library
        const FkPlan& plan = v.h_chain->plan;
        const bool cg = plan.fast && plan.codegen_id == 1 && n == ChainCode_panda::N && !interp && !v.tg->force_generic_fk &&
                        !v.tg->no_chain_codegen;
        if (cg) {
            name = f64 ? "dense_cost_kernel<f64, generated chain>" : "dense_cost_kernel<f32, generated chain>";
            hipLaunchKernelGGL((dense_cost_kernel<real, ChainCode_panda::N, 2>), grid, block, 0, stream, (const real*)trajs,
                               batch, A, H, (real*)costs, costs64);
            return launched();
        }
        A.chain = v.d_chain;
        if (max_pts < A.n_links) max_pts = A.n_links;
        // finalize_program admits at most SGPMP_MAX_POINTS points per term: the columns take at most 48 KB
        static_assert((size_t)SGPMP_MAX_POINTS * 3 * 64 * sizeof(double) <= 48 * 1024, "dense_cost_kernel: LDS columns");
        if (max_pts > SGPMP_MAX_POINTS) return hipErrorInvalidValue;
        const size_t lds = (size_t)max_pts * 3 * 64 * sizeof(real);
        name = f64 ? "dense_cost_kernel<f64, generic FK>" : "dense_cost_kernel<f32, generic FK>";
#define DENSE_CASE(NN)                                                                                               \
    case NN:                                                                                                         \
        hipLaunchKernelGGL((dense_cost_kernel<real, NN, 1>), grid, block, lds, stream, (const real*)trajs, batch, A, \
                           H, (real*)costs, costs64);                                                                \
        break;
        switch (n) {
            DENSE_CASE(1) DENSE_CASE(2) DENSE_CASE(3) DENSE_CASE(4) DENSE_CASE(5) DENSE_CASE(6) DENSE_CASE(7) DENSE_CASE(8)
            default: return hipErrorInvalidValue;
        }
#undef DENSE_CASE
        return launched();
    }
    name = f64 ? "dense_cost_kernel<f64, no FK>" : "dense_cost_kernel<f32, no FK>";
#define DENSE_CASE(NN)                                                                                               \
    case NN:                                                                                                         \
        hipLaunchKernelGGL((dense_cost_kernel<real, NN, 0>), grid, block, 0, stream, (const real*)trajs, batch, A,   \
                           H, (real*)costs, costs64);                                                                \
        break;
    switch (n) {
        DENSE_CASE(1) DENSE_CASE(2) DENSE_CASE(3) DENSE_CASE(4) DENSE_CASE(5) DENSE_CASE(6) DENSE_CASE(7) DENSE_CASE(8)
        default: return hipErrorInvalidValue;
    }
#undef DENSE_CASE
    return launched();
}

extern "C" int sgpmp_dense_cost(sgpmp_ctx* c, const void* trajs, int64_t batch, int n_sub, double dt, const void* spheres,
                                int n_spheres, double weight, const double* q_lo, const double* q_hi, const double* v_max,
                                double sigma_limit, int accumulate, void* costs, double* costs64, void* stream) {
    const bool limits = q_lo || q_hi || v_max;
    if (!c || batch < 0 || n_sub < 0 || n_sub > SGPMP_MAX_SUBSTEPS || !(dt > 0.) || !(weight >= 0.) || n_spheres < 0 ||
        (limits && !(sigma_limit > 0.)) || (batch > 0 && (!trajs || (!costs && !costs64))))
        return sgpmp_set_error(SGPMP_EINVAL, "sgpmp_dense_cost: bad argument (n_sub in [0, 31], dt > 0, weight >= 0, "
                                             "sigma_limit > 0 with limits, non-null trajs and one output)");
    SgpmpCtxView v;
    const int view_rc = sgpmp_ctx_view(c, &v);
    if (view_rc != SGPMP_OK) return view_rc;                   // (finalize_program said why)
    for (int i = 0; v.prog && i < v.prog->n_terms; ++i) {
        const int kind = v.prog->terms[i].kind;
        if ((kind == SGPMP_COST_SPHERES || kind == SGPMP_COST_SELF) && !v.have_chain)
            return sgpmp_set_error(SGPMP_ESTATE, "sgpmp_dense_cost: link-field terms need an FK chain (sgpmp_set_fk)");
        if (kind == SGPMP_COST_SPHERES && n_spheres > 0 && !spheres)
            return sgpmp_set_error(SGPMP_ESTATE, "sgpmp_dense_cost: n_spheres > 0 without obstacle spheres");
    }
    if (batch == 0) return SGPMP_OK;
    const hipError_t e = v.dims.dtype == SGPMP_F64
        ? launch_dense_cost<double>(v, trajs, batch, n_sub, dt, spheres, n_spheres, weight, q_lo, q_hi, v_max, sigma_limit,
                                    accumulate, costs, costs64, (hipStream_t)stream)
        : launch_dense_cost<float>(v, trajs, batch, n_sub, dt, spheres, n_spheres, weight, q_lo, q_hi, v_max, sigma_limit,
                                   accumulate, costs, costs64, (hipStream_t)stream);
    return e == hipSuccess ? SGPMP_OK : dense_hip_error("sgpmp_dense_cost", e);
}
