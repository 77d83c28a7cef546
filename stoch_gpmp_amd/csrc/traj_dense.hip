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

// hermite_coefs as a plain table real[SGPMP_MAX_SUBSTEPS][8] of the context's dtype, for gpmp_dense.hip's rows
void hermite_table(int dtype, int n_sub, double dt, void* out) {
    if (dtype == SGPMP_F64) { const HermiteK<double> H = hermite_coefs<double>(n_sub, dt); std::memcpy(out, &H, sizeof(H)); }
    else { const HermiteK<float> H = hermite_coefs<float>(n_sub, dt); std::memcpy(out, &H, sizeof(H)); }
}

// the particle means on the fine grid for sgpmp_gpmp_linearize (api.hip): the launch of sgpmp_interpolate
hipError_t launch_gpmp_fine(int dtype, int n, int T, const void* means, long long P, int n_sub, double dt, void* fine,
                            hipStream_t stream) {
    return dtype == SGPMP_F64 ? launch_interpolate<double>(n, T, means, P, n_sub, dt, fine, stream)
                              : launch_interpolate<float>(n, T, means, P, n_sub, dt, fine, stream);
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

// The dense-trajectory kernels do not evaluate SGPMP_COST_VOXEL_SDF, SGPMP_COST_BODY_SDF or SGPMP_COST_BODY_SELF: a cost list that holds the term is refused by name, never
// evaluated without it (which would drop a collision term).  -> the message, or null.
static const char* voxel_term_refusal(const char* who, const SgpmpCtxView& v) {
    static thread_local char msg[200];
    for (int i = 0; v.prog && i < v.prog->n_terms; ++i)
        if (v.prog->terms[i].kind == SGPMP_COST_VOXEL_SDF) {
            snprintf(msg, sizeof(msg), "%s: cost term %d (SGPMP_COST_VOXEL_SDF) is not evaluated on dense trajectories; "
                                       "the voxel distance term counts at the support waypoints only", who, i);
            return msg;
        } else if (v.prog->terms[i].kind == SGPMP_COST_BODY_SDF) {          // (the same holds for the body's spheres on that field)
            snprintf(msg, sizeof(msg), "%s: cost term %d (SGPMP_COST_BODY_SDF) is not evaluated on dense trajectories; "
                                       "the body distance term counts at the support waypoints only", who, i);
            return msg;
        } else if (v.prog->terms[i].kind == SGPMP_COST_BODY_SELF) {         // (and for the body's sphere pairs)
            snprintf(msg, sizeof(msg), "%s: cost term %d (SGPMP_COST_BODY_SELF) is not evaluated on dense trajectories; "
                                       "the body self-distance term counts at the support waypoints only", who, i);
            return msg;
        }
    return nullptr;
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
    if (const char* refused = voxel_term_refusal("sgpmp_validate", v)) return sgpmp_set_error(SGPMP_EINVAL, refused);
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
    int n_terms;                      // GRID / GRID_SDF / SPHERES / SELF terms of the cost program, in program order
    int has_qlim, has_vlim, accumulate;
    real weight, inv_sigma2;
    real q_lo[SGPMP_MAX_DOF], q_hi[SGPMP_MAX_DOF], v_max[SGPMP_MAX_DOF];
    TermK<real> t[SGPMP_MAX_TERMS];
};
// (HIP passes at most 4 KiB of kernel arguments)
static_assert(sizeof(DenseCostK<double>) + sizeof(HermiteK<double>) + 4 * sizeof(void*) <= 4096, "dense_cost_kernel: kernel arguments");

// a term of the planar point itself: the occupancy lookup or the signed-distance grid's hinge
template <typename real>
__device__ __forceinline__ real planar_field(const TermK<real>& tm, real x, real y) {
    return tm.kind == SGPMP_COST_GRID_SDF ? grid_sdf_field<real, false>(tm, x, y, nullptr, nullptr)
                                          : grid_value<real>(tm, x, y);
}

// ... and the hinge with its derivative, for dense_cost_grad_kernel (a plain call there: the kernel's text is also compiled
// without this header's functions, tests/test_cpu_dense_grad_wave.py, where the branch that calls it is never instantiated)
template <typename real>
__device__ __forceinline__ real grid_sdf_force(const TermK<real>& tm, real x, real y, real* fx, real* fy) {
    return grid_sdf_field<real, true>(tm, x, y, fx, fy);
}

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
                            f = planar_field<real>(tm, x[0], x[N > 1 ? 1 : 0]);
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
                            if (tm.kind == SGPMP_COST_GRID || tm.kind == SGPMP_COST_GRID_SDF) continue;
                            if (tm.n_interp > 0) add_interp_points<real>(tm, A.n_links, col, 64);
                            const real f = tm.kind == SGPMP_COST_SPHERES
                                ? spheres_field<real>(tm, tm.n_points, col, 64, A.spheres, A.n_spheres)
                                : self_field<real>(tm, tm.n_points, col, 64);
                            part += tm.K * f;
                        }
                    }
                    for (int ti = 0; ti < A.n_terms; ++ti) {
                        const TermK<real>& tm = A.t[ti];
                        if (tm.kind == SGPMP_COST_GRID || tm.kind == SGPMP_COST_GRID_SDF)
                            part += tm.K * planar_field<real>(tm, x[0], x[N > 1 ? 1 : 0]);
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
        if (s.kind != SGPMP_COST_GRID && s.kind != SGPMP_COST_GRID_SDF && s.kind != SGPMP_COST_SPHERES && s.kind != SGPMP_COST_SELF)
            continue;
        A.t[A.n_terms++] = make_termk<real>(s);
        if (s.kind != SGPMP_COST_GRID && s.kind != SGPMP_COST_GRID_SDF) {
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
    if (const char* refused = voxel_term_refusal("sgpmp_dense_cost", v)) return sgpmp_set_error(SGPMP_EINVAL, refused);
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

// ---------------------------------------------------------------------------------- sgpmp_dense_cost_grad
// Value and gradient, with respect to the SUPPORT states, of sgpmp_dense_cost's sum (optionally with the SPHERES / SELF terms on
// the support waypoints 1 .. T-1 as well).  dense_cost_kernel's mapping and the same hermite_state; per fine state the lane runs
//   1. forward kinematics that keeps, per joint, the axis z_j (third column of the link's rotation -- the rotation about z that
//      follows leaves it unchanged); the joint origin o_j is the link position P[j + 1] itself, so field_grad_kernel's separate
//      origin array is not needed;
//   2. the forces g_l = sum over terms K_term d field / d p_l on the LINK points: a term's interpolated points are never stored,
//      each is formed from its two links when it is read and hands its force back to them (1 - alpha, alpha);
//   3. field_grad_kernel's backward recurrence from the end effector, d f / d q_j = z_j . (M_j - o_j x F_j), F and M in double;
//   4. the adjoint of hermite_state: (g_q, g_v) of the state times the eight coefficients that formed it, into `ga` (own row i)
//      and `gb` (row i + 1).  Row i of the result is ga(lane i) + gb(lane i - 1): one __shfl_up per pass, lane 63's gb carried
//      to lane 0 of the next pass in a register.  Lane i stores row i: every element is written once, by one lane, no atomics.
// Where the points, forces and axes live: one LDS column per lane (SoA, stride 64, as MODE 1 of dense_cost_kernel) -- G of the L
// links in double, P of the L links and Z of the L - 1 joints in the compute type.  Independent of the number of interpolated
// points, so the Panda (L = 11) takes 32 KB in fp32 and 48 KB in fp64 whatever num_interpolate is; a chain beyond the 64 KB a workgroup may
// ask for is refused by the host.  Registers were the first choice and do not hold them: next to the lane's six state / adjoint
// rows of 2N reals (a, b, x, ga, gb, carry) and g_q, g_v, q, dq the 96 reals of a 10-joint chain pushed the fp32 instantiation
// past the 512 registers of a one-wave workgroup (880 bytes of scratch per lane; fp64 1.3 KB), and scratch is slower than LDS.
//   NJ > 0   chain length known at compile time (10: the Panda, 7), no interpolated points: the loops over links and pairs
//            unroll, every LDS address is an immediate offset;
//   NJ = 0   any chain, any term;
//   NJ = -1  no link field (limits only): no LDS.
// A non-finite fine state turns the trajectory's value and its whole gradient into NaN.  With T <= 64 the wave knows before its
// one store; with more passes a first sweep over the fine states (hermite_state alone, no kinematics) finds out beforehand, so
// that rows stored by an early pass never have to be written a second time.
#define SGPMP_GRAD_LDS_MAX (64 * 1024)

// this lane's columns, stride 64: G [L][3] in DOUBLE (gcol), then P [L][3] | Z [L - 1][3] in the compute type (col).  NJ > 0:
// L = NJ + 1 at compile time, no interpolated points.  The forces are summed in double in fp32 kernels too: the pair forces of
// the self field are equal and opposite, up to ~1e5 each with points a few centimetres apart, and what is left of them in a
// link's sum is the gradient -- in fp32 sums the rounding of the large partial sums (~1e-2) was more than a small true gradient.
template <typename real, int NJ>
struct GradCols {
    static constexpr bool FIXED = NJ > 0;
    static constexpr int UNROLL = (NJ > 0 && sizeof(real) == 4) ? 64 : 1;   // (fp64, unrolled: 116 bytes of scratch at NJ = 10)
    double* gcol;
    real* col;
    int L;
    __device__ __forceinline__ int links() const { return FIXED ? NJ + 1 : L; }
    __device__ __forceinline__ real p(int l, int r) const { return col[(l * 3 + r) * 64]; }
    __device__ __forceinline__ double g(int l, int r) const { return gcol[(l * 3 + r) * 64]; }
    __device__ __forceinline__ real z(int j, int r) const { return col[((links() + j) * 3 + r) * 64]; }
    __device__ __forceinline__ void set_p(int l, int r, real v) { col[(l * 3 + r) * 64] = v; }
    __device__ __forceinline__ void set_g(int l, int r, double v) { gcol[(l * 3 + r) * 64] = v; }
    __device__ __forceinline__ void set_z(int j, int r, real v) { col[((links() + j) * 3 + r) * 64] = v; }
};
// bytes of dynamic LDS of a chain of L links
template <typename real>
static size_t grad_lds_bytes(int L) { return (size_t)L * 3 * 64 * sizeof(double) + (size_t)(2 * L - 1) * 3 * 64 * sizeof(real); }

// fk_points_const's operations in the same order, keeping each joint's axis; the forces are cleared on the way
template <typename real, int N, class S>
__device__ __forceinline__ void fk_points_axes(ChainC chain, const real (&q)[N], S& s) {
    using O = RealOps<real>;
    real R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    real p[3] = {0, 0, 0};
    const int nj = s.links() - 1;
#pragma unroll
    for (int r = 0; r < 3; ++r) { s.set_p(0, r, 0); s.set_g(0, r, 0); }
#pragma unroll S::UNROLL
    for (int j = 0; j < nj; ++j) {
        ChainC ch = opaque(chain);                             // this joint's constants: loaded here, not hoisted and spilled
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
            real sn, cs;
            O::sincos_(qv, &sn, &cs);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const real a = Rn[r * 3 + 0], b = Rn[r * 3 + 1];
                Rn[r * 3 + 0] = a * cs + b * sn;
                Rn[r * 3 + 1] = b * cs - a * sn;
            }
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = Rn[i];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            s.set_p(j + 1, r, p[r]);
            s.set_g(j + 1, r, 0);
            s.set_z(j, r, Rn[r * 3 + 2]);
        }
    }
}

// Point `idx` of a term: a link, or (idx >= L) the interpolated point `ai` between links li and li + 1 (add_interp_points' formula)
template <typename real, class S>
__device__ __forceinline__ void grad_point(const S& s, const TermK<real>& tm, int idx, int li, int ai, real (&p)[3]) {
    if (S::FIXED || idx < s.links()) {
#pragma unroll
        for (int r = 0; r < 3; ++r) p[r] = s.p(idx, r);
    } else {
        const real al = tm.alpha[ai];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const real a = s.p(li, r), b = s.p(li + 1, r);
            p[r] = a + (b - a) * al;
        }
    }
}
// The same point in double, from the stored link points: where the forces that grad_force folds back (1 - alpha, alpha) act
template <typename real, class S>
__device__ __forceinline__ void grad_point_exact(const S& s, const TermK<real>& tm, int idx, int li, int ai, double (&p)[3]) {
    if (S::FIXED || idx < s.links()) {
#pragma unroll
        for (int r = 0; r < 3; ++r) p[r] = (double)s.p(idx, r);
    } else {
        const double al = (double)tm.alpha[ai];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double a = (double)s.p(li, r), b = (double)s.p(li + 1, r);
            p[r] = a + (b - a) * al;
        }
    }
}
template <typename real, typename gtype, class S>
__device__ __forceinline__ void grad_force(S& s, const TermK<real>& tm, int idx, int li, int ai, const gtype (&g)[3]) {
    if (S::FIXED || idx < s.links()) {
#pragma unroll
        for (int r = 0; r < 3; ++r) s.set_g(idx, r, s.g(idx, r) + (double)g[r]);
    } else {
        const double al = (double)tm.alpha[ai];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            s.set_g(li, r, s.g(li, r) + (1.0 - al) * (double)g[r]);
            s.set_g(li + 1, r, s.g(li + 1, r) + al * (double)g[r]);
        }
    }
}
// the points of a term in order: links 0 .. L-1, then per link interval its interpolated points
#define GRAD_POINT_NEXT(S_, tm_, idx_, li_, ai_) \
    if (!S_::FIXED && (idx_) >= s.links()) { if (++(ai_) == (tm_).n_interp) { (ai_) = 0; ++(li_); } }

// K x (field value) of one SPHERES (rbf, sdf, clamped sdf) or SELF term; K x d field / d p_l is added to the forces
template <typename real, class S>
__device__ __forceinline__ real field_forces(S& s, const TermK<real>& tm, const SGPMP_CONST real* sph, int n_sph) {
    using O = RealOps<real>;
    const int np = S::FIXED ? s.links() : tm.n_points;
    const real K = tm.K;
    real val = 0;
    if (tm.kind == SGPMP_COST_SPHERES && (tm.flags & 15) == SGPMP_FIELD_SDF) {
        // field_grad_kernel's rule: the first maximum in point-major order, zero force where the clamp is active
        const bool clampv = (tm.flags & SGPMP_FLAG_SDF_CLAMP) != 0;
        real best = -std::numeric_limits<real>::infinity();
        int bl = 0;
        real bg[3] = {0, 0, 0};
#pragma unroll S::UNROLL
        for (int idx = 0, li = tm.interp_lo, ai = 0; idx < np; ++idx) {
            real p[3];
            grad_point<real, S>(s, tm, idx, li, ai, p);
            for (int o = 0; o < n_sph; ++o) {
                const real dx = p[0] - sph[o * 4], dy = p[1] - sph[o * 4 + 1], dz = p[2] - sph[o * 4 + 2];
                const real dist = O::sqrt_(dx * dx + dy * dy + dz * dz);
                real sd = sph[o * 4 + 3] - dist;
                const bool cut = clampv && sd > (real)0;
                if (cut) sd = 0;
                if (sd > best) {
                    best = sd; bl = idx;
                    const real w = cut ? (real)0 : -K / dist;
                    bg[0] = w * dx; bg[1] = w * dy; bg[2] = w * dz;
                }
            }
            GRAD_POINT_NEXT(S, tm, idx, li, ai)
        }
        val = best;
#pragma unroll S::UNROLL
        for (int idx = 0, li = tm.interp_lo, ai = 0; idx < np; ++idx) {     // (uniform walk: no lane-dependent index)
            if (idx == bl) grad_force<real>(s, tm, idx, li, ai, bg);
            GRAD_POINT_NEXT(S, tm, idx, li, ai)
        }
    } else if (tm.kind == SGPMP_COST_SPHERES) {                // rbf (the occupancy count is refused by the host)
#pragma unroll S::UNROLL
        for (int idx = 0, li = tm.interp_lo, ai = 0; idx < np; ++idx) {
            real p[3], g[3] = {0, 0, 0};
            grad_point<real, S>(s, tm, idx, li, ai, p);
            for (int o = 0; o < n_sph; ++o) {
                const real dx = p[0] - sph[o * 4], dy = p[1] - sph[o * 4 + 1], dz = p[2] - sph[o * 4 + 2], rr = sph[o * 4 + 3];
                const real ir2 = (real)1 / (rr * rr);
                const real e = O::exp_((real)-0.5 * (dx * dx + dy * dy + dz * dz) * ir2);
                val += e;
                const real w = -e * ir2;
                g[0] += w * dx; g[1] += w * dy; g[2] += w * dz;
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) g[r] *= K;
            grad_force<real>(s, tm, idx, li, ai, g);
            GRAD_POINT_NEXT(S, tm, idx, li, ai)
        }
    } else {                                                   // SELF: diagonal (1 each, no force) + twice the strict lower triangle
        val = (real)np;
        const real k4 = (real)4 * tm.K2 * K;
#pragma unroll S::UNROLL
        for (int i = 1, il = tm.interp_lo, ia = 0; i < np; ++i) {
            real pi[3];
            double pid[3], gi[3] = {0, 0, 0};
            grad_point<real, S>(s, tm, i, il, ia, pi);
            grad_point_exact<real, S>(s, tm, i, il, ia, pid);
#pragma unroll S::UNROLL
            for (int j = 0, jl = tm.interp_lo, ja = 0; j < i; ++j) {
                real pj[3];
                double pjd[3];
                grad_point<real, S>(s, tm, j, jl, ja, pj);
                grad_point_exact<real, S>(s, tm, j, jl, ja, pjd);
                const real dx = pi[0] - pj[0], dy = pi[1] - pj[1], dz = pi[2] - pj[2];
                const real e = O::exp_((dx * dx + dy * dy + dz * dz) * tm.K2);
                val += (real)2 * e;
                const real w = k4 * e;
                // the force along the difference of the two points IN DOUBLE, where the folded forces act: the pair's moment
                // (p_i - p_j) x g is then zero to double rounding, as it is in exact arithmetic, instead of |g| |p_i - p_j| 2^-24
                const double wd = (double)w;
                const double fx = wd * (pid[0] - pjd[0]), fy = wd * (pid[1] - pjd[1]), fz = wd * (pid[2] - pjd[2]);
                const double gj[3] = {-fx, -fy, -fz};
                gi[0] += fx; gi[1] += fy; gi[2] += fz;
                grad_force<real>(s, tm, j, jl, ja, gj);
                GRAD_POINT_NEXT(S, tm, j, jl, ja)
            }
            grad_force<real>(s, tm, i, il, ia, gi);
            GRAD_POINT_NEXT(S, tm, i, il, ia)
        }
    }
    return K * val;
}

// field_grad_kernel's backward recurrence from the end effector: dq[k] = sum over the revolute joints j of q_k of z_j . (M_j - o_j x F_j)
template <typename real, int N, class S>
__device__ __forceinline__ void joint_torques(ChainC chain, const S& s, real (&dq)[N]) {
    double Fs[3] = {0, 0, 0}, Ms[3] = {0, 0, 0};             // (double, as the forces: GradCols)
#pragma unroll
    for (int k = 0; k < N; ++k) dq[k] = 0;
    const int nj = s.links() - 1;
#pragma unroll S::UNROLL
    for (int j = nj - 1; j >= 0; --j) {
        ChainC ch = opaque(chain);
        const int l = j + 1;
        const double px = s.p(l, 0), py = s.p(l, 1), pz = s.p(l, 2), gx = s.g(l, 0), gy = s.g(l, 1), gz = s.g(l, 2);
        Fs[0] += gx; Fs[1] += gy; Fs[2] += gz;
        Ms[0] += py * gz - pz * gy;
        Ms[1] += pz * gx - px * gz;
        Ms[2] += px * gy - py * gx;
        if (ch->j[j].revolute) {
            const int qidx = ch->j[j].qidx;
            const double tx = Ms[0] - (py * Fs[2] - pz * Fs[1]);
            const double ty = Ms[1] - (pz * Fs[0] - px * Fs[2]);
            const double tz = Ms[2] - (px * Fs[1] - py * Fs[0]);
            const real d = (real)((double)s.z(j, 0) * tx + (double)s.z(j, 1) * ty + (double)s.z(j, 2) * tz);
#pragma unroll
            for (int k = 0; k < N; ++k) dq[k] += (qidx == k) ? d : (real)0;
        }
    }
}

static_assert(sizeof(DenseCostK<double>) + sizeof(HermiteK<double>) + 6 * sizeof(void*) <= 4096, "dense_cost_grad_kernel: kernel arguments");

// SDF (NJ = -1 only): the terms are signed-distance grid terms (SGPMP_COST_GRID_SDF) -- a field of the planar point (x[0], x[1])
// itself, its force goes onto entries 0 and 1 of the fine state; no kinematics, no LDS.
template <typename real, int N, int NJ, bool SDF = false>
__global__ void __launch_bounds__(64)
dense_cost_grad_kernel(const real* __restrict__ trajs, long long batch, DenseCostK<real> A, HermiteK<real> H, int support,
                       real* __restrict__ grad, real* __restrict__ costs, double* __restrict__ costs64) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int lane = threadIdx.x;
    const int T = A.T, k1 = A.n_sub + 1;
    const real big = std::numeric_limits<real>::max();
    const real two_is2 = (real)2 * A.inv_sigma2;
    for (long long b = blockIdx.x; b < batch; b += gridDim.x) {
        const real* tr = trajs + (size_t)b * T * (2 * N);
        real* gr = grad + (size_t)b * T * (2 * N);
        bool any_bad = false;
        if (T > 64) {                                          // several passes: know about a non-finite state before the first store
            bool bad = false;
#pragma unroll 1
            for (int base = 0; base < T; base += 64) {
                const int i = base + lane;
                real a[2 * N], nb[2 * N], x[2 * N];
                load_interval<real, N>(tr, T, i, lane, a, nb);
                const int nm = i < T - 1 ? k1 : (i == T - 1 ? 1 : 0);
#pragma unroll 1
                for (int m = 0; m < nm; ++m) {
                    if (m == 0) {
#pragma unroll
                        for (int k = 0; k < 2 * N; ++k) x[k] = a[k];
                    } else {
                        hermite_state<real, N>(a, nb, H.c[m - 1], x);
                    }
#pragma unroll
                    for (int k = 0; k < 2 * N; ++k) bad = bad || !(fabs(x[k]) <= big);
                }
            }
            any_bad = __any(bad ? 1 : 0) != 0;
        }
        real part = 0, lim = 0;
        real carry[2 * N];                                     // lane 63's gb of the previous pass (every lane holds it)
#pragma unroll
        for (int k = 0; k < 2 * N; ++k) carry[k] = 0;
#pragma unroll 1
        for (int base = 0; base < T; base += 64) {
            const int i = base + lane;
            real a[2 * N], nb[2 * N], x[2 * N], ga[2 * N], gb[2 * N];
            load_interval<real, N>(tr, T, i, lane, a, nb);
#pragma unroll
            for (int k = 0; k < 2 * N; ++k) { ga[k] = 0; gb[k] = 0; }
            const int nm = (any_bad || i >= T) ? 0 : (i < T - 1 ? k1 : 1);
            bool bad = false;
#pragma unroll 1
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
                real gq[N], gv[N];
#pragma unroll
                for (int k = 0; k < N; ++k) { gq[k] = 0; gv[k] = 0; }
                if (A.has_qlim | A.has_vlim) {                 // C^1: 2 / sigma^2 x the signed excess, zero inside the limits
#pragma unroll
                    for (int k = 0; k < N; ++k) {
                        if (A.has_qlim) {
                            const real lo = A.q_lo[k] - x[k], hi = x[k] - A.q_hi[k];
                            if (lo > 0) { lim += lo * lo; gq[k] -= two_is2 * lo; }
                            if (hi > 0) { lim += hi * hi; gq[k] += two_is2 * hi; }
                        }
                        if (A.has_vlim) {
                            const real ve = fabs(x[N + k]) - A.v_max[k];
                            if (ve > 0) { lim += ve * ve; gv[k] += x[N + k] < 0 ? -two_is2 * ve : two_is2 * ve; }
                        }
                    }
                }
                if constexpr (NJ >= 0) {
                    if (m > 0 || (support && i >= 1)) {        // inserted states; with `support`, waypoints 1 .. T-1 as well
                        real q[N], dq[N];
#pragma unroll
                        for (int k = 0; k < N; ++k) q[k] = x[k];
                        const SGPMP_CONST real* sph = as_const(A.spheres);
                        real f = 0;
                        GradCols<real, NJ> s = {reinterpret_cast<double*>(lds_raw) + lane,
                                                reinterpret_cast<real*>(lds_raw + (size_t)A.n_links * 3 * 64 * sizeof(double)) + lane,
                                                A.n_links};
                        fk_points_axes<real, N>(as_const(A.chain), q, s);
                        for (int ti = 0; ti < A.n_terms; ++ti) f += field_forces<real>(s, A.t[ti], sph, A.n_spheres);
                        joint_torques<real, N>(as_const(A.chain), s, dq);
                        part += f;
#pragma unroll
                        for (int k = 0; k < N; ++k) gq[k] += A.weight * dq[k];
                    }
                }
                if constexpr (SDF) {
                    if (m > 0 || (support && i >= 1)) {        // the range of the link fields above
                        for (int ti = 0; ti < A.n_terms; ++ti) {
                            real fx, fy;
                            const real h = grid_sdf_force(A.t[ti], x[0], x[N > 1 ? 1 : 0], &fx, &fy);
                            const real w = A.weight * A.t[ti].K;
                            part += A.t[ti].K * h;
                            gq[0] += w * fx;
                            gq[N > 1 ? 1 : 0] += w * fy;
                        }
                    }
                }
                if (m == 0) {                                  // the support state itself: the identity
#pragma unroll
                    for (int k = 0; k < N; ++k) { ga[k] += gq[k]; ga[N + k] += gv[k]; }
                } else {                                       // the transpose of hermite_state's eight coefficients
                    const real* c = H.c[m - 1];
#pragma unroll
                    for (int k = 0; k < N; ++k) {
                        ga[k] += c[0] * gq[k] + c[4] * gv[k];
                        ga[N + k] += c[1] * gq[k] + c[5] * gv[k];
                        gb[k] += c[2] * gq[k] + c[6] * gv[k];
                        gb[N + k] += c[3] * gq[k] + c[7] * gv[k];
                    }
                }
            }
            if (T <= 64) any_bad = __any(bad ? 1 : 0) != 0;    // (one pass: nothing has been stored yet)
            const real nan = std::numeric_limits<real>::quiet_NaN();
            real* row = gr + (size_t)(i < T ? i : 0) * (2 * N);
#pragma unroll
            for (int k = 0; k < 2 * N; ++k) {
                real up = __shfl_up(gb[k], 1, 64);
                if (lane == 0) up = carry[k];
                carry[k] = __shfl(gb[k], 63, 64);
                real v = ga[k] + up;
                if (any_bad) v = nan;
                if (i < T) row[k] = A.accumulate ? row[k] + v : v;
            }
        }
        double acc = wave_sum((double)(A.weight * part) + (double)(A.inv_sigma2 * lim));
        if (lane == 0) {
            if (any_bad) acc = std::numeric_limits<double>::quiet_NaN();
            if (costs64) costs64[b] = acc;
            if (costs) costs[b] = (real)acc;
        }
    }
}

// SGPMP_OK, or the code of a refusal (message set)
template <typename real>
static int launch_dense_cost_grad(const SgpmpCtxView& v, const void* trajs, long long batch, int n_sub, double dt,
                                  const void* spheres, int n_spheres, double weight, const double* q_lo, const double* q_hi,
                                  const double* v_max, double sigma_limit, int support, int accumulate, void* grad, void* costs,
                                  double* costs64, hipStream_t stream) {
    constexpr bool f64 = sizeof(real) == 8;
    const int n = v.dims.n_dof;
    DenseCostK<real> A;
    std::memset(&A, 0, sizeof(A));
    A.T = v.dims.traj_len; A.n_sub = n_sub; A.accumulate = accumulate ? 1 : 0;
    A.weight = (real)weight;
    bool interp = false;
    int n_sdf = 0;
    // weight 0 (the limit part alone) evaluates no field; neither does n_sub 0 without the support waypoints
    for (int i = 0; v.prog && weight > 0. && (n_sub > 0 || support) && i < v.prog->n_terms; ++i) {
        const CostTerm& s = v.prog->terms[i];
        if (s.kind == SGPMP_COST_GRID_SDF) { A.t[A.n_terms++] = make_termk<real>(s); ++n_sdf; continue; }
        if (s.kind != SGPMP_COST_SPHERES && s.kind != SGPMP_COST_SELF) continue;   // (a GRID term with n_sub > 0 was refused)
        if (s.kind == SGPMP_COST_SPHERES && n_spheres < 1) continue;               // no obstacle: the term adds nothing
        A.t[A.n_terms++] = make_termk<real>(s);
        interp = interp || s.n_interp > 0;
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
    const char* name = "";
    size_t lds = 0;
    int nj = -1;                                               // -1: no link field; 0: generic; 10, 7: compile-time chain length
    if (n_sdf > 0 && n_sdf < A.n_terms)
        return sgpmp_set_error(SGPMP_EINVAL, "sgpmp_dense_cost_grad: a grid distance term together with link-field terms is not "
                                             "supported (the grid distance field belongs to planar cost lists)");
    if (n_sdf > 0 && n < 2) return sgpmp_set_error(SGPMP_EINVAL, "sgpmp_dense_cost_grad: a grid distance term needs n_dof >= 2");
    if (A.n_terms > 0 && n_sdf == 0) {
        A.spheres = n_spheres > 0 ? (const real*)spheres : nullptr;
        A.n_spheres = A.spheres ? n_spheres : 0;
        A.n_links = v.h_chain->n_links;
        A.chain = v.d_chain;
        const int joints = v.h_chain->n_joints;
        nj = (n == 7 && (joints == 10 || joints == 7) && !interp && !v.tg->force_generic_fk) ? joints : 0;
        {
            lds = grad_lds_bytes<real>(A.n_links);
            if (lds > SGPMP_GRAD_LDS_MAX) {
                char msg[256];
                snprintf(msg, sizeof(msg), "sgpmp_dense_cost_grad: a chain of %d links needs %d x 3 x 64 x 8 (forces) + (2 x %d - 1) x 3 x 64 x %d "
                         "(points, joint axes) = %zu bytes of LDS columns, the kernel's budget is %d: at most %d links in this dtype",
                         A.n_links, A.n_links, A.n_links, (int)sizeof(real), lds, SGPMP_GRAD_LDS_MAX,
                         (int)((SGPMP_GRAD_LDS_MAX / 192 + sizeof(real)) / (8 + 2 * sizeof(real))));
                return sgpmp_set_error(SGPMP_EINVAL, msg);
            }
        }
    }
#define GRAD_LAUNCH(NN, NJ_)                                                                                          \
    hipLaunchKernelGGL((dense_cost_grad_kernel<real, NN, NJ_>), grid, block, lds, stream, (const real*)trajs, batch, \
                       A, H, support ? 1 : 0, (real*)grad, (real*)costs, costs64)
#define GRAD_CASE(NN, NJ_) case NN: GRAD_LAUNCH(NN, NJ_); break;
    if (nj == 10) {
        name = f64 ? "dense_cost_grad_kernel<f64, 10 joints>" : "dense_cost_grad_kernel<f32, 10 joints>";
        GRAD_LAUNCH(7, 10);
    } else if (nj == 7) {
        name = f64 ? "dense_cost_grad_kernel<f64, 7 joints>" : "dense_cost_grad_kernel<f32, 7 joints>";
        GRAD_LAUNCH(7, 7);
    } else if (nj == 0) {
        name = f64 ? "dense_cost_grad_kernel<f64, generic>" : "dense_cost_grad_kernel<f32, generic>";
        switch (n) {
            GRAD_CASE(1, 0) GRAD_CASE(2, 0) GRAD_CASE(3, 0) GRAD_CASE(4, 0) GRAD_CASE(5, 0) GRAD_CASE(6, 0) GRAD_CASE(7, 0) GRAD_CASE(8, 0)
            default: return sgpmp_set_error(SGPMP_EINVAL, "sgpmp_dense_cost_grad: n_dof out of range");
        }
    } else if (n_sdf > 0) {
        name = f64 ? "dense_cost_grad_kernel<f64, grid distance>" : "dense_cost_grad_kernel<f32, grid distance>";
#define GRAD_SDF_CASE(NN)                                                                                             \
    case NN:                                                                                                          \
        hipLaunchKernelGGL((dense_cost_grad_kernel<real, NN, -1, true>), grid, block, 0, stream, (const real*)trajs, \
                           batch, A, H, support ? 1 : 0, (real*)grad, (real*)costs, costs64);                         \
        break;
        switch (n) {
            GRAD_SDF_CASE(2) GRAD_SDF_CASE(3) GRAD_SDF_CASE(4) GRAD_SDF_CASE(5) GRAD_SDF_CASE(6) GRAD_SDF_CASE(7) GRAD_SDF_CASE(8)
            default: return sgpmp_set_error(SGPMP_EINVAL, "sgpmp_dense_cost_grad: n_dof out of range");
        }
#undef GRAD_SDF_CASE
    } else {
        name = f64 ? "dense_cost_grad_kernel<f64, no FK>" : "dense_cost_grad_kernel<f32, no FK>";
        switch (n) {
            GRAD_CASE(1, -1) GRAD_CASE(2, -1) GRAD_CASE(3, -1) GRAD_CASE(4, -1) GRAD_CASE(5, -1) GRAD_CASE(6, -1) GRAD_CASE(7, -1) GRAD_CASE(8, -1)
            default: return sgpmp_set_error(SGPMP_EINVAL, "sgpmp_dense_cost_grad: n_dof out of range");
        }
    }
#undef GRAD_CASE
#undef GRAD_LAUNCH
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return dense_hip_error("sgpmp_dense_cost_grad", e);
    g_last_dense_kernel = name;                                // published only once the launch has been accepted
    return SGPMP_OK;
}

extern "C" int sgpmp_dense_cost_grad(sgpmp_ctx* c, const void* trajs, int64_t batch, int n_sub, double dt, const void* spheres,
                                     int n_spheres, double weight, const double* q_lo, const double* q_hi, const double* v_max,
                                     double sigma_limit, int support, int accumulate, void* grad, void* costs, double* costs64,
                                     void* stream) {
    const bool limits = q_lo || q_hi || v_max;
    if (!c || batch < 0 || n_sub < 0 || n_sub > SGPMP_MAX_SUBSTEPS || !(dt > 0.) || !(weight >= 0.) || n_spheres < 0 ||
        (limits && !(sigma_limit > 0.)) || (batch > 0 && (!trajs || !grad)))
        return sgpmp_set_error(SGPMP_EINVAL, "sgpmp_dense_cost_grad: bad argument (n_sub in [0, 31], dt > 0, weight >= 0, "
                                             "sigma_limit > 0 with limits, non-null trajs and grad)");
    SgpmpCtxView v;
    const int view_rc = sgpmp_ctx_view(c, &v);
    if (view_rc != SGPMP_OK) return view_rc;                   // (finalize_program said why)
    if (const char* refused = voxel_term_refusal("sgpmp_dense_cost_grad", v)) return sgpmp_set_error(SGPMP_EINVAL, refused);
    for (int i = 0; v.prog && i < v.prog->n_terms; ++i) {
        const int kind = v.prog->terms[i].kind;
        if ((kind == SGPMP_COST_SPHERES || kind == SGPMP_COST_SELF) && !v.have_chain)
            return sgpmp_set_error(SGPMP_ESTATE, "sgpmp_dense_cost_grad: link-field terms need an FK chain (sgpmp_set_fk)");
        if (kind == SGPMP_COST_SPHERES && n_spheres > 0 && !spheres)
            return sgpmp_set_error(SGPMP_ESTATE, "sgpmp_dense_cost_grad: n_spheres > 0 without obstacle spheres");
    }
    // never a silently zero gradient: the piecewise-constant terms are refused wherever a state would evaluate them
    for (int i = 0; v.prog && weight > 0. && i < v.prog->n_terms; ++i) {
        const CostTerm& s = v.prog->terms[i];
        if (s.kind == SGPMP_COST_GRID && n_sub > 0)
            return sgpmp_set_error(SGPMP_EINVAL, "sgpmp_dense_cost_grad: the grid lookup is piecewise constant and has no gradient "
                                                 "(weight = 0 gives the limit part alone)");
        if (s.kind == SGPMP_COST_SPHERES && (s.flags & 15) == SGPMP_FIELD_OCCUPANCY && n_spheres > 0 && (n_sub > 0 || support))
            return sgpmp_set_error(SGPMP_EINVAL, "sgpmp_dense_cost_grad: the occupancy count is piecewise constant and has no gradient "
                                                 "(rbf and sdf sphere fields do; weight = 0 gives the limit part alone)");
    }
    if (batch == 0) return SGPMP_OK;
    return v.dims.dtype == SGPMP_F64
        ? launch_dense_cost_grad<double>(v, trajs, batch, n_sub, dt, spheres, n_spheres, weight, q_lo, q_hi, v_max, sigma_limit,
                                         support, accumulate, grad, costs, costs64, (hipStream_t)stream)
        : launch_dense_cost_grad<float>(v, trajs, batch, n_sub, dt, spheres, n_spheres, weight, q_lo, q_hi, v_max, sigma_limit,
                                        support, accumulate, grad, costs, costs64, (hipStream_t)stream);
}
