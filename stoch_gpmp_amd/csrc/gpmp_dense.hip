// GPMP with continuous-time factors: the Gauss-Newton solve when collision rows on the GP-interpolated states and limit rows on
// all fine states are part of the linear system (sgpmp_gpmp_set_dense; no reference counterpart -- the reference's GPMP has
// rows at the T support waypoints only).
//
// With k = n_sub states inserted per interval, fine state m of interval t is x_f = Lambda[m] x_t + Psi[m] x_{t+1} (the 2 x 2
// blocks per degree of freedom of dense.hermite_weights; HermiteTab holds them as c0 .. c7).  Every new factor is a scalar row
// (A row = -d error / d x, b = error, as in gpmp.hip):
//   * collision row of field term f at an inserted state: error = field(q_f), precision = weight x K_f; with g = d field / d q_f
//     its entries are -c0 g, -c1 g on (q_t, v_t) and -c2 g, -c3 g on (q_{t+1}, v_{t+1});
//   * limit rows per degree of freedom j at every fine state, precision 1 / sigma_limit^2: max(0, q_lo - q), max(0, q - q_hi)
//     on row 0 of (Lambda, Psi), max(0, |q'| - v_max) on sign(q') x row 1; an inactive row is a zero row.
// A row touches x_t and x_{t+1} only: A^T K A stays block-tridiagonal, but the sub-diagonal block is no longer the constant
// -Q^-1 Phi and the diagonal blocks are full d x d.  With U (2d x R) the rows of interval t, U K U^T cut into (t,t), (t+1,t),
// (t+1,t+1) feeds S_t, E_{t+1} and -- carried over -- S_{t+1}.
//
// gpmp_dense_solve_kernel: gpmp_solve_kernel's block Cholesky over the waypoints (one wave per particle, 16 x 16 fp64 LDS tiles,
// products on v_mfma_f64_16x16x4_f64) with a per-interval E.  The ROW index is the K dimension of the matrix instruction: lane
// (i = l & 15, kq = l >> 4) forms entry i of row 4 c + kq of chunk c straight from the Jacobian in global memory (the support
// waypoint's own rows ride in the same stream with Lambda = I), so the three products of a chunk need no staging tile and their
// accumulators stay in registers for the whole interval; the accumulator layout (row kq + 4 r, column i) is the layout of the
// S-assembly loop.  Limit rows are 4 nonzeros on one degree of freedom: a lane adds them to its accumulator elements directly,
// from the fine (q, q') it evaluates from the means in LDS in hermite_state's operation order.  LDS per particle: the means and
// the solution, whatever n_sub; values and Jacobians stream, the first chunk of the next waypoint in flight during this
// waypoint's factorisation.
#include "sgpmp_internal.h"

typedef double d4 __attribute__((ext_vector_type(4)));
#define TS SGPMP_TILE

template <typename real>
__device__ __forceinline__ double ldr(const void* p, size_t i) { return (double)((const real*)p)[i]; }

__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ double mul_rn(double a, double b) { return __dmul_rn(a, b); }
// one coordinate of hermite_state (traj_dense.hip): the same multiply and three fmas, in the same order and type
template <typename real>
__device__ __forceinline__ real herm(const real* __restrict__ c, real aq, real av, real bq, real bv) {
    return __builtin_fma(c[3], bv, __builtin_fma(c[2], bq, __builtin_fma(c[1], av, mul_rn(c[0], aq))));
}

// The limit rows of fine state m of the interval (a, b), degree of freedom j: the errors e[3] = (q_lo - q)+, (q - q_hi)+,
// (|q'| - v_max)+ and the signed sums sP = e0 - e1, sV = -sign(q') e2 that multiply row 0 / row 1 in A^T K b.
struct LimitRow { double e0, e1, e2, sP, sV; };
template <typename real>
__device__ __forceinline__ LimitRow limit_row(const GpmpDenseArgs& da, const real* __restrict__ c, int m, int j, real aq, real av,
                                              real bq, real bv) {
    const real q = m == 0 ? aq : herm<real>(c, aq, av, bq, bv);
    const real v = m == 0 ? av : herm<real>(c + 4, aq, av, bq, bv);
    LimitRow r;
    r.e0 = da.has_lo ? fmax(da.q_lo[j] - (double)q, 0.) : 0.;
    r.e1 = da.has_hi ? fmax((double)q - da.q_hi[j], 0.) : 0.;
    r.e2 = da.has_v ? fmax(fabs((double)v) - da.v_max[j], 0.) : 0.;
    r.sP = r.e0 - r.e1;
    r.sV = v > (real)0 ? -r.e2 : r.e2;
    return r;
}

// ---------------------------------------------------------------------------------- trust-region damping
// Sum over this rank's particles of the field-and-dense part of diag(A^T K A): the support waypoints' collision rows (what
// gpmp_diag_kernel sums), the inserted states' collision rows and the limit rows -- velocity entries and waypoint 0 included.
// Workgroup = 8 particles, threads over the (t, c) elements of the diagonal, one fp64 atomic per element and workgroup.
#define SGPMP_DDIAG_PCHUNK 8
template <typename real>
__global__ void __launch_bounds__(256)
gpmp_dense_diag_kernel(GpmpArgs a, GpmpDenseArgs da, HermiteTab<real> H, const real* __restrict__ means,
                       double* __restrict__ diag_sum) {
    const int n = a.n, d = 2 * n, T = a.T, k = da.n_sub, k1 = k + 1;
    const size_t F1 = (size_t)da.Tf - 1;
    const int p0 = blockIdx.x * SGPMP_DDIAG_PCHUNK, p1 = min(p0 + SGPMP_DDIAG_PCHUNK, a.P);
    for (int e = threadIdx.x; e < T * d; e += blockDim.x) {
        const int t = e / d, c = e - t * d, j = c % n, tc = c < n ? 0 : 1;
        double s = 0.;
        for (int p = p0; p < p1; ++p) {
            const real* mp = means + (size_t)p * T * d;
            // side 0: fine states m = 0 .. k of interval t (x_t is the interval's first state); side 1: m = 1 .. k of interval t - 1
            for (int side = 0; side < 2; ++side) {
                const int ti = t - side;
                if (ti < 0) continue;
                const int m_lo = side, m_hi = ti <= T - 2 ? k : 0;
                const int tb = ti <= T - 2 ? ti + 1 : ti;
                const real aq = mp[ti * d + j], av = mp[ti * d + n + j], bq = mp[tb * d + j], bv = mp[tb * d + n + j];
                for (int m = m_lo; m <= m_hi; ++m) {
                    const real* hc = H.c[m > 0 ? m - 1 : 0];
                    const double pc = m == 0 ? (tc == 0 ? 1. : 0.) : (double)hc[2 * side + tc];
                    const double vc = m == 0 ? (tc == 1 ? 1. : 0.) : (double)hc[4 + 2 * side + tc];
                    if (m == 0 ? ti >= 1 : da.weight > 0.) {
                        const size_t row = (size_t)p * F1 + (size_t)ti * k1 + m - 1;
                        for (int f = 0; f < a.n_fields; ++f) {
                            if (m > 0 && !da.inserted[f]) continue;
                            const double h = pc * ldr<real>(a.f[f].grad, row * n + j);
                            s += (m == 0 ? a.f[f].K : da.weight * a.f[f].K) * h * h;
                        }
                    }
                    if (da.Klim > 0.) {
                        const LimitRow r = limit_row<real>(da, hc, m, j, aq, av, bq, bv);
                        const double nP = (r.e0 > 0. ? 1. : 0.) + (r.e1 > 0. ? 1. : 0.), nV = r.e2 > 0. ? 1. : 0.;
                        s += da.Klim * (nP * pc * pc + nV * vc * vc);
                    }
                }
            }
        }
        atomicAdd(&diag_sum[e], s);
    }
}

// ---------------------------------------------------------------------------------- the solve
// C = alpha * op(A) * op(B) + beta * Cin on 16x16 row-major LDS tiles, one wave (gpmp.hip: gp_mm16)
__device__ __forceinline__ void gd_mm16(double* C, const double* A, const double* B, bool tA, bool tB, double alpha,
                                        const double* Cin, double beta) {
    const int l = threadIdx.x;
    const int i = l & 15, kq = l >> 4;
    d4 acc = {0., 0., 0., 0.};
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
        const int k = 4 * kb + kq;
        const double a = tA ? A[k * TS + i] : A[i * TS + k];
        const double b = tB ? B[i * TS + k] : B[k * TS + i];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
    double cin[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) cin[r] = Cin ? Cin[(kq + 4 * r) * TS + i] : 0.;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) C[(kq + 4 * r) * TS + i] = alpha * acc[r] + beta * cin[r];
    __syncthreads();
}

// constant part of block (t,t) of A^T K A, element (r,c) (gpmp.hip: gp_diag_const)
__device__ __forceinline__ double gd_diag_const(const GpmpArgs& a, int t, int r, int c) {
    const int n = a.n;
    if ((r % n) != (c % n)) return 0.;
    const bool rp = r < n, cp = c < n;
    const double q = a.Kgp * (rp ? (cp ? a.c11 : a.c12) : (cp ? a.c12 : a.c22));
    const double m = a.c11 * a.dt + a.c12;
    const double pqp = a.Kgp * (rp ? (cp ? a.c11 : m) : (cp ? m : a.c11 * a.dt * a.dt + 2. * a.c12 * a.dt + a.c22));
    double v = 0.;
    if (t >= 1) v += q;
    if (t <= a.T - 2) v += pqp;
    if (r == c) {
        if (t == 0) v += a.Ks;
        if (t == a.T - 1) v += a.Kg;
    }
    return v;
}

// Row 4 c + kq of waypoint t's collision stream, as this lane sees it: rows [m = 0 .. kc][f = 0 .. F), m = 0 the support
// waypoint's own row (t >= 1), m >= 1 the inserted states of interval t.  Loads this lane's Jacobian entry and the value.
struct RowLoad { double g, val; };
template <typename real>
__device__ __forceinline__ RowLoad row_load(const void* const* fval, const void* const* fgrad, const int* fins, int F, int nrows,
                                            int rho, int t, int k1, size_t pbase, int n, int j, bool in_d) {
    RowLoad r = {0., 0.};
    if (rho < nrows) {
        const int m = rho / F, f = rho - m * F;
        if (m == 0 ? t >= 1 : fins[f] != 0) {
            const size_t row = pbase + (size_t)t * k1 + m - 1;
            r.val = ldr<real>(fval[f], row);
            if (in_d) r.g = ldr<real>(fgrad[f], row * n + j);
        }
    }
    return r;
}

template <typename real>
__global__ void __launch_bounds__(64)
gpmp_dense_solve_kernel(GpmpArgs a, GpmpDenseArgs da, HermiteTab<real> H, real* __restrict__ means, real* __restrict__ d_theta,
                        real* __restrict__ costs) {
    __shared__ double S[TS * TS], L[TS * TS], Li[TS * TS], Lp[TS * TS], W[TS * TS], E[TS * TS], Cn[TS * TS];
    __shared__ double g[TS], gn[TS], r[TS], tmp[TS], rinv[TS];
    __shared__ double csum[64];
    __shared__ real hc[(SGPMP_MAX_SUBSTEPS + 1) * 8];        // [m][8], m = 0: the identity
    __shared__ double fK[4];
    __shared__ const void* fval[4];
    __shared__ const void* fgrad[4];
    __shared__ int fins[4];
    // sized by the launch: means and solution [T][16] -- nothing that grows with n_sub
    extern __shared__ __align__(16) unsigned char gd_lds_raw[];
    const int l = threadIdx.x, p = blockIdx.x;
    const int i = l & 15, kq = l >> 4;
    const int n = a.n, d = 2 * n, T = a.T, k = da.n_sub, k1 = k + 1, F = a.n_fields;
    double* mu = reinterpret_cast<double*>(gd_lds_raw);
    double* y = mu + (size_t)T * TS;
    real* mp = means + (size_t)p * T * d;
    double* scr = a.scratch + (size_t)p * T * 2 * TS * TS;
    for (int e = l; e < T * TS; e += 64) {
        const int t = e / TS, c = e % TS;
        mu[e] = c < d ? (double)mp[t * d + c] : 0.;
    }
    for (int e = l; e < (SGPMP_MAX_SUBSTEPS + 1) * 8; e += 64) {
        const int m = e >> 3, c = e & 7;
        hc[e] = m == 0 ? (real)((c == 0 || c == 5) ? 1 : 0) : H.c[m - 1][c];
    }
    if (l < 4) {
        fK[l] = l < F ? a.f[l].K : 0.;
        fval[l] = l < F ? a.f[l].val : nullptr;
        fgrad[l] = l < F ? a.f[l].grad : nullptr;
        fins[l] = l < F ? da.inserted[l] : 0;
    }
    // this lane's four elements (row kq + 4 r, column i) of a tile: the constant sub-diagonal block -Q^-1 Phi, and whether the
    // element couples one degree of freedom with itself (where limit rows land), with the row's type (0: position, 1: velocity)
    const bool in_d = i < d;
    const int j = in_d ? i % n : 0, tb = i < n ? 0 : 1;
    double cE[4];
    bool same[4];
    int ta[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int rr = kq + 4 * q;
        double v = 0.;
        if (rr < d && in_d && (rr % n) == j) {
            const bool rp = rr < n;
            const double q1 = rp ? a.c11 : a.c12, q2 = rp ? a.c12 : a.c22;
            v = -a.Kgp * (tb == 0 ? q1 : q1 * a.dt + q2);
        }
        cE[q] = v;
        same[q] = rr < d && in_d && (rr % n) == j;
        ta[q] = rr < n ? 0 : 1;
        const int e = rr * TS + i;
        E[e] = v; Cn[e] = 0.; Lp[e] = 0.; L[e] = 0.; Li[e] = 0.; W[e] = 0.;
    }
    if (l < TS) gn[l] = 0.;
    __syncthreads();
    const long long gi = a.Kg > 0. ? (a.p_offset + p) / a.rows_per_goal : 0;
    const size_t pbase = (size_t)p * ((size_t)da.Tf - 1);
    const int kc = da.weight > 0. ? k : 0;                // inserted states that carry collision rows
    double cost = 0.;                                    // b^T K b, accumulated per lane, summed over the wave at the end
    RowLoad nxt = {0., 0.};                              // chunk 0 of the next waypoint (nothing at t = 0: no support row)
    if (F > 0) nxt = row_load<real>(fval, fgrad, fins, F, (T >= 2 ? kc + 1 : 1) * F, kq, 0, k1, pbase, n, j, in_d);

    for (int t = 0; t < T; ++t) {
        // ---- right-hand side g_t and the cost of the GP / start / goal factors at waypoint t (gpmp_solve_kernel)
        if (l < TS) {
            double v = 0.;
            if (l < d) {
                const int kk = l % n;
                const bool pos = l < n;
                if (t == 0 && a.Ks > 0.) {
                    const double e0 = ldr<real>(a.start, l) - mu[l];
                    v += a.Ks * e0;
                    cost += a.Ks * e0 * e0;
                }
                if (t == T - 1 && a.Kg > 0.) {
                    const double eg = ldr<real>(a.goals, (size_t)gi * d + l) - mu[t * TS + l];
                    v += a.Kg * eg;
                    cost += a.Kg * eg * eg;
                }
                if (t <= T - 2) {
                    const double ep = mu[(t + 1) * TS + kk] - (mu[t * TS + kk] + a.dt * mu[t * TS + n + kk]);
                    const double ev = mu[(t + 1) * TS + n + kk] - mu[t * TS + n + kk];
                    const double qp = a.Kgp * (a.c11 * ep + a.c12 * ev), qv = a.Kgp * (a.c12 * ep + a.c22 * ev);
                    v += pos ? qp : a.dt * qp + qv;
                    cost += pos ? ep * qp : ev * qv;
                }
                if (t >= 1) {
                    const double ep = mu[t * TS + kk] - (mu[(t - 1) * TS + kk] + a.dt * mu[(t - 1) * TS + n + kk]);
                    const double ev = mu[t * TS + n + kk] - mu[(t - 1) * TS + n + kk];
                    v -= a.Kgp * (pos ? a.c11 * ep + a.c12 * ev : a.c12 * ep + a.c22 * ev);
                }
            }
            g[l] = v;
        }
        // ---- rows of waypoint t / interval t: U K U^T cut into (t,t), (t+1,t), (t+1,t+1), and U K b
        d4 A11 = {0., 0., 0., 0.}, A21 = {0., 0., 0., 0.}, A22 = {0., 0., 0., 0.};
        double rg1 = 0., rg2 = 0.;
        const bool interval = t <= T - 2;
        {
            const int nrows = ((interval ? kc : 0) + 1) * F, chunks = (nrows + 3) >> 2;
            RowLoad cur = nxt;
            for (int c = 0; c < chunks; ++c) {
                if (c + 1 < chunks)
                    nxt = row_load<real>(fval, fgrad, fins, F, nrows, 4 * (c + 1) + kq, t, k1, pbase, n, j, in_d);
                const int rho = 4 * c + kq;
                const int m = rho < nrows ? rho / F : 0, f = rho < nrows ? rho - m * F : 0;
                const double Kr = rho < nrows ? (m == 0 ? fK[f] : da.weight * fK[f]) : 0.;
                const double u1 = -(double)hc[m * 8 + tb] * cur.g, u2 = -(double)hc[m * 8 + 2 + tb] * cur.g;
                A11 = __builtin_amdgcn_mfma_f64_16x16x4f64(Kr * u1, u1, A11, 0, 0, 0);
                A21 = __builtin_amdgcn_mfma_f64_16x16x4f64(Kr * u2, u1, A21, 0, 0, 0);
                A22 = __builtin_amdgcn_mfma_f64_16x16x4f64(Kr * u2, u2, A22, 0, 0, 0);
                rg1 += Kr * u1 * cur.val;
                rg2 += Kr * u2 * cur.val;
                if (i == 0) cost += Kr * cur.val * cur.val;
                cur = nxt;
            }
        }
        if (da.Klim > 0. && in_d) {
            const int tn = interval ? t + 1 : t;
            const real aq = (real)mu[t * TS + j], av = (real)mu[t * TS + n + j];
            const real bq = (real)mu[tn * TS + j], bv = (real)mu[tn * TS + n + j];
            for (int m = 0; m <= (interval ? k : 0); ++m) {
                const real* c = hc + m * 8;
                const LimitRow lr = limit_row<real>(da, c, m, j, aq, av, bq, bv);
                if (!(lr.e0 > 0.) && !(lr.e1 > 0.) && !(lr.e2 > 0.)) continue;
                const double nP = da.Klim * ((lr.e0 > 0. ? 1. : 0.) + (lr.e1 > 0. ? 1. : 0.)), nV = lr.e2 > 0. ? da.Klim : 0.;
                const double cPa = (double)c[tb], cPb = (double)c[2 + tb], cVa = (double)c[4 + tb], cVb = (double)c[6 + tb];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (!same[q]) continue;
                    const double rPa = (double)c[ta[q]], rPb = (double)c[2 + ta[q]];
                    const double rVa = (double)c[4 + ta[q]], rVb = (double)c[6 + ta[q]];
                    A11[q] += nP * rPa * cPa + nV * rVa * cVa;
                    A21[q] += nP * rPb * cPa + nV * rVb * cVa;
                    A22[q] += nP * rPb * cPb + nV * rVb * cVb;
                }
                if (kq == 0) {
                    rg1 += da.Klim * (lr.sP * cPa + lr.sV * cVa);
                    rg2 += da.Klim * (lr.sP * cPb + lr.sV * cVb);
                    if (tb == 0) cost += da.Klim * (lr.e0 * lr.e0 + lr.e1 * lr.e1 + lr.e2 * lr.e2);
                }
            }
        }
        rg1 += __shfl_xor(rg1, 16, 64); rg1 += __shfl_xor(rg1, 32, 64);
        rg2 += __shfl_xor(rg2, 16, 64); rg2 += __shfl_xor(rg2, 32, 64);
        if (l < TS) {
            g[l] += rg1 + gn[l];                         // + what interval t - 1 left for this waypoint
            gn[l] = rg2;
        }
        // chunk 0 of waypoint t + 1: in flight while this waypoint factors
        if (F > 0 && t + 1 < T)
            nxt = row_load<real>(fval, fgrad, fins, F, ((t + 1 <= T - 2 ? kc : 0) + 1) * F, kq, t + 1, k1, pbase, n, j, in_d);
        // ---- S = D_t + rows + damping - W W^T   (element (kq + 4 q, i): the accumulators' own layout)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int rr = kq + 4 * q, c = i, e = rr * TS + c;
            double v = 0.;
            if (rr < d && c < d) {
                v = gd_diag_const(a, t, rr, c) + Cn[e] + A11[q];
                if (rr == c)
                    v += a.diag_sum ? a.delta * (gd_diag_const(a, t, rr, rr) + a.diag_sum[t * d + rr] * a.inv_particles)
                                    : a.delta;
            } else if (rr == c) {
                v = 1.;                                   // padding keeps the tile positive definite
            }
            S[e] = v;
        }
        __syncthreads();
        if (t >= 1) {
            gd_mm16(W, E, Lp, false, true, 1., nullptr, 0.);         // W = E_t L_{t-1}^-T
            gd_mm16(S, W, W, false, true, -1., S, 1.);               // S -= W W^T
            if (l < TS) {                                            // r = g - W y_{t-1}
                double v = g[l];
                for (int c = 0; c < d; ++c) v -= W[l * TS + c] * y[(t - 1) * TS + c];
                r[l] = v;
            }
        } else if (l < TS) {
            r[l] = g[l];
        }
        // E_{t+1} = -Q^-1 Phi + (t+1,t) part of interval t; its (t+1,t+1) part waits in Cn (E_t was last read above)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = (kq + 4 * q) * TS + i;
            E[e] = cE[q] + A21[q];
            Cn[e] = A22[q];
        }
        __syncthreads();
        // ---- L L^T = S (lower), one column per step, lanes over rows
        for (int jc = 0; jc < TS; ++jc) {
            if (l >= jc && l < TS) {
                double v = S[l * TS + jc];
                for (int kk = 0; kk < jc; ++kk) v -= L[l * TS + kk] * L[jc * TS + kk];
                tmp[l] = v;
            }
            __syncthreads();
            const double piv = tmp[jc];
            if (!(piv > 0.) || !(piv < 1e300)) { if (l == 0) *a.status = 1; }
            const double rt = sqrt(piv > 0. ? piv : 1.);
            const double ri = 1. / rt;
            if (l < TS) L[l * TS + jc] = l > jc ? tmp[l] * ri : (l == jc ? rt : 0.);
            if (l == 0) rinv[jc] = ri;
            __syncthreads();
        }
        // ---- Li = L^-1 (forward substitution, lanes over columns)
        for (int ii = 0; ii < TS; ++ii) {
            if (l < TS) {
                double v = (ii == l) ? 1. : 0.;
                for (int kk = 0; kk < ii; ++kk) v -= L[ii * TS + kk] * Li[kk * TS + l];
                Li[ii * TS + l] = v * rinv[ii];
            }
            __syncthreads();
        }
        if (l < TS) {                                               // y_t = L^-1 r
            double v = 0.;
            for (int c = 0; c <= l; ++c) v += Li[l * TS + c] * r[c];
            y[t * TS + l] = v;
        }
        for (int e = l; e < TS * TS; e += 64) {                     // park L^-1 and W for the back sweep
            scr[(size_t)(2 * t) * TS * TS + e] = Li[e];
            scr[(size_t)(2 * t + 1) * TS * TS + e] = W[e];
            Lp[e] = Li[e];
        }
        __syncthreads();
    }
    // ---- cost of the linearisation point: b^T K b over every row, the new ones included
    csum[l] = cost;
    __syncthreads();
    if (l == 0) {
        double c = 0.;
        for (int e = 0; e < 64; ++e) c += csum[e];
        if (costs) costs[p] = (real)c;
    }
    // ---- backward: x_t = L_t^-T (y_t - W_{t+1}^T x_{t+1}), as gpmp_solve_kernel
    for (int t = T - 1; t >= 0; --t) {
        double nl[4], nw[4];
        if (t >= 1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                nl[q] = scr[(size_t)(2 * (t - 1)) * TS * TS + l + 64 * q];
                nw[q] = scr[(size_t)(2 * t + 1) * TS * TS + l + 64 * q];   // W_t, needed by step t-1
            }
        }
        if (l < TS) {
            double v = y[t * TS + l];
            if (t < T - 1)
                for (int c = 0; c < d; ++c) v -= W[c * TS + l] * y[(t + 1) * TS + c];   // W currently = W_{t+1}
            r[l] = v;
        }
        __syncthreads();
        if (l < TS) {
            double v = 0.;
            for (int c = l; c < TS; ++c) v += Li[c * TS + l] * r[c];
            y[t * TS + l] = v;
        }
        __syncthreads();
        if (t >= 1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) { Li[l + 64 * q] = nl[q]; W[l + 64 * q] = nw[q]; }
        }
        __syncthreads();
    }
    for (int e = l; e < T * d; e += 64) {
        const int t = e / d, c = e % d;
        const double x = y[t * TS + c];
        if (d_theta) d_theta[(size_t)p * T * d + e] = (real)x;
        mp[e] = (real)(mu[t * TS + c] + a.step_size * x);
    }
}

// ---------------------------------------------------------------------------------- launchers
template <typename real>
static HermiteTab<real> hermite_tab(int n_sub, double dt) {
    HermiteTab<real> H;
    hermite_table(sizeof(real) == 8 ? SGPMP_F64 : SGPMP_F32, n_sub, dt, &H);
    return H;
}
static_assert(sizeof(GpmpArgs) + sizeof(GpmpDenseArgs) + sizeof(HermiteTab<double>) + 4 * sizeof(void*) <= 4096,
              "gpmp_dense_solve_kernel: kernel arguments");

hipError_t launch_gpmp_dense_diag(int dtype, const GpmpArgs& a, const GpmpDenseArgs& da, const void* means, double* diag_sum,
                                  hipStream_t stream) {
    hipError_t e = hipMemsetAsync(diag_sum, 0, (size_t)a.T * 2 * a.n * sizeof(double), stream);
    if (e != hipSuccess || a.P <= 0) return e;
    const unsigned grid = (unsigned)((a.P + SGPMP_DDIAG_PCHUNK - 1) / SGPMP_DDIAG_PCHUNK);
    if (dtype == SGPMP_F64)
        hipLaunchKernelGGL((gpmp_dense_diag_kernel<double>), dim3(grid), dim3(256), 0, stream, a, da,
                           hermite_tab<double>(da.n_sub, da.dt), (const double*)means, diag_sum);
    else
        hipLaunchKernelGGL((gpmp_dense_diag_kernel<float>), dim3(grid), dim3(256), 0, stream, a, da,
                           hermite_tab<float>(da.n_sub, da.dt), (const float*)means, diag_sum);
    return hipGetLastError();
}

hipError_t launch_gpmp_dense_solve(int dtype, const GpmpArgs& a, const GpmpDenseArgs& da, void* means, void* d_theta,
                                   void* costs, hipStream_t stream) {
    if (a.P <= 0) return hipSuccess;
    // means and solution [T][16] only (the fields stay in HBM): 32 768 B at SGPMP_MAX_T_GPMP = 128, beside at most 17 648 B of static
    // tiles and tables -- 50 416 B, below the 64 KiB above which sgpmp_allow_lds would have to raise the kernel's limit
    static_assert((size_t)2 * SGPMP_MAX_T_GPMP * TS * sizeof(double) + 17648 <= 64 * 1024, "gpmp_dense_solve_kernel: call sgpmp_allow_lds");
    const size_t lds = (size_t)2 * a.T * TS * sizeof(double);
    if (dtype == SGPMP_F64)
        hipLaunchKernelGGL((gpmp_dense_solve_kernel<double>), dim3(a.P), dim3(64), lds, stream, a, da,
                           hermite_tab<double>(da.n_sub, da.dt), (double*)means, (double*)d_theta, (double*)costs);
    else
        hipLaunchKernelGGL((gpmp_dense_solve_kernel<float>), dim3(a.P), dim3(64), lds, stream, a, da,
                           hermite_tab<float>(da.n_sub, da.dt), (float*)means, (float*)d_theta, (float*)costs);
    return hipGetLastError();
}
