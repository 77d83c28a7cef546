// K4 -- exponentiated-cost reweight and mean update;  K5 -- importance-sampling weights.
//
// K4 replaces StochGPMP._update_distribution (planner.py:263-275):
//     w = softmax(-costs / temperature, dim=samples);  grad = sum_s w_s (x_s - mu);
//     mu += step_size * grad
// (the reference then rebuilds a MultivariateNormal -> a [P,M,M] Cholesky -- per iteration; the
// factor does not depend on the mean, so nothing is left to do here).
// One workgroup per particle: the S costs are reduced in LDS, then threads stride over the M = T*d
// trajectory elements, each streaming its column of the [S, M] sample block (coalesced rows).
//
// K5 replaces the Sigma_inv @ mu part of StochGPMP._get_costs (planner.py:233-236) in factored form:
//     x^T Sigma^-1 mu = (A x)^T a,   a = blkdiag(K_s, Q^-1 x (T-1), K_g) (A mu)
// with A x = (x_0, e_0(x), .., e_{T-2}(x), x_{T-1}) (mp_priors_multi.py:185-198); `a` is computed in
// fp64 once per particle per iteration and consumed by the cost sweep (K3).  The last block
// (x_{T-1} . K_g mu_{T-1}) is re-expressed on (x_0, e_0, ..) and folded into the first T blocks, so
// K3 needs exactly one weight vector per waypoint.
#include <hip/hip_ext.h>
#include <cstring>

#include "sgpmp_internal.h"
#include "update_common.h"

// update_kernel with ONE WAVE per particle: wave w of workgroup b updates particle 4 b + w in its own slice of the dynamic
// LDS (update_particle<.., 64>: no workgroup barrier, the four particles do not wait for each other), then ONE barrier and one
// importance-sampling tail for the four particles with all 256 threads (is_weight_elem of the owning particle's means in
// LDS: a pure function of (means, e), the bits of update_kernel's tail).  A quarter of update_kernel's waves: inside a
// two-chain optimize() the update runs under the other chain's fused launch, where every wave waits for a slot, and its
// duration there is serial in its own chain -- 55.9 -> 45.9 us per half at the headline shape (profiles/r12).
// Storing steps without a folded end-effector term only (update_plan.hip: plan_update).
template <typename real, typename cost_t, int VW>
__global__ void __launch_bounds__(256)
update_kernel_quad(int M, int S, int P, const cost_t* __restrict__ costs, const real* __restrict__ samples,
                   real* __restrict__ means, double temperature, double step_size,
                   real* __restrict__ weights, real* __restrict__ grad, real* __restrict__ means_prev,
                   double* __restrict__ stats, IswNext<real> nx, real* __restrict__ means_copy,
                   const float* __restrict__ part, int gpp, unsigned* __restrict__ nnz, unsigned nnz_threshold,
                   unsigned slice_bytes) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int p0 = (int)blockIdx.x * SGPMP_UPD_QUAD, p = p0 + wave;
    // (issued first, consumed last -- as in update_particle's own tail)
    const bool iso_tail = nx.out && nx.isotropic;
    const int nd = 2 * nx.n;
    const double q00 = iso_tail ? nx.Qinv[0] : 0., q01 = iso_tail ? nx.Qinv[nx.n] : 0.;
    const double q10 = iso_tail ? nx.Qinv[nx.n * nd] : 0., q11 = iso_tail ? nx.Qinv[nx.n * nd + nx.n] : 0.;
    if (p < P) {                                         // (a wave without a particle goes straight to the barrier)
        const unsigned prev = nnz ? nnz[p] : 0u;         // partials exist iff THIS step's launch saw the count above the threshold
        const float* part_p = nullptr;
        if (part && nnz && prev > nnz_threshold) part_p = part + (size_t)p * gpp * (M + 4);
        update_particle<real, cost_t, VW, 64>(p, M, S, costs + (size_t)p * S, samples + (size_t)p * S * M, (size_t)M, means,
                                              temperature, step_size, weights, grad, means_prev, stats, nx, means_copy,
                                              lds_raw + (size_t)wave * slice_bytes, nullptr, part_p, gpp, nnz ? nnz + p : nullptr);
    }
    if (nx.out) {
        __syncthreads();                                  // the new means of the workgroup's particles are in their slices
        const int Tn = M / nd, E = (Tn + 1) * nd;         // elements per particle; particle p0 + q owns [q E, (q + 1) E)
        const int live = P - p0 < SGPMP_UPD_QUAD ? P - p0 : SGPMP_UPD_QUAD;
        const size_t mu_off = upd_means_offset(S);
        real* out = nx.out + (size_t)p0 * E;
        for (int i = threadIdx.x; i < live * E; i += SGPMP_UPD_THREADS) {
            const int q = i / E, e = i - q * E;
            const real* mu_new = reinterpret_cast<const real*>(lds_raw + (size_t)q * slice_bytes + mu_off);
            out[i] = iso_tail ? is_weight_elem_iso<real>(nx.n, Tn, mu_new, q00, q01, q10, q11, nx.ks, nx.kg, nx.dt, temperature, e)
                              : is_weight_elem<real>(nx.n, Tn, mu_new, nx.Qinv, nx.ks, nx.kg, nx.dt, temperature, nx.isotropic, e);
        }
    }
}

// One update launch: the tail's descriptor, the folded term, either kernel.  `done` (multi-GPU statistics): the event is signalled
// by this kernel's own dispatch packet (hipExtLaunchKernelGGL stop event) instead of a separate barrier packet behind it
template <typename real, typename cost_t, int VW>
static void enqueue_update(const UpdatePlan& pl, const UpdateIo& io, const RegenArgs& rg) {
    const int n = pl.shape.n, T = pl.shape.T, S = pl.shape.S, M = T * 2 * n;
    const PriorDev* pr = pl.tail ? io.isw_prior : nullptr;
    const IswNext<real> nx = {pr ? (real*)io.isw_next : nullptr, pr ? pr->Qinv : nullptr, pr ? pr->ks : 0., pr ? pr->kg : -1.,
                              pr ? pr->dt : 0., n, pr ? pr->isotropic : 1};
    const float* part = sizeof(real) == 4 && VW == 4 ? io.part : nullptr;
    const dim3 grid(pl.grid), block(SGPMP_UPD_THREADS);
    if (pl.quad) {
        hipExtLaunchKernelGGL((update_kernel_quad<real, cost_t, VW>), grid, block, pl.lds, io.stream, (hipEvent_t) nullptr, io.done, 0u, M, S,
                              pl.shape.P, (const cost_t*)io.costs, (const real*)io.samples, (real*)io.means, io.temperature, io.step_size,
                              (real*)io.weights, (real*)io.grad, (real*)io.means_prev, io.stats, nx, (real*)io.means_copy, part, (S + 7) / 8,
                              io.nnz, io.nnz_threshold, pl.slice);
        return;
    }
    const EeFold<real> ee = io.ee.term ? EeFold<real>{io.ee.d_chain, make_ee_target<real>(*io.ee.term), n, T, (real*)io.ee.costs}
                                       : EeFold<real>{nullptr, EeTarget<real>{}, n, T, nullptr};
    hipExtLaunchKernelGGL((update_kernel<real, cost_t, VW>), grid, block, pl.lds, io.stream, (hipEvent_t) nullptr, io.done, 0u, M, S,
                          (const cost_t*)io.costs, (const real*)io.samples, (real*)io.means, io.temperature, io.step_size, (real*)io.weights,
                          (real*)io.grad, (real*)io.means_prev, io.stats, nx, (real*)io.means_copy, part, (S + 7) / 8, io.nnz,
                          io.nnz_threshold, rg, pl.regen_off, ee, pl.ee_off);
}

hipError_t launch_update(const UpdatePlan& pl, const UpdateIo& io) {
    if (!pl.ok) return hipErrorInvalidValue;
    if (pl.shape.P <= 0) return hipSuccess;
    // store-free step: the rows with weight are regenerated behind the kernel's usual scratch
    RegenArgs rg;
    std::memset(&rg, 0, sizeof(rg));
    if (const RegenHost& r = io.regen; r.recipe != 0) {
        rg.recipe = r.recipe; rg.N = pl.shape.n; rg.L = r.L; rg.R = pl.regen_rows; rg.seed = r.seed; rg.draw = r.draw;
        rg.mode_offset = r.mode_offset; rg.coef = r.coef; rg.pre = r.pre; rg.store_threshold = r.store_threshold;
    }
    auto go = [&](auto real_tag, auto cost_tag) {
        using real = decltype(real_tag); using cost_t = decltype(cost_tag);
        if (pl.vw == 4) enqueue_update<real, cost_t, 4>(pl, io, rg); else enqueue_update<real, cost_t, 2>(pl, io, rg);
    };
    if (pl.shape.dtype == SGPMP_F64) go(double{}, double{});
    else if (pl.shape.costs_dtype == SGPMP_F64) go(float{}, double{});
    else go(float{}, float{});
    return hipGetLastError();
}

// Per-goal statistics of the particle means -- what the multi-GPU all-reduce carries besides the cost sums (SURVEY.md
// 8e: "per-goal sum_p mu_p and sum_p mu_p mu_p^T-diagonal"; north_star: "weighted-mean/covariance statistics"): the
// modes of the trajectory distribution are the goals (p = g * nppg + k, planner.py:215), and the first two moments of
// a mode's particles are what a covariance adaptation (MultiMPPrior.set_Sigma_invs, mp_priors_multi.py:125-128) or a
// mode summary would consume.  out [G][M + 1][2] doubles is ACCUMULATED into (zero it first): [g][m] = (sum of
// mu_p[m], sum of mu_p[m]^2) over this shard's particles of goal g, [g][M] = (their number, 0).
// grid = (ceil((M + 1) / 64), G), 1024 threads: lane = element, the 16 waves take the goal's particles of this shard
// round-robin; the waves' partial sums meet in LDS and are added in wave order -- NO atomics, so the sums are bitwise
// reproducible run to run for a given sharding (round 3's version added up to 32 slices with fp64 atomics in whatever
// order they arrived).  Across different shardings the order of the additions differs: equal to rounding only.
#define SGPMP_MS_WAVES 16
template <typename real>
__global__ void __launch_bounds__(64 * SGPMP_MS_WAVES)
mode_stats_kernel(int M, int P, long long p_offset, int nppg, int G, const real* __restrict__ means,
                  double* __restrict__ out) {
    __shared__ double red[SGPMP_MS_WAVES][64][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = blockIdx.x * 64 + lane;
    const int g = blockIdx.y;
    // local particles of goal g: global [g nppg, (g + 1) nppg) -- the last goal also takes what lies beyond (as the
    // clamp min(G - 1, p / nppg) of the cost kernels does) -- cut to this shard [p_offset, p_offset + P)
    const long long lo = (long long)g * nppg, hi = g == G - 1 ? (long long)1 << 62 : lo + nppg;
    const long long a = lo > p_offset ? lo - p_offset : 0;
    const long long b = hi - p_offset < (long long)P ? hi - p_offset : (long long)P;
    double s1 = 0., s2 = 0.;
    if (m < M) {
        long long p = a + wave;
        for (; p + 3 * SGPMP_MS_WAVES < b; p += 4 * SGPMP_MS_WAVES) {            // four independent loads in flight
            const double v0 = (double)means[(size_t)p * M + m], v1 = (double)means[(size_t)(p + SGPMP_MS_WAVES) * M + m];
            const double v2 = (double)means[(size_t)(p + 2 * SGPMP_MS_WAVES) * M + m];
            const double v3 = (double)means[(size_t)(p + 3 * SGPMP_MS_WAVES) * M + m];
            s1 += v0; s2 += v0 * v0; s1 += v1; s2 += v1 * v1; s1 += v2; s2 += v2 * v2; s1 += v3; s2 += v3 * v3;
        }
        for (; p < b; p += SGPMP_MS_WAVES) {
            const double v = (double)means[(size_t)p * M + m];
            s1 += v; s2 += v * v;
        }
    }
    red[wave][lane][0] = s1; red[wave][lane][1] = s2;
    __syncthreads();
    if (wave == 0) {
        double t1 = red[0][lane][0], t2 = red[0][lane][1];
#pragma unroll
        for (int w = 1; w < SGPMP_MS_WAVES; ++w) { t1 += red[w][lane][0]; t2 += red[w][lane][1]; }
        double* o = out + ((size_t)g * (M + 1) + m) * 2;
        if (m < M) { o[0] += t1; o[1] += t2; }                                   // (ACCUMULATES, as documented: one writer per element)
        else if (m == M) o[0] += (double)(b > a ? b - a : 0);
    }
}

hipError_t launch_mode_stats(int dtype, int n, int T, int P, long long p_offset, int nppg, int G, const void* means,
                             double* out, hipStream_t stream) {
    if (P <= 0) return hipSuccess;
    const int M = T * 2 * n;
    dim3 grid((unsigned)((M + 1 + 63) / 64), (unsigned)G), block(64 * SGPMP_MS_WAVES);
    if (dtype == SGPMP_F64)
        hipLaunchKernelGGL((mode_stats_kernel<double>), grid, block, 0, stream, M, P, p_offset, nppg, G, (const double*)means, out);
    else
        hipLaunchKernelGGL((mode_stats_kernel<float>), grid, block, 0, stream, M, P, p_offset, nppg, G, (const float*)means, out);
    return hipGetLastError();
}

// statistics of the second particle half of a pipelined step (api.hip, StepPipe) added to the first half's
__global__ void stats_add_kernel(double* __restrict__ dst, const double* __restrict__ src) {
    if (threadIdx.x < SGPMP_STAT_SHARDS * 4) dst[threadIdx.x] += src[threadIdx.x];
}

hipError_t launch_stats_add(double* dst, const double* src, hipStream_t stream) {
    hipLaunchKernelGGL(stats_add_kernel, dim3(1), dim3(SGPMP_STAT_SHARDS * 4), 0, stream, dst, src);
    return hipGetLastError();
}

// K5: one thread per (particle, block row t in [0,T], component i).
template <typename real>
__global__ void is_weights_kernel(int n, int T, int P, const real* __restrict__ means,
                                  const double* __restrict__ Qinv, double ks, double kg, double dt,
                                  double temperature, int isotropic, real* __restrict__ out,
                                  double* __restrict__ zero_stats) {
    const int d = 2 * n;
    // grid = (ceil((T+1) d / 256), P): 32-bit index arithmetic (64-bit div / mod cost more than the math)
    const int p = blockIdx.y;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (zero_stats && p == 0 && e < SGPMP_STAT_SHARDS * 4) zero_stats[e] = 0.;   // this step's statistics start from zero
    if (e >= (T + 1) * d) return;
    out[(size_t)p * (T + 1) * d + e] = is_weight_elem<real>(n, T, means + (size_t)p * T * d, Qinv, ks, kg, dt,
                                                             temperature, isotropic, e);
}

hipError_t launch_is_weights(int dtype, int n, int T, const PriorDev& prior, const void* means,
                             int n_particles, double temperature, void* out, double* zero_stats,
                             hipStream_t stream) {
    const long long total = (long long)n_particles * (T + 1) * 2 * n;
    if (total <= 0) return hipSuccess;
    const int block = 256;
    const dim3 grid((unsigned)(((T + 1) * 2 * n + block - 1) / block), (unsigned)n_particles);
    if (dtype == SGPMP_F64)
        hipLaunchKernelGGL((is_weights_kernel<double>), grid, dim3(block), 0, stream, n, T,
                           n_particles, (const double*)means, prior.Qinv, prior.ks, prior.kg, prior.dt,
                           temperature, prior.isotropic, (double*)out, zero_stats);
    else
        hipLaunchKernelGGL((is_weights_kernel<float>), grid, dim3(block), 0, stream, n, T,
                           n_particles, (const float*)means, prior.Qinv, prior.ks, prior.kg, prior.dt,
                           temperature, prior.isotropic, (float*)out, zero_stats);
    return hipGetLastError();
}
