// SGPMP_COST_BODY_SELF (include/sgpmp.h has the definition): the kernels of the body's self-collision term, sphere pairs with radii
// under an allowed-pair mask.  The field code itself is body_self_device.h.  Three launches, none of them part of the cost sweep
// or of a fused step:
//   body_self_cost_kernel  adds K * sum_t f(q_t) to the costs the sweep has just written (launch_cost calls it behind the sweep)
//   body_self_grad_kernel  value and gradient at joint configurations (sgpmp_field_grad, the GPMP rows), and the clearance query
//   body_self_eval_kernel  the field on explicit link frames (sgpmp_field_eval)
// All three: one wave per workgroup, lane = configuration, and the wave's centre image [M][3][64] in dynamic LDS sized by the
// actual sphere count (3 * M * 64 * sizeof(real): 13.5 KiB at M = 18 in fp32, 96 KiB at M = 64 in fp64).
#include "chain_code_generated.h"
#include "sgpmp_internal.h"
#include "cost_device.h"
#include "cost_host.h"
#include "body_self_device.h"

// The table of sgpmp_set_body with the pair rows of sgpmp_set_body_pairs behind it (api.hip: one allocation).
template <typename real>
static BodySelfK<real> make_bodyselfk(const CostTerm& t) {
    BodySelfK<real> b;
    const char* base = (const char*)t.body;
    b.link = (const int*)base;
    b.sph = (const real*)(base + SGPMP_MAX_BODY * sizeof(int));
    b.rows = (const unsigned long long*)(base + SGPMP_MAX_BODY * sizeof(int) + (size_t)SGPMP_MAX_BODY * 4 * sizeof(real));
    b.n = t.n_body;
    return b;
}

static size_t body_self_lds(int dtype, int n_body) {
    return (size_t)3 * n_body * SGPMP_WAVE * (dtype == SGPMP_F64 ? sizeof(double) : sizeof(float));
}

template <typename real>
__device__ __forceinline__ real* body_self_image() {
    extern __shared__ __attribute__((aligned(16))) unsigned char body_self_smem[];
    return reinterpret_cast<real*>(body_self_smem) + (threadIdx.x & (SGPMP_WAVE - 1));
}

// One wave per trajectory, lane = waypoint 1 + lane (+ 64 per further trip; the image is reused, a lane reads only its own
// column); the lanes' sums are added across the wave in double (a butterfly: every lane ends with the same sum, in an order that
// is a function of the lane count alone) and lane 0 adds K * sum to the trajectory's cost, as body_cost_kernel does.  One writer
// per cost element, no atomics.
template <typename real>
__global__ void __launch_bounds__(SGPMP_WAVE)
body_self_cost_kernel(const ChainDev* __restrict__ chain, real K, real margin, BodySelfK<real> body, int n, int T,
                      const real* __restrict__ trajs, long long batch, real* __restrict__ costs, double* __restrict__ costs64) {
    const long long b = blockIdx.x;
    if (b >= batch) return;
    const int lane = threadIdx.x & (SGPMP_WAVE - 1);
    ChainC ch = as_const(chain);
    real* cen = body_self_image<real>();
    double part = 0;
    for (int t = 1 + lane; t < T; t += SGPMP_WAVE) {
        body_self_walk<real, 0, false>(ch, body, trajs + ((size_t)b * T + t) * 2 * n, cen, nullptr, nullptr);
        part += (double)body_self_pairs<real, 0, BSELF_VALUE>(body, margin, cen, nullptr, nullptr, nullptr);
    }
    const double add = (double)K * wave_sum(part);
    if (lane == 0) {
        if (costs) costs[b] = (real)((double)costs[b] + add);
        if (costs64) costs64[b] += add;
    }
}

hipError_t launch_body_self_cost(int dtype, int n, int T, const CostTerm& term, const ChainDev* d_chain, const void* trajs,
                                 long long batch, void* costs, double* costs64, hipStream_t stream) {
    if (batch <= 0 || T < 2) return hipSuccess;
    if (!term.body || term.n_body < 2 || term.n_body > SGPMP_MAX_BODY || batch >= (1LL << 31)) return hipErrorInvalidValue;
    const size_t lds = body_self_lds(dtype, term.n_body);
    hipError_t e;
    if (dtype == SGPMP_F64) {
        if ((e = sgpmp_allow_lds(body_self_cost_kernel<double>, lds)) != hipSuccess) return e;
        hipLaunchKernelGGL((body_self_cost_kernel<double>), dim3((unsigned)batch), dim3(SGPMP_WAVE), lds, stream, d_chain, term.K,
                           term.K2, make_bodyselfk<double>(term), n, T, (const double*)trajs, batch, (double*)costs, costs64);
    } else {
        if ((e = sgpmp_allow_lds(body_self_cost_kernel<float>, lds)) != hipSuccess) return e;
        hipLaunchKernelGGL((body_self_cost_kernel<float>), dim3((unsigned)batch), dim3(SGPMP_WAVE), lds, stream, d_chain,
                           (float)term.K, (float)term.K2, make_bodyselfk<float>(term), n, T, (const float*)trajs, batch,
                           (float*)costs, costs64);
    }
    return hipGetLastError();
}

// One lane per configuration; q laid out as body_grad_kernel's (traj_T = 0: [B, n]; traj_T = T: configuration b is waypoint
// 1 + b % (T-1) of trajectory b / (T-1) of [P, T, 2n]).  Every gradient entry is written once, by the revolute joint that owns it.
template <typename real, int NJ, int MODE>
__global__ void __launch_bounds__(SGPMP_WAVE)
body_self_grad_kernel(const ChainDev* __restrict__ chain, real margin, BodySelfK<real> body, int n, const real* __restrict__ q,
                      long long batch, int traj_T, real* __restrict__ value, real* __restrict__ grad) {
    const long long b = (long long)blockIdx.x * SGPMP_WAVE + threadIdx.x;
    if (b >= batch) return;
    const real* qb = traj_T > 0 ? q + ((size_t)(b / (traj_T - 1)) * traj_T + 1 + b % (traj_T - 1)) * 2 * n
                                : q + (size_t)b * n;
    ChainC ch = as_const(chain);
    real* cen = body_self_image<real>();
    constexpr int MJ = NJ > 0 ? NJ : SGPMP_MAX_JOINTS;
    real Z[MJ][3], Oj[MJ][3], acc[MJ];
    body_self_walk<real, NJ, true>(ch, body, qb, cen, Z, Oj);
    const real val = body_self_pairs<real, NJ, MODE>(body, margin, cen, Z, Oj, acc);
    if (value) value[b] = val;
    real* gb = grad + (size_t)b * n;
    const int nj = NJ > 0 ? NJ : ch->n_joints;
#pragma unroll
    for (int j = 0; j < MJ; ++j)
        if (j < nj && ch->j[j].revolute) gb[ch->j[j].qidx] = acc[j];
}

hipError_t launch_body_self_grad(int dtype, int n, const CostTerm& term, const ChainDev* d_chain, int n_joints, const void* q,
                                 long long batch, int traj_T, void* value, void* grad, hipStream_t stream) {
    const int block = SGPMP_WAVE;
    if (batch <= 0) return hipSuccess;
    if (!term.body || term.n_body < 2 || term.n_body > SGPMP_MAX_BODY || !grad || (batch + block - 1) / block >= (1LL << 31))
        return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((batch + block - 1) / block);
    const bool query = (term.flags & SGPMP_FLAG_GRID_DISTANCE) != 0;
    const size_t lds = body_self_lds(dtype, term.n_body);
    hipError_t e = hipSuccess;
#define BSG_LAUNCH(REAL, NJ, MODE)                                                                  \
    do {                                                                                            \
        if ((e = sgpmp_allow_lds(body_self_grad_kernel<REAL, NJ, MODE>, lds)) != hipSuccess) return e; \
        hipLaunchKernelGGL((body_self_grad_kernel<REAL, NJ, MODE>), dim3(grid), dim3(block), lds, stream, d_chain, \
                           (REAL)term.K2, make_bodyselfk<REAL>(term), n, (const REAL*)q, batch, traj_T, \
                           (REAL*)value, (REAL*)grad);                                              \
    } while (0)
#define BSG_CHAIN(REAL, MODE)                                                                       \
    do {                                                                                            \
        if (n_joints == 10 && n == 7) BSG_LAUNCH(REAL, 10, MODE);                                   \
        else if (n_joints == 7 && n == 7) BSG_LAUNCH(REAL, 7, MODE);                                \
        else BSG_LAUNCH(REAL, 0, MODE);                                                             \
    } while (0)
    if (dtype == SGPMP_F64) { if (query) BSG_CHAIN(double, BSELF_QUERY); else BSG_CHAIN(double, BSELF_GRAD); }
    else { if (query) BSG_CHAIN(float, BSELF_QUERY); else BSG_CHAIN(float, BSELF_GRAD); }
#undef BSG_CHAIN
#undef BSG_LAUNCH
    return hipGetLastError();
}

// Frames [B, n_links, 4, 4] -> f [B], one lane per configuration (the host has checked the body's last link against n_links).
template <typename real>
__global__ void __launch_bounds__(SGPMP_WAVE)
body_self_eval_kernel(real margin, BodySelfK<real> body, const real* __restrict__ frames, long long batch, int n_links,
                      real* __restrict__ out) {
    const long long b = (long long)blockIdx.x * SGPMP_WAVE + threadIdx.x;
    if (b >= batch) return;
    real* cen = body_self_image<real>();
    body_self_frames<real>(body, frames + (size_t)b * n_links * 16, cen);
    out[b] = body_self_pairs<real, 0, BSELF_VALUE>(body, margin, cen, nullptr, nullptr, nullptr);
}

hipError_t launch_body_self_eval(int dtype, const CostTerm& term, const void* frames, long long batch, int n_links, void* out,
                                 hipStream_t stream) {
    const int block = SGPMP_WAVE;
    if (batch <= 0) return hipSuccess;
    if (!term.body || term.n_body < 2 || term.n_body > SGPMP_MAX_BODY || !frames || !out || (batch + block - 1) / block >= (1LL << 31))
        return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((batch + block - 1) / block);
    const size_t lds = body_self_lds(dtype, term.n_body);
    hipError_t e;
    if (dtype == SGPMP_F64) {
        if ((e = sgpmp_allow_lds(body_self_eval_kernel<double>, lds)) != hipSuccess) return e;
        hipLaunchKernelGGL((body_self_eval_kernel<double>), dim3(grid), dim3(block), lds, stream, (double)term.K2,
                           make_bodyselfk<double>(term), (const double*)frames, batch, n_links, (double*)out);
    } else {
        if ((e = sgpmp_allow_lds(body_self_eval_kernel<float>, lds)) != hipSuccess) return e;
        hipLaunchKernelGGL((body_self_eval_kernel<float>), dim3(grid), dim3(block), lds, stream, (float)term.K2,
                           make_bodyselfk<float>(term), (const float*)frames, batch, n_links, (float*)out);
    }
    return hipGetLastError();
}
