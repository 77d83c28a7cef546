// SGPMP_COST_BODY_SDF (include/sgpmp.h has the definition): the kernels of the body collision spheres on the voxel signed-distance
// field.  The field code itself is body_device.h; the term's distance and hinge are voxel_sdf_distance / voxel_sdf_field of
// cost_device.h.  Three launches, none of them part of the cost sweep or of a fused step:
//   body_cost_kernel  adds K * sum_t f(q_t) to the costs the sweep has just written (launch_cost calls it behind the sweep)
//   body_grad_kernel  value and gradient at joint configurations (sgpmp_field_grad, the GPMP rows), and the clearance query
//   body_eval_kernel  the field on explicit link frames (sgpmp_field_eval)
#include "chain_code_generated.h"
#include "sgpmp_internal.h"
#include "cost_device.h"
#include "cost_host.h"
#include "body_device.h"

template <typename real>
static BodyK<real> make_bodyk(const CostTerm& t) {
    BodyK<real> b;
    b.link = (const int*)t.body;
    b.sph = (const real*)((const char*)t.body + SGPMP_MAX_BODY * sizeof(int));
    b.n = t.n_body;
    return b;
}

// One wave per trajectory, lane = waypoint 1 + lane (+ 64 per further trip); the lanes' sums are added across the wave in double
// (a butterfly: every lane ends with the same sum, in an order that is a function of the lane count alone) and lane 0 adds
// K * sum to the trajectory's cost, as ee_goal_kernel does.  One writer per cost element, no atomics.
template <typename real>
__global__ void __launch_bounds__(256)
body_cost_kernel(const ChainDev* __restrict__ chain, TermK<real> tm, BodyK<real> body, int n, int T,
                 const real* __restrict__ trajs, long long batch, real* __restrict__ costs, double* __restrict__ costs64) {
    const long long b = (long long)blockIdx.x * (blockDim.x / SGPMP_WAVE) + threadIdx.x / SGPMP_WAVE;
    if (b >= batch) return;                                 // (the whole wave)
    const int lane = threadIdx.x & (SGPMP_WAVE - 1);
    ChainC ch = as_const(chain);
    double part = 0;
    for (int t = 1 + lane; t < T; t += SGPMP_WAVE)
        part += (double)body_field<real, 0, BODY_VALUE>(ch, tm, body, trajs + ((size_t)b * T + t) * 2 * n, nullptr);
    const double add = (double)tm.K * wave_sum(part);
    if (lane == 0) {
        if (costs) costs[b] = (real)((double)costs[b] + add);
        if (costs64) costs64[b] += add;
    }
}

hipError_t launch_body_cost(int dtype, int n, int T, const CostTerm& term, const ChainDev* d_chain, const void* trajs,
                            long long batch, void* costs, double* costs64, hipStream_t stream) {
    const int block = 256, wpb = block / SGPMP_WAVE;
    if (batch <= 0 || T < 2) return hipSuccess;
    if (!term.body || term.n_body < 1 || term.n_body > SGPMP_MAX_BODY || (batch + wpb - 1) / wpb >= (1LL << 31))
        return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((batch + wpb - 1) / wpb);
    if (dtype == SGPMP_F64)
        hipLaunchKernelGGL((body_cost_kernel<double>), dim3(grid), dim3(block), 0, stream, d_chain, make_termk<double>(term),
                           make_bodyk<double>(term), n, T, (const double*)trajs, batch, (double*)costs, costs64);
    else
        hipLaunchKernelGGL((body_cost_kernel<float>), dim3(grid), dim3(block), 0, stream, d_chain, make_termk<float>(term),
                           make_bodyk<float>(term), n, T, (const float*)trajs, batch, (float*)costs, costs64);
    return hipGetLastError();
}

// One thread per configuration; q laid out as field_grad_kernel's (traj_T = 0: [B, n]; traj_T = T: configuration b is waypoint
// 1 + b % (T-1) of trajectory b / (T-1) of [P, T, 2n]).  Every gradient entry is written once, by the revolute joint that owns it:
// a context's chain has exactly n = n_dof revolute joints with qidx 0 .. n-1 (sgpmp_set_fk refuses any other chain), and the
// callers (sgpmp_field_grad, sgpmp_gpmp_linearize) refuse the term without a chain.
template <typename real, int NJ, int MODE>
__global__ void __launch_bounds__(64)
body_grad_kernel(const ChainDev* __restrict__ chain, TermK<real> tm, BodyK<real> body, int n, const real* __restrict__ q,
                 long long batch, int traj_T, real* __restrict__ value, real* __restrict__ grad) {
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const real* qb = traj_T > 0 ? q + ((size_t)(b / (traj_T - 1)) * traj_T + 1 + b % (traj_T - 1)) * 2 * n
                                : q + (size_t)b * n;
    ChainC ch = as_const(chain);
    constexpr int MJ = NJ > 0 ? NJ : SGPMP_MAX_JOINTS;
    real acc[MJ];
    const real val = body_field<real, NJ, MODE>(ch, tm, body, qb, acc);
    if (value) value[b] = val;
    real* gb = grad + (size_t)b * n;
    const int nj = NJ > 0 ? NJ : ch->n_joints;
#pragma unroll
    for (int j = 0; j < MJ; ++j)
        if (j < nj && ch->j[j].revolute) gb[ch->j[j].qidx] = acc[j];
}

hipError_t launch_body_grad(int dtype, int n, const CostTerm& term, const ChainDev* d_chain, int n_joints, const void* q,
                            long long batch, int traj_T, void* value, void* grad, hipStream_t stream) {
    const int block = 64;
    if (batch <= 0) return hipSuccess;
    if (!term.body || term.n_body < 1 || term.n_body > SGPMP_MAX_BODY || !grad || (batch + block - 1) / block >= (1LL << 31))
        return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((batch + block - 1) / block);
    const bool query = (term.flags & SGPMP_FLAG_GRID_DISTANCE) != 0;
#define BG_LAUNCH(REAL, NJ, MODE)                                                                   \
    hipLaunchKernelGGL((body_grad_kernel<REAL, NJ, MODE>), dim3(grid), dim3(block), 0, stream, d_chain, \
                       make_termk<REAL>(term), make_bodyk<REAL>(term), n, (const REAL*)q, batch, traj_T, \
                       (REAL*)value, (REAL*)grad)
#define BG_CHAIN(REAL, MODE)                                                                        \
    do {                                                                                            \
        if (n_joints == 10 && n == 7) BG_LAUNCH(REAL, 10, MODE);                                    \
        else if (n_joints == 7 && n == 7) BG_LAUNCH(REAL, 7, MODE);                                 \
        else BG_LAUNCH(REAL, 0, MODE);                                                              \
    } while (0)
    if (dtype == SGPMP_F64) { if (query) BG_CHAIN(double, BODY_QUERY); else BG_CHAIN(double, BODY_GRAD); }
    else { if (query) BG_CHAIN(float, BODY_QUERY); else BG_CHAIN(float, BODY_GRAD); }
#undef BG_CHAIN
#undef BG_LAUNCH
    return hipGetLastError();
}

// Frames [B, n_links, 4, 4] -> f [B], one thread per configuration (the host has checked the body's last link against n_links).
template <typename real>
__global__ void __launch_bounds__(64)
body_eval_kernel(TermK<real> tm, BodyK<real> body, const real* __restrict__ frames, long long batch, int n_links,
                 real* __restrict__ out) {
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    out[b] = body_field_frames<real>(tm, body, frames + (size_t)b * n_links * 16);
}

hipError_t launch_body_eval(int dtype, const CostTerm& term, const void* frames, long long batch, int n_links, void* out,
                            hipStream_t stream) {
    const int block = 64;
    if (batch <= 0) return hipSuccess;
    if (!term.body || term.n_body < 1 || term.n_body > SGPMP_MAX_BODY || !frames || !out || (batch + block - 1) / block >= (1LL << 31))
        return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((batch + block - 1) / block);
    if (dtype == SGPMP_F64)
        hipLaunchKernelGGL((body_eval_kernel<double>), dim3(grid), dim3(block), 0, stream, make_termk<double>(term),
                           make_bodyk<double>(term), (const double*)frames, batch, n_links, (double*)out);
    else
        hipLaunchKernelGGL((body_eval_kernel<float>), dim3(grid), dim3(block), 0, stream, make_termk<float>(term),
                           make_bodyk<float>(term), (const float*)frames, batch, n_links, (float*)out);
    return hipGetLastError();
}
