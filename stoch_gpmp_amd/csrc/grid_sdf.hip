// Signed-distance grid field (SGPMP_COST_GRID_SDF; include/sgpmp.h has the definition): the exact Euclidean distance transform
// of an occupancy grid on the device, and the term's value / gradient kernel behind sgpmp_field_grad and the GPMP rows.  The
// field function itself is grid_sdf_field in cost_device.h, shared with the sweep and the dense-trajectory kernels.
#include <cstdio>

#include "chain_code_generated.h"
#include "sgpmp_internal.h"
#include "cost_device.h"
#include "cost_host.h"

// ---------------------------------------------------------------------------------- the transform
// Separable and exact (integers until the one square root).  A cell is either occupied or free, so of its two column distances
// -- to the nearest occupied and to the nearest free cell of its column -- one is zero: pass 1 leaves ONE signed number per
// cell in the output buffer itself, + the distance in cells to the nearest occupied cell of the column for a free cell,
// - the distance to the nearest free one for an occupied cell (SDF_NONE where the column has none), as a value of the
// context's type (integers up to 8192 are exact in fp32).  No scratch memory, no allocation.
#define SDF_NONE 8192                  // > any distance in a 4096 x 4096 grid; NONE^2 + 4095^2 fits an int
#define SDF_MAX_DIM 4096

// Pass 1: one thread per column (a wave reads and writes consecutive cells of a row), down the column and back up.
template <typename real>
__global__ void __launch_bounds__(256)
grid_sdf_columns_kernel(const real* __restrict__ occ, int ny, int nx, double threshold, real* __restrict__ out) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= nx) return;
    int to_occ = SDF_NONE, to_free = SDF_NONE;             // rows since the last occupied / free cell above
    for (int y = 0; y < ny; ++y) {
        const bool o = (double)occ[(size_t)y * nx + x] > threshold;
        to_occ = o ? 0 : (to_occ < SDF_NONE ? to_occ + 1 : SDF_NONE);
        to_free = o ? (to_free < SDF_NONE ? to_free + 1 : SDF_NONE) : 0;
        out[(size_t)y * nx + x] = o ? (real)-to_free : (real)to_occ;
    }
    to_occ = SDF_NONE; to_free = SDF_NONE;
    for (int y = ny - 1; y >= 0; --y) {
        const real down = out[(size_t)y * nx + x];
        const bool o = down < (real)0;
        to_occ = o ? 0 : (to_occ < SDF_NONE ? to_occ + 1 : SDF_NONE);
        to_free = o ? (to_free < SDF_NONE ? to_free + 1 : SDF_NONE) : 0;
        const int d = (int)(o ? -down : down), up = o ? to_free : to_occ;
        const int m = up < d ? up : d;
        out[(size_t)y * nx + x] = o ? (real)-m : (real)m;
    }
}

// Pass 2: one workgroup per row, the row's two integer arrays staged in LDS (every lane reads the same word per step: a
// broadcast), per cell the minimum over the row of (x - x')^2 + g(x')^2.  The row is read before any of it is overwritten, and
// no other workgroup touches it.
template <typename real>
__global__ void __launch_bounds__(256)
grid_sdf_rows_kernel(int ny, int nx, double cell, real* __restrict__ sdf) {
    __shared__ int g_occ[SDF_MAX_DIM], g_free[SDF_MAX_DIM];
    real* row = sdf + (size_t)blockIdx.x * nx;
    for (int x = threadIdx.x; x < nx; x += blockDim.x) {
        const int v = (int)row[x];
        g_occ[x] = v > 0 ? v : 0;
        g_free[x] = v < 0 ? -v : 0;
    }
    __syncthreads();
    const double cap = cell * (double)(nx + ny);
    for (int x = threadIdx.x; x < nx; x += blockDim.x) {
        const bool o = g_occ[x] == 0;                      // occupied: its distance to an occupied cell is zero
        const int* g = o ? g_free : g_occ;
        int best = SDF_NONE * SDF_NONE;
        for (int xp = 0; xp < nx; ++xp) {
            const int dx = x - xp, gy = g[xp];
            const int c = dx * dx + gy * gy;
            best = c < best ? c : best;
        }
        double s = best >= SDF_NONE * SDF_NONE ? cap : (__dsqrt_rn((double)best) - 0.5) * cell;
        row[x] = (real)(o ? -s : s);
    }
}

template <typename real>
static hipError_t launch_grid_sdf_build(const void* occ, int ny, int nx, double cell, double threshold, void* sdf,
                                        hipStream_t stream) {
    hipLaunchKernelGGL((grid_sdf_columns_kernel<real>), dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, stream,
                       (const real*)occ, ny, nx, threshold, (real*)sdf);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((grid_sdf_rows_kernel<real>), dim3((unsigned)ny), dim3(256), 0, stream, ny, nx, cell, (real*)sdf);
    return hipGetLastError();
}

extern "C" int sgpmp_grid_sdf_build(sgpmp_ctx* c, const void* occ, int ny, int nx, double cell, double threshold, void* sdf,
                                    void* stream) {
    if (!c || !occ || !sdf || occ == sdf || ny < 1 || nx < 1 || ny > SDF_MAX_DIM || nx > SDF_MAX_DIM || !(cell > 0.) ||
        !(threshold == threshold))
        return sgpmp_set_error(SGPMP_EINVAL, "sgpmp_grid_sdf_build: bad argument (distinct non-null occ and sdf, 1 <= ny, nx <= 4096, "
                                             "cell > 0, a threshold that is not NaN)");
    const hipError_t e = sgpmp_ctx_dtype(c) == SGPMP_F64
        ? launch_grid_sdf_build<double>(occ, ny, nx, cell, threshold, sdf, (hipStream_t)stream)
        : launch_grid_sdf_build<float>(occ, ny, nx, cell, threshold, sdf, (hipStream_t)stream);
    if (e != hipSuccess) {
        char msg[160];
        snprintf(msg, sizeof(msg), "sgpmp_grid_sdf_build: HIP error: %s", hipGetErrorString(e));
        return sgpmp_set_error(SGPMP_EHIP, msg);
    }
    return SGPMP_OK;
}

// ---------------------------------------------------------------------------------- value and gradient of the term
// One thread per configuration; q as field_grad_kernel reads it (traj_T = 0: [B, n]; traj_T = T: waypoint 1 + b % (T-1) of
// trajectory b / (T-1) of [P, T, 2n]).
template <typename real>
__global__ void __launch_bounds__(64)
grid_sdf_grad_kernel(TermK<real> tm, int n, const real* __restrict__ q, long long batch, int traj_T, real* __restrict__ value,
                     real* __restrict__ grad) {
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const real* qb = traj_T > 0 ? q + ((size_t)(b / (traj_T - 1)) * traj_T + 1 + b % (traj_T - 1)) * 2 * n
                                : q + (size_t)b * n;
    real gx, gy, h;
    if (tm.flags & SGPMP_FLAG_GRID_DISTANCE) {             // the interpolated distance d itself and dd/d(x, y)
        h = grid_sdf_distance<real, true>(tm, qb[0], qb[1], &gx, &gy);
        if (!(h == h)) { gx = h; gy = h; }
    } else {
        h = grid_sdf_field<real, true>(tm, qb[0], qb[1], &gx, &gy);
    }
    if (value) value[b] = h;
    real* gb = grad + (size_t)b * n;
    gb[0] = gx; gb[1] = gy;
    for (int k = 2; k < n; ++k) gb[k] = 0;
}

hipError_t launch_grid_sdf_grad(int dtype, int n, const CostTerm& term, const void* q, long long batch, int traj_T, void* value,
                                void* grad, hipStream_t stream) {
    const int block = 64;
    const unsigned grid = (unsigned)((batch + block - 1) / block);
    if (grid == 0) return hipSuccess;
    if (dtype == SGPMP_F64)
        hipLaunchKernelGGL((grid_sdf_grad_kernel<double>), dim3(grid), dim3(block), 0, stream, make_termk<double>(term), n,
                           (const double*)q, batch, traj_T, (double*)value, (double*)grad);
    else
        hipLaunchKernelGGL((grid_sdf_grad_kernel<float>), dim3(grid), dim3(block), 0, stream, make_termk<float>(term), n,
                           (const float*)q, batch, traj_T, (float*)value, (float*)grad);
    return hipGetLastError();
}
