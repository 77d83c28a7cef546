// Signed-distance fields on occupancy (SGPMP_COST_GRID_SDF: a planar grid, SGPMP_COST_VOXEL_SDF: a volume; include/sgpmp.h has the
// definitions): ONE exact Euclidean distance transform on the device behind both builders, and the grid term's value / gradient
// kernel behind sgpmp_field_grad and the GPMP rows.  The field functions themselves are grid_sdf_field and voxel_sdf_field in
// cost_device.h, shared with the sweep, the dense-trajectory kernels and field_eval_kernel / field_grad_kernel (cost_sweep.hip).
#include <cstdio>

#include "chain_code_generated.h"
#include "sgpmp_internal.h"
#include "cost_device.h"
#include "cost_host.h"

// ---------------------------------------------------------------------------------- the transform
// Separable and exact (integers until the one square root), in place in the output buffer: no scratch memory, no allocation.
// A cell is either occupied or free, so of its two distances -- to the nearest occupied and to the nearest free cell -- one is
// zero: every pass leaves ONE signed number per cell, + towards the nearest occupied cell seen so far for a free cell, - towards
// the nearest free one for an occupied cell (never zero: the sign IS the occupancy), as a value of the context's type.
//
// The grid (2 passes) and the volume (3 passes) differ in what that number is between the passes, the template parameter
// SQUARED of the kernels below, and both choices are forced:
//   * the grid's first pass leaves the run length UNSQUARED: a squared distance on a 4096 x 4096 grid reaches 2 * 4095^2 > 2^24
//     and is not exact in fp32, a run length (<= SDF_NONE = 8192) is; its last pass squares in int as it reads.  A volume is at
//     most 512 per axis, 3 * 511^2 = 783 363 < 2^20, so it can -- and with a middle pass between, must -- carry squares;
//   * the sentinels ("there is no such cell") stay distinct: SDF_NONE = 8192 on the grid's run lengths (the last pass compares
//     against 8192^2; 8192^2 + 4095^2 fits an int), VOX_NONE = 2^20 on the volume's squares (exact in fp32).  Where there is no
//     cell of the other kind the result is the cap, cell * (nx + ny) or cell * (nx + ny + nz).
#define SDF_NONE 8192
#define SDF_MAX_DIM 4096
#define VOX_NONE (1 << 20)
#define VOX_MAX_DIM 512
#define VOX_TILE_X 32                  // y pass: x columns per workgroup; the [ny][32] int tile is <= 64 KiB of LDS
#define VOX_TILE_Y 8                   // y pass: 256 threads = 32 columns x 8 row groups, a thread takes rows yg, yg + 8, ...

// First pass, down the slowest axis: one thread per line of `count` cells at `stride` (grid: a column, count = ny, stride = nx;
// volume: a (y, x) column, count = nz, stride = ny * nx -- there are `stride` lines, and consecutive lanes are on consecutive
// cells), forwards and back.  Leaves the signed run length, squared on the way back where SQUARED.
template <typename real, bool SQUARED>
__global__ void __launch_bounds__(256)
sdf_line_scan_kernel(const real* __restrict__ occ, int count, int stride, double threshold, real* __restrict__ out) {
    constexpr int NONE = SQUARED ? VOX_NONE : SDF_NONE;
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= stride) return;
    int to_occ = NONE, to_free = NONE;                         // cells since the last occupied / free one (NONE: none yet)
    for (int i = 0; i < count; ++i) {
        const size_t at = (size_t)i * stride + c;
        const bool o = (double)occ[at] > threshold;
        to_occ = o ? 0 : (to_occ < NONE ? to_occ + 1 : NONE);
        to_free = o ? (to_free < NONE ? to_free + 1 : NONE) : 0;
        out[at] = o ? (real)-to_free : (real)to_occ;
    }
    to_occ = NONE; to_free = NONE;
    for (int i = count - 1; i >= 0; --i) {
        const size_t at = (size_t)i * stride + c;
        const real fwd = out[at];
        const bool o = fwd < (real)0;
        to_occ = o ? 0 : (to_occ < NONE ? to_occ + 1 : NONE);
        to_free = o ? (to_free < NONE ? to_free + 1 : NONE) : 0;
        const int d = (int)(o ? -fwd : fwd), back = o ? to_free : to_occ;
        const int m = back < d ? back : d;
        const int r = !SQUARED ? m : m < NONE ? m * m : NONE;
        out[at] = o ? (real)-r : (real)r;
    }
}

// Pass y of a volume: one workgroup per (z, 32 x columns); the [ny][32] signed tile is staged in LDS before any of it is
// overwritten, and no other workgroup touches it.  Lanes along x: the global accesses are 128-byte runs, the LDS reads of a wave 32
// consecutive words (its two row groups read the same words: a broadcast).  Per cell the minimum over y' of (y - y')^2 + g(y').
template <typename real>
__global__ void __launch_bounds__(VOX_TILE_X * VOX_TILE_Y)
voxel_sdf_y_kernel(int ny, int nx, real* __restrict__ sdf) {
    extern __shared__ int vox_tile[];                          // [ny][VOX_TILE_X]
    const int xl = threadIdx.x % VOX_TILE_X, yg = threadIdx.x / VOX_TILE_X;
    const int x = blockIdx.x * VOX_TILE_X + xl;
    real* slice = sdf + (size_t)blockIdx.y * ny * nx;
    const bool in = x < nx;
    for (int y = yg; y < ny; y += VOX_TILE_Y) vox_tile[y * VOX_TILE_X + xl] = in ? (int)slice[(size_t)y * nx + x] : VOX_NONE;
    __syncthreads();
    if (!in) return;
    for (int y = yg; y < ny; y += VOX_TILE_Y) {
        const bool o = vox_tile[y * VOX_TILE_X + xl] < 0;
        int best = VOX_NONE;
        for (int yp = 0; yp < ny; ++yp) {
            const int v = vox_tile[yp * VOX_TILE_X + xl];
            const int g = o ? (v < 0 ? -v : 0) : (v > 0 ? v : 0);    // squared distance along z to a cell of the OTHER kind
            const int dy = y - yp;
            const int c = dy * dy + g;
            best = c < best ? c : best;
        }
        slice[(size_t)y * nx + x] = o ? (real)-best : (real)best;
    }
}

// Last pass, along x: one workgroup per row of at most CAPACITY cells, the row staged in LDS (every lane reads the same word per
// step: a broadcast) before any of it is overwritten -- no other workgroup touches it --, per cell the minimum over x' of
// (x - x')^2 + g(x'), then the one square root.  Where not SQUARED the row holds run lengths, squared here as they are read.
// The row is split into two arrays of squares, towards the occupied and towards the free cells (0 at a cell of the kind itself),
// so that the inner loop is a read, a multiply-add and a minimum: picking the side from ONE signed array per candidate cost the
// 2048 x 2048 grid 19 % of its build time.
template <typename real, bool SQUARED, int CAPACITY>
__global__ void __launch_bounds__(256)
sdf_last_axis_kernel(int nx, double cell, double cap, real* __restrict__ sdf) {
    constexpr int NONE = SQUARED ? VOX_NONE : SDF_NONE * SDF_NONE;
    __shared__ int g_occ[CAPACITY], g_free[CAPACITY];
    real* row = sdf + (size_t)blockIdx.x * nx;
    for (int x = threadIdx.x; x < nx; x += blockDim.x) {
        const int v = (int)row[x], sq = SQUARED ? (v < 0 ? -v : v) : v * v;
        g_occ[x] = v > 0 ? sq : 0;
        g_free[x] = v < 0 ? sq : 0;
    }
    __syncthreads();
    for (int x = threadIdx.x; x < nx; x += blockDim.x) {
        const bool o = g_occ[x] == 0;                      // occupied: its distance to an occupied cell is zero
        const int* g = o ? g_free : g_occ;
        int best = NONE;
        for (int xp = 0; xp < nx; ++xp) {
            const int dx = x - xp;
            const int c = dx * dx + g[xp];
            best = c < best ? c : best;
        }
        const double s = best >= NONE ? cap : (__dsqrt_rn((double)best) - 0.5) * cell;
        row[x] = (real)(o ? -s : s);
    }
}

// The passes of one build on `stream`; a grid is VOLUME = false with nz = 1.
template <typename real, bool VOLUME>
static hipError_t launch_sdf_build(const void* occ, int nz, int ny, int nx, double cell, double threshold, void* sdf,
                                   hipStream_t stream) {
    const int lines = VOLUME ? ny * nx : nx;
    hipLaunchKernelGGL((sdf_line_scan_kernel<real, VOLUME>), dim3((unsigned)((lines + 255) / 256)), dim3(256), 0, stream,
                       (const real*)occ, VOLUME ? nz : ny, lines, threshold, (real*)sdf);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (VOLUME) {
        hipLaunchKernelGGL((voxel_sdf_y_kernel<real>), dim3((unsigned)((nx + VOX_TILE_X - 1) / VOX_TILE_X), (unsigned)nz),
                           dim3(VOX_TILE_X * VOX_TILE_Y), (size_t)ny * VOX_TILE_X * sizeof(int), stream, ny, nx, (real*)sdf);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const int block = !VOLUME ? 256 : nx <= 64 ? 64 : nx <= 128 ? 128 : 256;
    hipLaunchKernelGGL((sdf_last_axis_kernel<real, VOLUME, VOLUME ? VOX_MAX_DIM : SDF_MAX_DIM>), dim3((unsigned)(nz * ny)),
                       dim3(block), 0, stream, nx, cell, cell * (double)(VOLUME ? nx + ny + nz : nx + ny), (real*)sdf);
    return hipGetLastError();
}

// Both entry points: the argument check (`bad`: the entry point's own message), the launches, a HIP error under its name.
template <bool VOLUME>
static int sdf_build(const char* name, const char* bad, sgpmp_ctx* c, const void* occ, int nz, int ny, int nx, double cell,
                     double threshold, void* sdf, void* stream) {
    constexpr int max_dim = VOLUME ? VOX_MAX_DIM : SDF_MAX_DIM;
    if (!c || !occ || !sdf || occ == sdf || nz < 1 || ny < 1 || nx < 1 || nz > max_dim || ny > max_dim || nx > max_dim ||
        !(cell > 0.) || !(threshold == threshold))
        return sgpmp_set_error(SGPMP_EINVAL, bad);
    const hipError_t e = sgpmp_ctx_dtype(c) == SGPMP_F64
        ? launch_sdf_build<double, VOLUME>(occ, nz, ny, nx, cell, threshold, sdf, (hipStream_t)stream)
        : launch_sdf_build<float, VOLUME>(occ, nz, ny, nx, cell, threshold, sdf, (hipStream_t)stream);
    if (e != hipSuccess) {
        char msg[160];
        snprintf(msg, sizeof(msg), "%s: HIP error: %s", name, hipGetErrorString(e));
        return sgpmp_set_error(SGPMP_EHIP, msg);
    }
    return SGPMP_OK;
}

extern "C" int sgpmp_grid_sdf_build(sgpmp_ctx* c, const void* occ, int ny, int nx, double cell, double threshold, void* sdf,
                                    void* stream) {
    static_assert(SDF_MAX_DIM < SDF_NONE && SDF_NONE <= (1 << 24), "SDF_NONE: a run length, exact in fp32");
    static_assert((long long)SDF_NONE * SDF_NONE + (long long)(SDF_MAX_DIM - 1) * (SDF_MAX_DIM - 1) < (1ll << 31), "SDF_NONE^2: int");
    return sdf_build<false>("sgpmp_grid_sdf_build",
                            "sgpmp_grid_sdf_build: bad argument (distinct non-null occ and sdf, 1 <= ny, nx <= 4096, "
                            "cell > 0, a threshold that is not NaN)", c, occ, 1, ny, nx, cell, threshold, sdf, stream);
}

extern "C" int sgpmp_voxel_sdf_build(sgpmp_ctx* c, const void* occ, int nz, int ny, int nx, double cell, double threshold,
                                     void* sdf, void* stream) {
    static_assert((size_t)VOX_MAX_DIM * VOX_TILE_X * sizeof(int) <= 64 * 1024, "voxel_sdf_y_kernel: LDS tile");
    static_assert(3 * (VOX_MAX_DIM - 1) * (VOX_MAX_DIM - 1) < VOX_NONE && VOX_NONE <= (1 << 24), "VOX_NONE: exact in fp32");
    return sdf_build<true>("sgpmp_voxel_sdf_build",
                           "sgpmp_voxel_sdf_build: bad argument (distinct non-null occ and sdf, "
                           "1 <= nz, ny, nx <= 512, cell > 0, a threshold that is not NaN)", c, occ, nz, ny, nx, cell, threshold,
                           sdf, stream);
}

// ---------------------------------------------------------------------------------- value and gradient of the grid term
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
