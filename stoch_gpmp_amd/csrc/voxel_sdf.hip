// Voxel signed-distance field (SGPMP_COST_VOXEL_SDF; include/sgpmp.h has the definition): the exact Euclidean distance transform
// of an occupancy volume on the device.  The field function itself is voxel_sdf_field in cost_device.h; the sweep, field_eval_kernel
// and field_grad_kernel (cost_sweep.hip) call it -- this file holds the transform alone.
#include <cstdio>

#include "sgpmp_internal.h"

// ---------------------------------------------------------------------------------- the transform
// Separable and exact (integers until the one square root), in place in the output volume, grid_sdf.hip's scheme one dimension up.
// A cell is either occupied or free, so of its two distances -- to the nearest occupied and to the nearest free cell -- one is
// zero: every pass leaves ONE signed number per cell, + the squared distance in cells to the nearest occupied cell seen so far
// for a free cell, - the squared distance to the nearest free one for an occupied cell (never zero: the sign IS the occupancy),
// VOX_NONE where there is none, as a value of the context's type (integers up to 2^20 are exact in fp32; a squared distance
// is at most 3 * 511^2 = 783 363).  No scratch volume, no allocation.
#define VOX_NONE (1 << 20)
#define VOX_MAX_DIM 512
#define VOX_TILE_X 32                  // y pass: x columns per workgroup; the [ny][32] int tile is <= 64 KiB of LDS
#define VOX_TILE_Y 8                   // y pass: 256 threads = 32 columns x 8 row groups, a thread takes rows yg, yg + 8, ...

// Pass z: one thread per (y, x) column, consecutive lanes on consecutive cells of a z slice; up the column and back down.
template <typename real>
__global__ void __launch_bounds__(256)
voxel_sdf_z_kernel(const real* __restrict__ occ, int nz, int plane, double threshold, real* __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;       // y * nx + x
    if (c >= plane) return;
    int to_occ = VOX_NONE, to_free = VOX_NONE;                 // slices since the last occupied / free cell (VOX_NONE: none yet)
    for (int z = 0; z < nz; ++z) {
        const size_t at = (size_t)z * plane + c;
        const bool o = (double)occ[at] > threshold;
        to_occ = o ? 0 : (to_occ < VOX_NONE ? to_occ + 1 : VOX_NONE);
        to_free = o ? (to_free < VOX_NONE ? to_free + 1 : VOX_NONE) : 0;
        out[at] = o ? (real)-to_free : (real)to_occ;           // (a distance in cells, squared by the way back)
    }
    to_occ = VOX_NONE; to_free = VOX_NONE;
    for (int z = nz - 1; z >= 0; --z) {
        const size_t at = (size_t)z * plane + c;
        const real up = out[at];
        const bool o = up < (real)0;
        to_occ = o ? 0 : (to_occ < VOX_NONE ? to_occ + 1 : VOX_NONE);
        to_free = o ? (to_free < VOX_NONE ? to_free + 1 : VOX_NONE) : 0;
        const int d = (int)(o ? -up : up), back = o ? to_free : to_occ;
        const int m = back < d ? back : d;
        const int sq = m < VOX_NONE ? m * m : VOX_NONE;
        out[at] = o ? (real)-sq : (real)sq;
    }
}

// Pass y: one workgroup per (z, 32 x columns); the [ny][32] signed tile is staged in LDS before any of it is overwritten, and no
// other workgroup touches it.  Lanes along x: the global accesses are 128-byte runs, the LDS reads of a wave 32 consecutive words
// (its two row groups read the same words: a broadcast).  Per cell the minimum over y' of (y - y')^2 + g(y').
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

// Pass x: one workgroup per row, the row staged in LDS (every lane reads the same word per step: a broadcast), then the one
// square root.
template <typename real>
__global__ void __launch_bounds__(256)
voxel_sdf_x_kernel(int nx, double cell, double cap, real* __restrict__ sdf) {
    __shared__ int g_row[VOX_MAX_DIM];
    real* row = sdf + (size_t)blockIdx.x * nx;
    for (int x = threadIdx.x; x < nx; x += blockDim.x) g_row[x] = (int)row[x];
    __syncthreads();
    for (int x = threadIdx.x; x < nx; x += blockDim.x) {
        const bool o = g_row[x] < 0;
        int best = VOX_NONE;
        for (int xp = 0; xp < nx; ++xp) {
            const int v = g_row[xp];
            const int g = o ? (v < 0 ? -v : 0) : (v > 0 ? v : 0);
            const int dx = x - xp;
            const int c = dx * dx + g;
            best = c < best ? c : best;
        }
        const double s = best >= VOX_NONE ? cap : (__dsqrt_rn((double)best) - 0.5) * cell;
        row[x] = (real)(o ? -s : s);
    }
}

template <typename real>
static hipError_t launch_voxel_sdf_build(const void* occ, int nz, int ny, int nx, double cell, double threshold, void* sdf,
                                         hipStream_t stream) {
    const int plane = ny * nx;
    hipLaunchKernelGGL((voxel_sdf_z_kernel<real>), dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, stream, (const real*)occ,
                       nz, plane, threshold, (real*)sdf);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((voxel_sdf_y_kernel<real>), dim3((unsigned)((nx + VOX_TILE_X - 1) / VOX_TILE_X), (unsigned)nz),
                       dim3(VOX_TILE_X * VOX_TILE_Y), (size_t)ny * VOX_TILE_X * sizeof(int), stream, ny, nx, (real*)sdf);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int block = nx <= 64 ? 64 : nx <= 128 ? 128 : 256;
    hipLaunchKernelGGL((voxel_sdf_x_kernel<real>), dim3((unsigned)(nz * ny)), dim3(block), 0, stream, nx, cell,
                       cell * (double)(nx + ny + nz), (real*)sdf);
    return hipGetLastError();
}

extern "C" int sgpmp_voxel_sdf_build(sgpmp_ctx* c, const void* occ, int nz, int ny, int nx, double cell, double threshold,
                                     void* sdf, void* stream) {
    static_assert((size_t)VOX_MAX_DIM * VOX_TILE_X * sizeof(int) <= 64 * 1024, "voxel_sdf_y_kernel: LDS tile");
    static_assert(3 * (VOX_MAX_DIM - 1) * (VOX_MAX_DIM - 1) < VOX_NONE && VOX_NONE <= (1 << 24), "VOX_NONE: exact in fp32");
    if (!c || !occ || !sdf || occ == sdf || nz < 1 || ny < 1 || nx < 1 || nz > VOX_MAX_DIM || ny > VOX_MAX_DIM || nx > VOX_MAX_DIM ||
        !(cell > 0.) || !(threshold == threshold))
        return sgpmp_set_error(SGPMP_EINVAL, "sgpmp_voxel_sdf_build: bad argument (distinct non-null occ and sdf, "
                                             "1 <= nz, ny, nx <= 512, cell > 0, a threshold that is not NaN)");
    const hipError_t e = sgpmp_ctx_dtype(c) == SGPMP_F64
        ? launch_voxel_sdf_build<double>(occ, nz, ny, nx, cell, threshold, sdf, (hipStream_t)stream)
        : launch_voxel_sdf_build<float>(occ, nz, ny, nx, cell, threshold, sdf, (hipStream_t)stream);
    if (e != hipSuccess) {
        char msg[160];
        snprintf(msg, sizeof(msg), "sgpmp_voxel_sdf_build: HIP error: %s", hipGetErrorString(e));
        return sgpmp_set_error(SGPMP_EHIP, msg);
    }
    return SGPMP_OK;
}
