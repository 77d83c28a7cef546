// Host driver for the voxel signed-distance field's device functions (csrc/cost_device.h: voxel_sdf_distance, voxel_sdf_field):
// tests/test_cpu_voxel_sdf.py cuts their text out of the header into voxel_sdf_funcs.inc; only the device qualifiers and the
// struct they read are restated here.  Built with -fsanitize=address,undefined -ffp-contract=off; reads one case from a text file
// (argv[1]: dtype nz ny nx cell ox oy oz margin npts, the volume, the points) and prints h, d, dh/dx, dh/dy, dh/dz per point.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <vector>
#define __device__
#define __forceinline__ inline
#define SGPMP_MAX_INTERP 8
using std::fmax;
using std::fmin;
template <typename real> struct RealOps {
    static real mul_rn(real a, real b) { return a * b; }
    static real add_rn(real a, real b) { return a + b; }
    static real floor_(real a) { return std::floor(a); }
};
template <typename real> struct TermK {
    int kind, flags; real K, K2, dt, c11, c12, c22, selfc, inv_cell, off_x, off_y; const void* dev_data; int dim0, dim1;
    long long rows_per_goal; int n_points, n_interp, interp_lo, interp_hi; real alpha[SGPMP_MAX_INTERP]; };

#include "voxel_sdf_funcs.inc"

template <typename real>
static int go(FILE* in, int nz, int ny, int nx, double cell, const double* off, double margin, int npts) {
    std::vector<real> sdf((size_t)nz * ny * nx);               // (exactly nz x ny x nx: an index past it is a sanitizer report)
    for (auto& v : sdf) { double d; if (fscanf(in, "%lf", &d) != 1) return 2; v = (real)d; }
    TermK<real> tm = {};
    tm.K = 1; tm.K2 = (real)margin; tm.inv_cell = (real)(1. / cell);
    tm.off_x = (real)off[0]; tm.off_y = (real)off[1]; tm.dt = (real)off[2];
    tm.dev_data = sdf.data(); tm.dim0 = ny; tm.dim1 = nx; tm.rows_per_goal = nz;
    for (int p = 0; p < npts; ++p) {
        double x, y, z;
        if (fscanf(in, "%lf %lf %lf", &x, &y, &z) != 3) return 2;
        real g[3] = {0, 0, 0}, dd[3] = {0, 0, 0};
        const real h = voxel_sdf_field<real, true>(tm, (real)x, (real)y, (real)z, g);
        const real h0 = voxel_sdf_field<real, false>(tm, (real)x, (real)y, (real)z, nullptr);
        const real d = voxel_sdf_distance<real, true>(tm, (real)x, (real)y, (real)z, dd);
        if (!(h == h0 || (h != h && h0 != h0))) return 3;      // value with and without the gradient: the same bits
        printf("%.17g %.17g %.17g %.17g %.17g\n", (double)h, (double)d, (double)g[0], (double)g[1], (double)g[2]);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 1;
    FILE* in = fopen(argv[1], "r");
    if (!in) return 1;
    int dtype, nz, ny, nx, npts; double cell, off[3], margin;
    if (fscanf(in, "%d %d %d %d %lf %lf %lf %lf %lf %d", &dtype, &nz, &ny, &nx, &cell, &off[0], &off[1], &off[2], &margin, &npts) != 10)
        return 2;
    const int rc = dtype ? go<double>(in, nz, ny, nx, cell, off, margin, npts) : go<float>(in, nz, ny, nx, cell, off, margin, npts);
    fclose(in);
    return rc;
}
