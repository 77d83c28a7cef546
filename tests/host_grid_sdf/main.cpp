// Host driver for the signed-distance grid field's device functions (csrc/cost_device.h: grid_sdf_distance, grid_sdf_field):
// tests/test_cpu_grid_sdf.py cuts their text out of the header into grid_sdf_funcs.inc; only the device qualifiers and the two
// structs they read are restated here.  Built with -fsanitize=address,undefined -ffp-contract=off; reads one case from a text
// file (argv[1]: dtype ny nx cell ox oy margin npts, the grid, the points) and prints h, d, dh/dx, dh/dy per point.
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

#include "grid_sdf_funcs.inc"

template <typename real>
static int go(FILE* in, int ny, int nx, double cell, double ox, double oy, double margin, int npts) {
    std::vector<real> sdf((size_t)ny * nx);                    // (exactly ny x nx: an index past it is a sanitizer report)
    for (auto& v : sdf) { double d; if (fscanf(in, "%lf", &d) != 1) return 2; v = (real)d; }
    TermK<real> tm = {};
    tm.K = 1; tm.K2 = (real)margin; tm.inv_cell = (real)(1. / cell); tm.off_x = (real)ox; tm.off_y = (real)oy;
    tm.dev_data = sdf.data(); tm.dim0 = ny; tm.dim1 = nx;
    for (int p = 0; p < npts; ++p) {
        double x, y;
        if (fscanf(in, "%lf %lf", &x, &y) != 2) return 2;
        real gx = 0, gy = 0, dx = 0, dy = 0;
        const real h = grid_sdf_field<real, true>(tm, (real)x, (real)y, &gx, &gy);
        const real h0 = grid_sdf_field<real, false>(tm, (real)x, (real)y, nullptr, nullptr);
        const real d = grid_sdf_distance<real, true>(tm, (real)x, (real)y, &dx, &dy);
        if (!(h == h0 || (h != h && h0 != h0))) return 3;      // value with and without the gradient: the same bits
        printf("%.17g %.17g %.17g %.17g\n", (double)h, (double)d, (double)gx, (double)gy);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 1;
    FILE* in = fopen(argv[1], "r");
    if (!in) return 1;
    int dtype, ny, nx, npts; double cell, ox, oy, margin;
    if (fscanf(in, "%d %d %d %lf %lf %lf %lf %d", &dtype, &ny, &nx, &cell, &ox, &oy, &margin, &npts) != 8) return 2;
    const int rc = dtype ? go<double>(in, ny, nx, cell, ox, oy, margin, npts) : go<float>(in, ny, nx, cell, ox, oy, margin, npts);
    fclose(in);
    return rc;
}
