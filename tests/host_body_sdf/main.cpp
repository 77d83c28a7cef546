// Host driver for the device text of the body collision spheres (csrc/body_device.h, included as it stands under BODY_DEVICE_HOST)
// on the voxel field's device functions (csrc/cost_device.h: tests/test_cpu_body_sdf.py cuts their text out of the header into
// voxel_sdf_funcs.inc, as tests/host_voxel_sdf does).  Only the device qualifiers, RealOps, and the structs the text reads are
// restated here.  Built with -fsanitize=address,undefined -ffp-contract=off; reads one case from a text file (argv[1]):
//   dtype nz ny nx cell ox oy oz margin | the volume | nj, per joint R[9] t[3] revolute qidx | M, per sphere link cx cy cz r |
//   n B | B rows of q
// and prints per configuration: f, df/dq [n], min clearance, its gradient [n], f on the frames of a host-side walk.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <vector>
#define __device__
#define __forceinline__ inline
#define SGPMP_CONST
#define SGPMP_MAX_INTERP 8
#define SGPMP_MAX_JOINTS 16
#define BODY_DEVICE_HOST 1
using std::fmax;
using std::fmin;
template <typename real> struct RealOps {
    static real mul_rn(real a, real b) { return a * b; }
    static real add_rn(real a, real b) { return a + b; }
    static real floor_(real a) { return std::floor(a); }
    static void sincos_(real a, real* s, real* c) { *s = std::sin(a); *c = std::cos(a); }
};
template <typename real> struct TermK {
    int kind, flags; real K, K2, dt, c11, c12, c22, selfc, inv_cell, off_x, off_y; const void* dev_data; int dim0, dim1;
    long long rows_per_goal; int n_points, n_interp, interp_lo, interp_hi; real alpha[SGPMP_MAX_INTERP]; };
struct JointDev { double R[9]; double t[3]; int revolute; int qidx; };
struct ChainDev { int n_joints; int n_links; JointDev j[SGPMP_MAX_JOINTS]; };
typedef const ChainDev* ChainC;
template <typename real> struct JointK {
    static real R(ChainC ch, int j, int i) { return (real)ch->j[j].R[i]; }
    static real t(ChainC ch, int j, int i) { return (real)ch->j[j].t[i]; }
};

#include "voxel_sdf_funcs.inc"
#include "body_device.h"

template <typename real>
static bool same(real a, real b) { return a == b || (a != a && b != b); }

template <typename real>
static int go(FILE* in, int nz, int ny, int nx, double cell, const double* off, double margin) {
    std::vector<real> sdf((size_t)nz * ny * nx);               // (exactly nz x ny x nx: an index past it is a sanitizer report)
    for (auto& v : sdf) { double d; if (fscanf(in, "%lf", &d) != 1) return 2; v = (real)d; }
    TermK<real> tm = {};
    tm.K = 1; tm.K2 = (real)margin; tm.inv_cell = (real)(1. / cell);
    tm.off_x = (real)off[0]; tm.off_y = (real)off[1]; tm.dt = (real)off[2];
    tm.dev_data = sdf.data(); tm.dim0 = ny; tm.dim1 = nx; tm.rows_per_goal = nz;
    ChainDev ch = {};
    if (fscanf(in, "%d", &ch.n_joints) != 1 || ch.n_joints < 1 || ch.n_joints > SGPMP_MAX_JOINTS) return 2;
    ch.n_links = ch.n_joints + 1;
    for (int j = 0; j < ch.n_joints; ++j) {
        for (int i = 0; i < 9; ++i) if (fscanf(in, "%lf", &ch.j[j].R[i]) != 1) return 2;
        for (int i = 0; i < 3; ++i) if (fscanf(in, "%lf", &ch.j[j].t[i]) != 1) return 2;
        if (fscanf(in, "%d %d", &ch.j[j].revolute, &ch.j[j].qidx) != 2) return 2;
    }
    int M;
    if (fscanf(in, "%d", &M) != 1 || M < 1) return 2;
    std::vector<int> link(M);                                  // (exactly M entries: a read past the table is a sanitizer report)
    std::vector<real> sph((size_t)M * 4);
    for (int m = 0; m < M; ++m) {
        double v[4];
        if (fscanf(in, "%d %lf %lf %lf %lf", &link[m], &v[0], &v[1], &v[2], &v[3]) != 5) return 2;
        for (int k = 0; k < 4; ++k) sph[m * 4 + k] = (real)v[k];
    }
    BodyK<real> body = {link.data(), sph.data(), M};
    int n, B;
    if (fscanf(in, "%d %d", &n, &B) != 2 || n < 1 || n > SGPMP_MAX_JOINTS) return 2;
    for (int b = 0; b < B; ++b) {
        std::vector<real> q(n);
        for (auto& v : q) { double d; if (fscanf(in, "%lf", &d) != 1) return 2; v = (real)d; }
        real acc[SGPMP_MAX_JOINTS], accq[SGPMP_MAX_JOINTS];
        const real f = body_field<real, 0, BODY_GRAD>(&ch, tm, body, q.data(), acc);
        const real f0 = body_field<real, 0, BODY_VALUE>(&ch, tm, body, q.data(), nullptr);
        const real s = body_field<real, 0, BODY_QUERY>(&ch, tm, body, q.data(), accq);
        if (!same(f, f0)) return 3;                            // value with and without the gradient: the same bits
        if (ch.n_joints == 10) {                               // the compiled-in chain length against the generic form
            real a10[10], q10[10];
            if (!same(f, body_field<real, 10, BODY_GRAD>(&ch, tm, body, q.data(), a10))) return 4;
            if (!same(s, body_field<real, 10, BODY_QUERY>(&ch, tm, body, q.data(), q10))) return 4;
            for (int j = 0; j < 10; ++j) if (!same(a10[j], acc[j]) || !same(q10[j], accq[j])) return 4;
        }
        // the frames of the same walk, for body_field_frames
        std::vector<real> fr((size_t)ch.n_links * 16, (real)0);
        real R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0};
        for (int l = 0; l <= ch.n_joints; ++l) {
            for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) fr[l * 16 + r * 4 + c] = R[r * 3 + c]; fr[l * 16 + r * 4 + 3] = p[r]; }
            fr[l * 16 + 15] = 1;
            if (l == ch.n_joints) break;
            const JointDev& J = ch.j[l];
            real Rn[9];
            for (int r = 0; r < 3; ++r) p[r] += R[r * 3] * (real)J.t[0] + R[r * 3 + 1] * (real)J.t[1] + R[r * 3 + 2] * (real)J.t[2];
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c)
                    Rn[r * 3 + c] = R[r * 3] * (real)J.R[c] + R[r * 3 + 1] * (real)J.R[3 + c] + R[r * 3 + 2] * (real)J.R[6 + c];
            if (J.revolute) {
                const real sn = std::sin(q[J.qidx]), cs = std::cos(q[J.qidx]);
                for (int r = 0; r < 3; ++r) { const real aa = Rn[r * 3], bb = Rn[r * 3 + 1]; Rn[r * 3] = aa * cs + bb * sn; Rn[r * 3 + 1] = bb * cs - aa * sn; }
            }
            for (int i = 0; i < 9; ++i) R[i] = Rn[i];
        }
        const real ff = body_field_frames<real>(tm, body, fr.data());
        printf("%.17g", (double)f);
        for (int j = 0; j < ch.n_joints; ++j) if (ch.j[j].revolute) printf(" %.17g", (double)acc[j]);
        printf(" %.17g", (double)s);
        for (int j = 0; j < ch.n_joints; ++j) if (ch.j[j].revolute) printf(" %.17g", (double)accq[j]);
        printf(" %.17g\n", (double)ff);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 1;
    FILE* in = fopen(argv[1], "r");
    if (!in) return 1;
    int dtype, nz, ny, nx; double cell, off[3], margin;
    if (fscanf(in, "%d %d %d %d %lf %lf %lf %lf %lf", &dtype, &nz, &ny, &nx, &cell, &off[0], &off[1], &off[2], &margin) != 9) return 2;
    const int rc = dtype ? go<double>(in, nz, ny, nx, cell, off, margin) : go<float>(in, nz, ny, nx, cell, off, margin);
    fclose(in);
    return rc;
}
