// Host driver for the device text of the body's self-collision term (csrc/body_self_device.h, included as it stands under
// BODY_SELF_DEVICE_HOST).  Only the device qualifiers, RealOps and the chain struct are restated here; the centre image, LDS on the
// device, is a plain array of exactly 3 * M * SGPMP_WAVE elements, of which the program uses column 0 (a lane's column), so an
// index past the image is a sanitizer report.  Built with -fsanitize=address,undefined -ffp-contract=off; reads one case from a
// text file (argv[1]):
//   dtype margin | nj, per joint R[9] t[3] revolute qidx | M, per sphere link cx cy cz r | M pair rows (decimal uint64) | n B |
//   B rows of q
// and prints per configuration: f, df/dq [n], min clearance, its gradient [n], f on the frames of a host-side walk.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <vector>
#define __device__
#define __forceinline__ inline
#define SGPMP_CONST
#define SGPMP_MAX_JOINTS 16
#define SGPMP_WAVE 64
#define BODY_SELF_DEVICE_HOST 1
template <typename real> struct RealOps {
    static real sqrt_(real a) { return std::sqrt(a); }
    static void sincos_(real a, real* s, real* c) { *s = std::sin(a); *c = std::cos(a); }
};
struct JointDev { double R[9]; double t[3]; int revolute; int qidx; };
struct ChainDev { int n_joints; int n_links; JointDev j[SGPMP_MAX_JOINTS]; };
typedef const ChainDev* ChainC;
template <typename real> struct JointK {
    static real R(ChainC ch, int j, int i) { return (real)ch->j[j].R[i]; }
    static real t(ChainC ch, int j, int i) { return (real)ch->j[j].t[i]; }
};

#include "body_self_device.h"

template <typename real>
static bool same(real a, real b) { return a == b || (a != a && b != b); }

// A compiled-in chain length (body_self.hip has 10 and 7) against the generic form: the same bits.
template <typename real, int NJ>
static bool fixed_matches(const ChainDev& ch, const BodySelfK<real>& body, real margin, const real* q, real* cen, real f, real s,
                          const real* acc, const real* accq) {
    real Z[NJ][3], O[NJ][3], a[NJ], aq[NJ];
    body_self_walk<real, NJ, true>(&ch, body, q, cen, Z, O);
    if (!same(f, body_self_pairs<real, NJ, BSELF_GRAD>(body, margin, cen, Z, O, a))) return false;
    if (!same(s, body_self_pairs<real, NJ, BSELF_QUERY>(body, margin, cen, Z, O, aq))) return false;
    for (int j = 0; j < NJ; ++j) if (!same(a[j], acc[j]) || !same(aq[j], accq[j])) return false;
    return true;
}

template <typename real>
static int go(FILE* in, double margin_d) {
    const real margin = (real)margin_d;
    ChainDev ch = {};
    if (fscanf(in, "%d", &ch.n_joints) != 1 || ch.n_joints < 1 || ch.n_joints > SGPMP_MAX_JOINTS) return 2;
    ch.n_links = ch.n_joints + 1;
    for (int j = 0; j < ch.n_joints; ++j) {
        for (int i = 0; i < 9; ++i) if (fscanf(in, "%lf", &ch.j[j].R[i]) != 1) return 2;
        for (int i = 0; i < 3; ++i) if (fscanf(in, "%lf", &ch.j[j].t[i]) != 1) return 2;
        if (fscanf(in, "%d %d", &ch.j[j].revolute, &ch.j[j].qidx) != 2) return 2;
    }
    int M;
    if (fscanf(in, "%d", &M) != 1 || M < 2 || M > 64) return 2;
    std::vector<int> link(M);                                  // (exactly M entries: a read past a table is a sanitizer report)
    std::vector<real> sph((size_t)M * 4);
    std::vector<unsigned long long> rows(M);
    for (int m = 0; m < M; ++m) {
        double v[4];
        if (fscanf(in, "%d %lf %lf %lf %lf", &link[m], &v[0], &v[1], &v[2], &v[3]) != 5) return 2;
        for (int k = 0; k < 4; ++k) sph[m * 4 + k] = (real)v[k];
    }
    for (int m = 0; m < M; ++m) if (fscanf(in, "%llu", &rows[m]) != 1) return 2;
    BodySelfK<real> body = {link.data(), sph.data(), rows.data(), M};
    std::vector<real> cen((size_t)3 * M * SGPMP_WAVE), cen2((size_t)3 * M * SGPMP_WAVE);
    int n, B;
    if (fscanf(in, "%d %d", &n, &B) != 2 || n < 1 || n > SGPMP_MAX_JOINTS) return 2;
    for (int b = 0; b < B; ++b) {
        std::vector<real> q(n);
        for (auto& v : q) { double d; if (fscanf(in, "%lf", &d) != 1) return 2; v = (real)d; }
        real Z[SGPMP_MAX_JOINTS][3], Oj[SGPMP_MAX_JOINTS][3], acc[SGPMP_MAX_JOINTS], accq[SGPMP_MAX_JOINTS];
        body_self_walk<real, 0, true>(&ch, body, q.data(), cen.data(), Z, Oj);
        const real f = body_self_pairs<real, 0, BSELF_GRAD>(body, margin, cen.data(), Z, Oj, acc);
        const real s = body_self_pairs<real, 0, BSELF_QUERY>(body, margin, cen.data(), Z, Oj, accq);
        body_self_walk<real, 0, false>(&ch, body, q.data(), cen2.data(), nullptr, nullptr);
        const real f0 = body_self_pairs<real, 0, BSELF_VALUE>(body, margin, cen2.data(), nullptr, nullptr, nullptr);
        if (!same(f, f0)) return 3;                            // value with and without the gradient: the same bits
        if (ch.n_joints == 10 && !fixed_matches<real, 10>(ch, body, margin, q.data(), cen2.data(), f, s, acc, accq)) return 4;
        if (ch.n_joints == 7 && !fixed_matches<real, 7>(ch, body, margin, q.data(), cen2.data(), f, s, acc, accq)) return 4;
        // the frames of the same walk, for body_self_frames
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
        body_self_frames<real>(body, fr.data(), cen2.data());
        const real ff = body_self_pairs<real, 0, BSELF_VALUE>(body, margin, cen2.data(), nullptr, nullptr, nullptr);
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
    int dtype; double margin;
    if (fscanf(in, "%d %lf", &dtype, &margin) != 2) return 2;
    const int rc = dtype ? go<double>(in, margin) : go<float>(in, margin);
    fclose(in);
    return rc;
}
