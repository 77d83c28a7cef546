// Device side of SGPMP_COST_BODY_SELF (include/sgpmp.h has the definition): the hinge on the clearance between the body's own
// collision spheres, over the counted pairs.  A lane is one configuration.  Two phases:
//   1. the forward-kinematics walk of body_device.h (it keeps the rotation), which writes the world centre of every sphere into
//      the lane's column of a centre image cen[m][3][SGPMP_WAVE] -- LDS on the device: all M centres are needed at once, up to
//      192 values, too many to index dynamically in registers; the image is lane-contiguous, so every access is conflict-free,
//      and a lane reads back only what it wrote itself (no barrier);
//   2. the pair loop over the set bits j > i of the mask rows -- wave-uniform, the table is read through the constant address
//      space -- which reads two triples from the image per pair.
// Included by body_self.hip, and by tests/host_body_self/main.cpp, which compiles this text for the host (it restates the
// qualifiers, the chain struct and RealOps, gives the image as a plain array, and defines BODY_SELF_DEVICE_HOST).
#pragma once
#ifndef BODY_SELF_DEVICE_HOST
#include "cost_device.h"
#endif

// The body table and the pair rows as the kernels read them: wave-uniform (scalar loads).
template <typename real>
struct BodySelfK {
    const int* link;                    // [n] link index of sphere m, non-decreasing
    const real* sph;                    // [n][4] centre in the link's frame, radius
    const unsigned long long* rows;     // [n] bit j of rows[i]: pair (i, j) is counted; only bits j > i are read
    int n;
};

enum { BSELF_VALUE = 0, BSELF_GRAD = 1, BSELF_QUERY = 2 };

// Phase 1 from joint values q (the lane's n): centres into cen (the lane's column: element (m, r) at cen[(m * 3 + r) * SGPMP_WAVE]).
// G: also the axis Z[j] and origin Oj[j] of every joint, in the world.  NJ > 0: the chain length at compile time -- the walk
// unrolls and Z, Oj live in registers; NJ = 0: any chain (dynamically indexed arrays).
template <typename real, int NJ, bool G>
__device__ __forceinline__ void body_self_walk(ChainC ch, const BodySelfK<real>& body, const real* q, real* cen, real (*Z)[3],
                                               real (*Oj)[3]) {
    using O = RealOps<real>;
    const int nj = NJ > 0 ? NJ : ch->n_joints;
    const SGPMP_CONST int* lk = (const SGPMP_CONST int*)body.link;
    const SGPMP_CONST real* sp = (const SGPMP_CONST real*)body.sph;
    real R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0};
    int m = 0;
#pragma unroll
    for (int l = 0; l <= nj; ++l) {
        while (m < body.n && lk[m] == l) {                 // the spheres of link l
            const real cx = sp[m * 4 + 0], cy = sp[m * 4 + 1], cz = sp[m * 4 + 2];
#pragma unroll
            for (int r = 0; r < 3; ++r)
                cen[(m * 3 + r) * SGPMP_WAVE] = p[r] + (R[r * 3 + 0] * cx + R[r * 3 + 1] * cy + R[r * 3 + 2] * cz);
            ++m;
        }
        if (l == nj) break;
        // through joint l: Trans(xyz) RPY, then Rz(q) for a revolute joint
        real F[9], tt[3], Rn[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) F[i] = JointK<real>::R(ch, l, i);
#pragma unroll
        for (int i = 0; i < 3; ++i) tt[i] = JointK<real>::t(ch, l, i);
#pragma unroll
        for (int r = 0; r < 3; ++r) p[r] += R[r * 3 + 0] * tt[0] + R[r * 3 + 1] * tt[1] + R[r * 3 + 2] * tt[2];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                Rn[r * 3 + c] = R[r * 3 + 0] * F[c] + R[r * 3 + 1] * F[3 + c] + R[r * 3 + 2] * F[6 + c];
        if constexpr (G) {
#pragma unroll
            for (int r = 0; r < 3; ++r) { Z[l][r] = Rn[r * 3 + 2]; Oj[l][r] = p[r]; }       // joint axis and origin
        }
        if (ch->j[l].revolute) {
            real sn, cs;
            O::sincos_(q[ch->j[l].qidx], &sn, &cs);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const real aa = Rn[r * 3 + 0], bb = Rn[r * 3 + 1];
                Rn[r * 3 + 0] = aa * cs + bb * sn;
                Rn[r * 3 + 1] = bb * cs - aa * sn;
            }
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = Rn[i];
    }
}

// Phase 1 from explicit link frames fr [n_links][4][4] (row-major): the frames carry the rotations.
template <typename real>
__device__ __forceinline__ void body_self_frames(const BodySelfK<real>& body, const real* fr, real* cen) {
    const SGPMP_CONST int* lk = (const SGPMP_CONST int*)body.link;
    const SGPMP_CONST real* sp = (const SGPMP_CONST real*)body.sph;
    for (int m = 0; m < body.n; ++m) {
        const real* f = fr + (size_t)lk[m] * 16;
        const real cx = sp[m * 4 + 0], cy = sp[m * 4 + 1], cz = sp[m * 4 + 2];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            cen[(m * 3 + r) * SGPMP_WAVE] = f[r * 4 + 3] + (f[r * 4 + 0] * cx + f[r * 4 + 1] * cy + f[r * 4 + 2] * cz);
    }
}

// z . ((w - o) x g)
template <typename real>
__device__ __forceinline__ real body_self_torque(const real* z, const real* o, const real* w, const real* g) {
    const real rx = w[0] - o[0], ry = w[1] - o[1], rz = w[2] - o[2];
    return z[0] * (ry * g[2] - rz * g[1]) + z[1] * (rz * g[0] - rx * g[2]) + z[2] * (rx * g[1] - ry * g[0]);
}

// Phase 2: the counted pairs (i, j), i < j, i ascending then j ascending.
//   BSELF_VALUE: -> f = sum h_ij,  h_ij = (margin + r_i + r_j) - D_ij where that is > 0.
//   BSELF_GRAD:  also acc[k] = df/dq of JOINT k (by joint index; fixed joints carry a value nobody reads).  The force on sphere j is
//                g = (p_i - p_j) / D, the force on sphere i its negative; for a joint in front of both links the two torques cancel
//                (g is parallel to p_i - p_j), so a pair adds z_k . ((p_j - o_k) x g) to the joints link_i <= k < link_j only.
//                Exactly 0 where h = 0 and where D = 0 (no division).
//   BSELF_QUERY: -> min over the pairs of s_ij = D_ij - r_i - r_j, acc = the gradient through the first arg-min pair (strict comparison).
// A non-finite coordinate of a counted sphere makes the value and every acc[k] NaN.
template <typename real, int NJ, int MODE>
__device__ __forceinline__ real body_self_pairs(const BodySelfK<real>& body, real margin, const real* cen, const real (*Z)[3],
                                                const real (*Oj)[3], real* acc) {
    using O = RealOps<real>;
    constexpr bool G = MODE != BSELF_VALUE;
    constexpr int MJ = NJ > 0 ? NJ : SGPMP_MAX_JOINTS;
    const SGPMP_CONST int* lk = (const SGPMP_CONST int*)body.link;
    const SGPMP_CONST real* sp = (const SGPMP_CONST real*)body.sph;
    const SGPMP_CONST unsigned long long* rw = (const SGPMP_CONST unsigned long long*)body.rows;
    real val = MODE == BSELF_QUERY ? (real)__builtin_inff() : (real)0, bad = 0;
    if constexpr (G) {
#pragma unroll
        for (int k = 0; k < MJ; ++k) acc[k] = 0;
    }
    for (int i = 0; i < body.n; ++i) {
        unsigned long long row = rw[i] & ~((2ULL << i) - 1ULL);          // bits j > i (i = 63: none)
        if (!row) continue;
        const real pi[3] = {cen[(i * 3 + 0) * SGPMP_WAVE], cen[(i * 3 + 1) * SGPMP_WAVE], cen[(i * 3 + 2) * SGPMP_WAVE]};
        const real ri = sp[i * 4 + 3];
        const int li = lk[i];
        while (row) {
            const int j = __builtin_ctzll(row);
            row &= row - 1ULL;
            if (j >= body.n) break;                                      // (sgpmp_set_body_pairs has refused such a bit)
            const real pj[3] = {cen[(j * 3 + 0) * SGPMP_WAVE], cen[(j * 3 + 1) * SGPMP_WAVE], cen[(j * 3 + 2) * SGPMP_WAVE]};
            const real rj = sp[j * 4 + 3];
            const int lj = lk[j];
            const real d[3] = {pi[0] - pj[0], pi[1] - pj[1], pi[2] - pj[2]};
            const real D = O::sqrt_(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            const real chk = D - D;                                      // NaN for a NaN or infinite distance
            if (!(chk == 0)) bad = chk;
            if constexpr (MODE == BSELF_QUERY) {
                const real s = D - ri - rj;
                if (s < val) {
                    val = s;
                    const real inv = D > 0 ? (real)-1 / D : (real)0;     // ds/dp_j = -(p_i - p_j) / D
                    const real g[3] = {d[0] * inv, d[1] * inv, d[2] * inv};
#pragma unroll
                    for (int k = 0; k < MJ; ++k)
                        acc[k] = (k >= li && k < lj) ? body_self_torque<real>(Z[k], Oj[k], pj, g) : (real)0;
                }
            } else {
                const real e = (margin + ri + rj) - D;
                if (e > 0) {
                    val += e;
                    if constexpr (G) {
                        if (D > 0) {
                            const real inv = (real)1 / D;                // dh/dp_j = (p_i - p_j) / D
                            const real g[3] = {d[0] * inv, d[1] * inv, d[2] * inv};
#pragma unroll
                            for (int k = 0; k < MJ; ++k)
                                if (k >= li && k < lj) acc[k] += body_self_torque<real>(Z[k], Oj[k], pj, g);
                        }
                    }
                }
            }
        }
    }
    if (!(bad == bad)) val = bad;
    if constexpr (G) {
        if (!(val == val)) {
#pragma unroll
            for (int k = 0; k < MJ; ++k) acc[k] = val;
        }
    }
    return val;
}
