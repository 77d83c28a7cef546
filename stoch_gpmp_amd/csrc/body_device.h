// Device side of SGPMP_COST_BODY_SDF (include/sgpmp.h has the definition): the hinge of the voxel signed-distance field at the
// body's collision spheres.  One forward-kinematics walk that keeps the rotation -- twelve live values -- and evaluates a link's
// spheres as the walk passes the link: the table is link-ordered, so one cursor runs through it once.  The distance and the hinge
// are voxel_sdf_distance / voxel_sdf_field of cost_device.h, called unchanged: the per-sphere margin + r_m travels in a copy of
// the term's K2.  Included by body_sdf.hip, and by tests/host_body_sdf/main.cpp, which compiles this text for the host (it
// restates the qualifiers, the chain struct and RealOps, and defines BODY_DEVICE_HOST).
#pragma once
#ifndef BODY_DEVICE_HOST
#include "cost_device.h"
#endif

// The body table as the kernels read it: wave-uniform, so through the constant address space (scalar loads).
template <typename real>
struct BodyK {
    const int* link;              // [n] link index of sphere m, non-decreasing
    const real* sph;              // [n][4] centre in the link's frame, radius
    int n;
};

enum { BODY_VALUE = 0, BODY_GRAD = 1, BODY_QUERY = 2 };

// World centre of a sphere with centre c in the frame (R, p).
template <typename real>
__device__ __forceinline__ void body_point(const real* R, const real* p, real cx, real cy, real cz, real* w) {
#pragma unroll
    for (int r = 0; r < 3; ++r) w[r] = p[r] + (R[r * 3 + 0] * cx + R[r * 3 + 1] * cy + R[r * 3 + 2] * cz);
}

// The field of ONE configuration q (the lane's n joint values).
//   BODY_VALUE: -> f = sum_m h_m.
//   BODY_GRAD:  also acc[j] = df/dq of JOINT j (by joint index; fixed joints stay 0): the axes z_j and origins o_j of the joints
//               walked so far are kept, and every sphere adds z_j . ((p_m - o_j) x g_m) to the joints in front of its link.
//   BODY_QUERY: -> min_m (d(p_m) - r_m) and acc = the gradient through the first arg-min sphere (table order, strict comparison).
// A NaN distance anywhere makes the value and every acc[j] NaN.  NJ > 0: the chain length at compile time -- the walk unrolls and
// z, o, acc live in registers; NJ = 0: any chain (dynamically indexed arrays).
template <typename real, int NJ, int MODE>
__device__ __forceinline__ real body_field(ChainC ch, const TermK<real>& tm, const BodyK<real>& body, const real* q, real* acc) {
    using O = RealOps<real>;
    constexpr bool G = MODE != BODY_VALUE;
    constexpr int MJ = NJ > 0 ? NJ : SGPMP_MAX_JOINTS;
    const int nj = NJ > 0 ? NJ : ch->n_joints;
    const SGPMP_CONST int* lk = (const SGPMP_CONST int*)body.link;
    const SGPMP_CONST real* sp = (const SGPMP_CONST real*)body.sph;
    real Z[G ? MJ : 1][3], Oj[G ? MJ : 1][3];
    real R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0};
    real val = MODE == BODY_QUERY ? (real)__builtin_inff() : (real)0, bad = 0;
    if constexpr (G) {
#pragma unroll
        for (int j = 0; j < MJ; ++j) acc[j] = 0;
    }
    int m = 0;
#pragma unroll
    for (int l = 0; l <= nj; ++l) {
        while (m < body.n && lk[m] == l) {                 // the spheres of link l
            real w[3], g[3] = {0, 0, 0};
            body_point<real>(R, p, sp[m * 4 + 0], sp[m * 4 + 1], sp[m * 4 + 2], w);
            const real rad = sp[m * 4 + 3];
            ++m;
            if constexpr (MODE == BODY_QUERY) {
                const real s = voxel_sdf_distance<real, true>(tm, w[0], w[1], w[2], g) - rad;
                if (!(s == s)) bad = s;
                if (s < val) {
                    val = s;
#pragma unroll
                    for (int j = 0; j < MJ; ++j) {
                        real e = 0;
                        if (j < l) {
                            const real rx = w[0] - Oj[j][0], ry = w[1] - Oj[j][1], rz = w[2] - Oj[j][2];
                            e = Z[j][0] * (ry * g[2] - rz * g[1]) + Z[j][1] * (rz * g[0] - rx * g[2]) + Z[j][2] * (rx * g[1] - ry * g[0]);
                        }
                        acc[j] = e;
                    }
                }
            } else {
                TermK<real> ts = tm;
                ts.K2 = tm.K2 + rad;                        // the hinge on (margin + r_m) - d
                val += voxel_sdf_field<real, G>(ts, w[0], w[1], w[2], g);
                if constexpr (G) {
#pragma unroll
                    for (int j = 0; j < MJ; ++j)
                        if (j < l) {
                            const real rx = w[0] - Oj[j][0], ry = w[1] - Oj[j][1], rz = w[2] - Oj[j][2];
                            acc[j] += Z[j][0] * (ry * g[2] - rz * g[1]) + Z[j][1] * (rz * g[0] - rx * g[2]) + Z[j][2] * (rx * g[1] - ry * g[0]);
                        }
                }
            }
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
    if constexpr (MODE == BODY_QUERY) val = !(bad == bad) ? bad : val;
    if constexpr (G) {
        if (!(val == val)) {
#pragma unroll
            for (int j = 0; j < MJ; ++j) acc[j] = val;
        }
    }
    return val;
}

// The field on explicit link frames fr [n_links][4][4] (row-major): the frames carry the rotations.
template <typename real>
__device__ __forceinline__ real body_field_frames(const TermK<real>& tm, const BodyK<real>& body, const real* fr) {
    const SGPMP_CONST int* lk = (const SGPMP_CONST int*)body.link;
    const SGPMP_CONST real* sp = (const SGPMP_CONST real*)body.sph;
    real val = 0;
    for (int m = 0; m < body.n; ++m) {
        const real* f = fr + (size_t)lk[m] * 16;
        const real R[9] = {f[0], f[1], f[2], f[4], f[5], f[6], f[8], f[9], f[10]}, p[3] = {f[3], f[7], f[11]};
        real w[3];
        body_point<real>(R, p, sp[m * 4 + 0], sp[m * 4 + 1], sp[m * 4 + 2], w);
        TermK<real> ts = tm;
        ts.K2 = tm.K2 + sp[m * 4 + 3];
        val += voxel_sdf_field<real, false>(ts, w[0], w[1], w[2], nullptr);
    }
    return val;
}
