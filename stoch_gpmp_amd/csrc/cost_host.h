// Host side of cost_device.h's kernel-argument structs, shared by the translation units that launch field code
// (cost_sweep.hip, traj_dense.hip).  Not part of the run-time compiler's sources: hiprtc sees device code only.
#pragma once
#include "cost_device.h"

template <typename real>
static inline TermK<real> make_termk(const CostTerm& s) {
    TermK<real> k;
    k.kind = s.kind; k.flags = s.flags;
    k.K = (real)s.K; k.K2 = (real)s.K2; k.dt = (real)s.dt;
    k.c11 = (real)s.c11; k.c12 = (real)s.c12; k.c22 = (real)s.c22; k.selfc = (real)s.selfc;
    k.inv_cell = (real)s.inv_cell; k.off_x = (real)s.off_x; k.off_y = (real)s.off_y;
    k.dev_data = s.dev_data; k.dim0 = s.dim0; k.dim1 = s.dim1; k.rows_per_goal = s.rows_per_goal;
    k.n_points = s.n_points; k.n_interp = s.n_interp; k.interp_lo = s.interp_lo; k.interp_hi = s.interp_hi;
    for (int a = 0; a < SGPMP_MAX_INTERP; ++a) k.alpha[a] = (real)s.alpha[a];
    return k;
}
