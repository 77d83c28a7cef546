// Host side of cost_device.h's kernel-argument structs, shared by the translation units that launch field code
// (cost_sweep.hip, traj_dense.hip) or decide on such launches (step_plan.hip).  Not part of the run-time compiler's sources: hiprtc sees device code only.
#pragma once
#include <cstring>

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

// the program as named fields (FlatProg); false: a term of an unknown kind, or two of one kind
template <typename real>
static inline bool make_flat(const CostProgram& p, FlatProg<real>& f) {
    std::memset(&f, 0, sizeof(f));
    for (int i = 0; i < p.n_terms; ++i) {
        const TermK<real> k = make_termk<real>(p.terms[i]);
        int* has = nullptr;
        TermK<real>* slot = nullptr;
        switch (k.kind) {
            case SGPMP_COST_GP: has = &f.has_gp; slot = &f.gp; break;
            case SGPMP_COST_GOAL_PRIOR: has = &f.has_goal; slot = &f.goal; break;
            case SGPMP_COST_GRID: has = &f.has_grid; slot = &f.grid; break;
            case SGPMP_COST_SELF: has = &f.has_self; slot = &f.self; break;
            case SGPMP_COST_SPHERES: has = &f.has_sph; slot = &f.sph; f.sph_index = i; break;
            case SGPMP_COST_EE_GOAL: continue;      // evaluated by ee_goal_kernel after the sweep
            default: return false;
        }
        if (*has) return false;                      // a second term of this kind: not flat
        *has = 1;
        *slot = k;
    }
    return true;
}
