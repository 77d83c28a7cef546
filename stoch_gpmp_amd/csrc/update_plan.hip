// The update launch (K4, update.hip) decided on the host: no kernel, no HIP call.  launch_update enqueues what plan_update says;
// tests/host_asan/update_table.cpp holds it to a table of shapes on the CPU.  The layout itself is sgpmp_internal.h's.
#include "sgpmp_internal.h"

// LDS of update_kernel without the regeneration: weights + indices (+ the new means for the tail when they fit)
static size_t update_tail_lds(int dtype, int n, int T, int S) { return upd_means_offset(S) + (size_t)T * 2 * n * (dtype == SGPMP_F64 ? 8 : 4); }
static size_t update_base_lds(int dtype, int n, int T, int S) {
    const size_t with_tail = update_tail_lds(dtype, n, T, S);
    return upd_lds_fits(with_tail) ? with_tail : upd_weights_bytes(S);
}

// Rows update_kernel can regenerate per round for this shape (4, 2, 1), or 0: a store-free step is not possible (the caller
// then stores the samples as always).  fp32, M a multiple of 4 (16-byte elements), T even (a Philox block is two waypoints).
// (weak, as update_ee_fold_fits: the host-side sanitizer harness links its stand-ins for the two beside this file)
__attribute__((weak)) int update_regen_rows(int dtype, int n, int T, int S, int recipe) {
    if (dtype != SGPMP_F32 || (T * 2 * n) % 4 != 0 || T % 2 != 0 || recipe < 1 || recipe > 2) return 0;
    const size_t base = upd_lds_round(update_base_lds(dtype, n, T, S));
    for (int R = 4; R >= 1; R >>= 1)
        if (upd_lds_fits(base + regen_lds_bytes(recipe, T, n, R))) return R;
    return 0;
}

// does update_kernel's scratch leave room for the folded end-effector term (S more doubles)?
__attribute__((weak)) bool update_ee_fold_fits(int dtype, int n, int T, int S) {
    return upd_lds_fits(upd_lds_round(update_base_lds(dtype, n, T, S)) + (size_t)S * sizeof(double));
}

// Which launches take update_kernel_quad: a function of (S, P), the scratch size and what the launch is asked for, never of
// timing.  It can run wherever nothing is regenerated, no end-effector term is folded in and four slices fit the workgroup's
// LDS (the switch update_wide < 0 takes it there: tests, A/B).  It is TAKEN where it measured faster
// (profiles/r12/update_quad_ab.txt and update_quad_rule_points.txt, same machine, alternating runs):
//  * only for a half of a two-chain step (RegenHost::beside_chain).  Alone on the GPU it is the longer kernel -- a lane owns
//    S / 64 costs and as many of the virtual waves' butterflies, one after the other: config 2 (planar 256 x 64 x 128, one
//    chain) lost 10 .. 13 %, config 1 (planar 4 x 16 x 64 fp64) 3 .. 8 %, single-iteration calls at the headline shape
//    (P = 1024, one chain) 1.0 .. 2.6 % with it.
//  * SGPMP_UPD_QUAD_MIN_P = 512 <= P < SGPMP_UPD_QUAD_END_P = 1024 particles per half.  Against update_kernel, Panda T = 64,
//    whole problem P x S: 1024 x 128 (the headline) +2.4 .. +3.2 %, 1024 x 64 +0.4 .. +3.2 %, 1024 x 256 +0.6 .. +1.6 %;
//    512 x 128 (halves of 256) level inside 2 % of noise, config 5's share (512 x 256, T = 128) -1.3 .. -3.5 %;
//    2048 x 128 (halves of 1024) -0.6, -0.9, +0.2 %.
//  * S <= SGPMP_UPD_QUAD_MAX_S = 256, where the measurements end (+0.6 .. +1.6 % at 1024 x 256: four costs per lane).
static bool update_quad_applies(int S, int P, size_t lds_one, bool regen, bool ee, bool beside_chain, int update_wide) {
    if (update_wide > 0 || regen || ee) return false;
    if (!upd_lds_fits(SGPMP_UPD_QUAD * upd_lds_round(lds_one))) return false;
    return update_wide < 0 || (beside_chain && S <= SGPMP_UPD_QUAD_MAX_S && P >= SGPMP_UPD_QUAD_MIN_P && P < SGPMP_UPD_QUAD_END_P);
}

UpdatePlan plan_update(const UpdateShape& shape, const UpdateWants& wants, int update_wide) {
    const int dtype = shape.dtype, n = shape.n, T = shape.T, S = shape.S, P = shape.P;
    UpdatePlan refused = {shape}, p = {shape, true};
    refused.kernel = p.kernel = "";
    // (the softmax coefficients of the partials reuse the index array as doubles: 8 bytes per group of 8 rows fit its 4 S)
    // + the new means for the tail.  Shapes whose weights fit the 64 KB of a workgroup but not together with
    // the means (e.g. S = 4096, T = 512, n = 7 in fp32: 77 KB) run WITHOUT the tail: the next step then
    // computes its importance-sampling weights with K5, as before the tail existed.
    p.tail = wants.isw_tail && upd_lds_fits(update_tail_lds(dtype, n, T, S));
    size_t lds = p.tail ? update_tail_lds(dtype, n, T, S) : upd_weights_bytes(S);
    if (P <= 0) return p;
    // store-free step: the rows with weight are regenerated behind the kernel's usual scratch (sized WITH the tail's means: without
    // them the offset is merely generous)
    if (wants.regen_recipe != 0) {
        p.regen_rows = dtype == SGPMP_F32 && wants.has_nnz ? update_regen_rows(dtype, n, T, S, wants.regen_recipe) : 0;
        if (p.regen_rows < 1) return refused;                    // (the caller asked update_regen_rows before the launch that skipped the stores)
        p.regen_off = (unsigned)upd_lds_round(update_base_lds(dtype, n, T, S));
        lds = p.regen_off + regen_lds_bytes(wants.regen_recipe, T, n, p.regen_rows);
    }
    // the step's end-effector goal term inside this kernel: S doubles behind everything else
    if (wants.ee_fold) {
        p.ee_off = (unsigned)upd_lds_round(lds);
        lds = p.ee_off + (size_t)S * sizeof(double);
        if (!upd_lds_fits(lds)) return refused;                  // (the caller checks update_ee_fold_fits first)
    }
    p.quad = (p.tail || !wants.isw_tail) && update_quad_applies(S, P, lds, wants.regen_recipe != 0, wants.ee_fold, wants.beside_chain, update_wide);
    p.slice = (unsigned)upd_lds_round(lds);
    p.grid = p.quad ? (unsigned)((P + SGPMP_UPD_QUAD - 1) / SGPMP_UPD_QUAD) : (unsigned)P;
    p.lds = p.quad ? SGPMP_UPD_QUAD * p.slice : (unsigned)lds;
    p.vw = (T * 2 * n) % 4 == 0 ? 4 : 2;
    p.kernel = p.quad ? "update_kernel_quad" : "update_kernel";
    return p;
}
