// The update launch's ONE decision (csrc/update_plan.hip: plan_update, the real object) and the two questions plan_step asks of
// the same layout (update_regen_rows for recipes 1 and 2, update_ee_fold_fits) held to a table of shapes on the CPU, under
// AddressSanitizer + UBSan.  update_table_rows.inc: shape, wants, the update_wide switch, and what is expected.
// The rows were recorded once from launch_update as it was at the commit before plan_update (its values printed in front of the
// launch): BASELINE configs 1-5, the reference's example sizes and the shapes of plan_table_rows.inc, fp32 with fp32 and fp64
// costs and fp64; the tail kept and dropped; every boundary of the rows per regeneration round; the refusals; the folded
// end-effector term at its last and first sample counts; the one-wave-per-particle rule at its edges; two elements per
// thread; no particles.  A refused row (ok = 0) expects nothing else of the plan.
// Beyond the rows: no two regions of a particle's scratch overlap, and every region ends inside the launch's dynamic LDS.
// Exit code 0 and UPDATE_TABLE_OK = pass.  TEST INFRASTRUCTURE (tests/test_cpu_host.py).
#include <cstdio>
#include <cstring>

#include "sgpmp_internal.h"

struct UpdateRow {
    UpdateShape shape; UpdateWants wants; int update_wide;
    int ok, tail, regen_rows, regen_off, ee_off, slice, lds, quad, grid, vw;
    int regen_rows1, regen_rows2, ee_fits;
};
static const UpdateRow kRows[] = {
#include "update_table_rows.inc"
};

// the regions of one particle's scratch in the order of the layout: each begins where the one before ends or later, on 16 bytes
static bool regions_ok(const UpdatePlan& p, const UpdateWants& w) {
    const UpdateShape& s = p.shape;
    const size_t M = (size_t)s.T * 2 * s.n, one = p.quad ? p.slice : p.lds;
    size_t end = upd_weights_bytes(s.S);
    bool ok = true;
    auto region = [&](size_t off, size_t bytes) { ok = ok && off >= end && off % 16 == 0; end = off + bytes; };
    if (p.tail) region(upd_means_offset(s.S), M * (s.dtype == SGPMP_F64 ? 8 : 4));
    if (w.regen_recipe) region(p.regen_off, regen_lds_bytes(w.regen_recipe, s.T, s.n, p.regen_rows));
    if (w.ee_fold) region(p.ee_off, (size_t)s.S * 8);
    return ok && end <= one && (p.quad ? p.lds == SGPMP_UPD_QUAD * p.slice : p.slice == upd_lds_round(p.lds));
}

int main() {
    int bad = 0, n = 0;
    for (const UpdateRow& r : kRows) {
        const UpdatePlan p = plan_update(r.shape, r.wants, r.update_wide);
        const int asked[] = {update_regen_rows(r.shape.dtype, r.shape.n, r.shape.T, r.shape.S, 1), update_regen_rows(r.shape.dtype, r.shape.n, r.shape.T, r.shape.S, 2),
                             (int)update_ee_fold_fits(r.shape.dtype, r.shape.n, r.shape.T, r.shape.S)};
        const int got[] = {p.ok, p.tail, p.regen_rows, (int)p.regen_off, (int)p.ee_off, (int)p.slice, (int)p.lds, p.quad, (int)p.grid, p.vw, asked[0], asked[1], asked[2]};
        const int want[] = {r.ok, r.tail, r.regen_rows, r.regen_off, r.ee_off, r.slice, r.lds, r.quad, r.grid, r.vw, r.regen_rows1, r.regen_rows2, r.ee_fits};
        const bool same = p.ok ? std::memcmp(got, want, sizeof(got)) == 0 : !r.ok && std::memcmp(got + 10, want + 10, 3 * sizeof(int)) == 0;
        const bool laid_out = !p.ok || r.shape.P <= 0 || regions_ok(p, r.wants);
        const bool named = std::strcmp(p.kernel, !p.ok || r.shape.P <= 0 ? "" : p.quad ? "update_kernel_quad" : "update_kernel") == 0;
        n += 1;
        if (!same || !laid_out || !named || std::memcmp(&p.shape, &r.shape, sizeof(UpdateShape)) != 0) {
            bad += 1;
            std::fprintf(stderr, "row %d (dtype %d costs %d n %d T %d S %d P %d wants %d%d%d%d%d wide %d)%s%s:\n  got ", n, r.shape.dtype, r.shape.costs_dtype,
                         r.shape.n, r.shape.T, r.shape.S, r.shape.P, r.wants.isw_tail, r.wants.regen_recipe, r.wants.ee_fold, r.wants.beside_chain,
                         r.wants.has_nnz, r.update_wide, laid_out ? "" : " REGIONS OVERLAP OR LEAVE THE SCRATCH", named ? "" : " kernel name wrong");
            for (int v : got) std::fprintf(stderr, " %d", v);
            std::fprintf(stderr, "\n  want");
            for (int v : want) std::fprintf(stderr, " %d", v);
            std::fprintf(stderr, "\n");
        }
    }
    std::printf("%d rows, %d wrong\n", n, bad);
    if (bad == 0 && n > 700) std::printf("UPDATE_TABLE_OK\n");
    return bad != 0;
}
