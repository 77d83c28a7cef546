// The plain GPMP solve's ONE launch decision (csrc/sgpmp_internal.h: gpmp_solve_layout, the function launch_gpmp_solve and
// sgpmp_gpmp_solve call) printed for every admissible traj_len and field count, on the CPU under AddressSanitizer + UBSan:
// one line "T F ppw per_particle lds" per pair, then GPMP_LAYOUT_OK.  tests/test_cpu_gpmp_dense.py holds the lines to the
// arithmetic and to the boundary rows.  TEST INFRASTRUCTURE.
#include <cstdio>

#include "sgpmp_internal.h"

int main() {
    std::printf("LIMITS %d %d\n", SGPMP_MAX_T_GPMP, SGPMP_MAX_GPMP_FIELDS);
    for (int T = 2; T <= SGPMP_MAX_T_GPMP; ++T)
        for (int F = 0; F <= SGPMP_MAX_GPMP_FIELDS; ++F) {
            const GpmpSolveLayout l = gpmp_solve_layout(T, F);
            std::printf("%d %d %d %zu %zu\n", T, F, l.ppw, l.per_particle, l.lds);
        }
    std::printf("GPMP_LAYOUT_OK\n");
    return 0;
}
