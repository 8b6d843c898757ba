// TEST-ONLY: CPU build of the parametric sensitivity (boundmpc_amd/csrc/bmpc_sens.inl) over the lane emulator of the wave program (the same text
// the GPU kernel bmpc_service_kernel<ZLDS, SensBatch> runs, its slicing of the batch included; phases as loops over the 64 lanes in a caller-chosen order).  Used by tests/test_sensitivity.py; never
// built, loaded or fallen back to by the product.
#include <cstdio>
#include <cstring>
#include <vector>

#include "bmpc_emu_host.h"
#include "../../boundmpc_amd/csrc/bmpc_dual.inl"
#include "../../boundmpc_amd/csrc/bmpc_sens.inl"

extern "C" int bmpc_emu_sens_len(void) { return bmpc::SENS_LEN; }

// dx [B][44 N] (and dlam_eq [B][36 N], dnu [B][57 N], rec [B][4] where not NULL) of the points (p, x, lam_g0, lam_x0) of B problems along dp
// [B][n_p] at the barrier level mu; lam_g0 / lam_x0 may be NULL.  poison: LDS and workspace hold NaN before every problem (a read of a word the
// program has not written shows up in the result)
extern "C" int bmpc_emu_sens(int N, int S, double h, const bmpc::Opts *opts, int B, const double *p, const double *x, const double *lam_g0,
                             const double *lam_x0, const double *dp, double mu, double *dx, double *dlam_eq, double *dnu, double *rec,
                             int lane_order, int poison) {
    if (!bmpc::emu_shape_ok(N, S)) return 1;
    std::vector<double> lds(bmpc::L_SIZE, 0.0), scr(bmpc::make_scr(N).size, 0.0);
    const ServiceArgsT<bmpc::Opts, bmpc::SensBatch> a{N, S, B, h, *opts, scr.data(), 0, {p, x, lam_g0, lam_x0, dp, mu, dx, dlam_eq, dnu, rec}};
    for (int b = 0; b < B; b++) {
        bmpc::Wave W = bmpc::emu_wave(a, lds, scr, lane_order, 0, poison);
        const bmpc::SensIn d = a.job.problem(N, S, b);
        if (bmpc::emu_zlds(N, S)) bmpc::wave_sensitivity<true>(W, d); else bmpc::wave_sensitivity<false>(W, d);
    }
    return 0;
}
