// TEST-ONLY: CPU build of the primal-dual warm-start conversion (boundmpc_amd/csrc/bmpc_dual.inl) over the lane emulator of the wave
// program (the same text the GPU kernel bmpc_service_kernel<ZLDS, DualBatch> runs, its slicing of the batch included; phases as loops over the 64 lanes in a caller-chosen order).  Used by
// tests/test_dual_warm_start.py; never built, loaded or fallen back to by the product.
#include <cstdio>
#include <cstring>
#include <vector>

#include "bmpc_emu_host.h"
#include "../../boundmpc_amd/csrc/bmpc_dual.inl"

// state [B][57 N + 2] from (p, x0, lam_g, lam_x) of B problems; lam_g / lam_x may be NULL.  poison: LDS and workspace hold NaN before every
// problem (a read of a word the conversion has not written shows up in the state)
extern "C" int bmpc_emu_state_from_multipliers(int N, int S, double h, const bmpc::Opts *opts, int B, const double *p, const double *x0,
                                               const double *lam_g, const double *lam_x, double mu0, double *state, int lane_order, int poison) {
    if (!bmpc::emu_shape_ok(N, S)) return 1;
    std::vector<double> lds(bmpc::L_SIZE, 0.0), scr(bmpc::make_scr(N).size, 0.0);
    const ServiceArgsT<bmpc::Opts, bmpc::DualBatch> a{N, S, B, h, *opts, scr.data(), 0, {p, x0, lam_g, lam_x, state, mu0}};
    for (int b = 0; b < B; b++) {
        bmpc::Wave W = bmpc::emu_wave(a, lds, scr, lane_order, 0, poison);
        const bmpc::DualIn d = a.job.problem(N, S, b);
        if (bmpc::emu_zlds(N, S)) bmpc::wave_state_from_multipliers<true>(W, d); else bmpc::wave_state_from_multipliers<false>(W, d);
    }
    return 0;
}
