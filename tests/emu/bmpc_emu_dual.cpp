// TEST-ONLY: CPU build of the primal-dual warm-start conversion (boundmpc_amd/csrc/bmpc_dual.inl) over the lane emulator of the wave
// program (the same text the GPU kernel bmpc_service_kernel<ZLDS, DualBatch> runs, its slicing of the batch included; phases as loops over the 64 lanes in a caller-chosen order).  Used by
// tests/test_dual_warm_start.py; never built, loaded or fallen back to by the product.
#include <cstdio>
#include <cstring>
#include <vector>

#include "bmpc_emu_host.h"
#define LANES_BEGIN for (int li_ = 0; li_ < 64; ++li_) { const int lane = W.order[li_]; (void)lane;
#define LANES_END }
#define LIDX lane

#include "../../boundmpc_amd/csrc/bmpc_wave.inl"
#include "../../boundmpc_amd/csrc/bmpc_dual.inl"

// state [B][57 N + 2] from (p, x0, lam_g, lam_x) of B problems; lam_g / lam_x may be NULL.  poison: LDS and workspace hold NaN before every
// problem (a read of a word the conversion has not written shows up in the state)
extern "C" int bmpc_emu_state_from_multipliers(int N, int S, double h, const bmpc::Opts *opts, int B, const double *p, const double *x0,
                                               const double *lam_g, const double *lam_x, double mu0, double *state, int lane_order, int poison) {
    if (S > bmpc::SMAX || S < 2 || N < 1 || N > bmpc::NMAX) return 1;
    const bmpc::Scr sc = bmpc::make_scr(N);
    const bmpc::DualBatch a{p, x0, lam_g, lam_x, state, mu0};
    std::vector<double> lds(bmpc::L_SIZE, 0.0), scr(sc.size, 0.0);
    for (int b = 0; b < B; b++) {
        if (poison) { std::fill(lds.begin(), lds.end(), std::nan("")); std::fill(scr.begin(), scr.end(), std::nan("")); }
        bmpc::Wave W; W.N = N; W.S = S; W.h = h; W.o = *opts; W.L = lds.data(); W.G = bmpc::make_gptr(scr.data()); W.wv = 0; W.it_base = 0;
        for (int i = 0; i < 64; i++) W.order[i] = lane_order == 0 ? i : (lane_order == 1 ? 63 - i : (i * 37 + 11) % 64);
        const bmpc::DualIn d = a.problem(N, S, b);
        if (N <= 11 && S <= bmpc::SMAX_ZLDS) bmpc::wave_state_from_multipliers<true>(W, d); else bmpc::wave_state_from_multipliers<false>(W, d);
    }
    return 0;
}
