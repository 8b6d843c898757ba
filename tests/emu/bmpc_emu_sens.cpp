// TEST-ONLY: CPU build of the parametric sensitivity (boundmpc_amd/csrc/bmpc_sens.inl) over the lane emulator of the wave program (the same text
// the GPU kernel bmpc_service_kernel<ZLDS, SensBatch> runs, its slicing of the batch included; phases as loops over the 64 lanes in a caller-chosen order).  Used by tests/test_sensitivity.py; never
// built, loaded or fallen back to by the product.
#include <cstdio>
#include <cstring>
#include <vector>

#include "bmpc_emu_host.h"
#define LANES_BEGIN for (int li_ = 0; li_ < 64; ++li_) { const int lane = W.order[li_]; (void)lane;
#define LANES_END }
#define LIDX lane

#include "../../boundmpc_amd/csrc/bmpc_wave.inl"
#include "../../boundmpc_amd/csrc/bmpc_dual.inl"
#include "../../boundmpc_amd/csrc/bmpc_sens.inl"

extern "C" int bmpc_emu_sens_len(void) { return bmpc::SENS_LEN; }

// dx [B][44 N] (and dlam_eq [B][36 N], dnu [B][57 N], rec [B][4] where not NULL) of the points (p, x, lam_g0, lam_x0) of B problems along dp
// [B][n_p] at the barrier level mu; lam_g0 / lam_x0 may be NULL.  poison: LDS and workspace hold NaN before every problem (a read of a word the
// program has not written shows up in the result)
extern "C" int bmpc_emu_sens(int N, int S, double h, const bmpc::Opts *opts, int B, const double *p, const double *x, const double *lam_g0,
                             const double *lam_x0, const double *dp, double mu, double *dx, double *dlam_eq, double *dnu, double *rec,
                             int lane_order, int poison) {
    if (S > bmpc::SMAX || S < 2 || N < 1 || N > bmpc::NMAX) return 1;
    const bmpc::Scr sc = bmpc::make_scr(N);
    const bmpc::SensBatch a{p, x, lam_g0, lam_x0, dp, mu, dx, dlam_eq, dnu, rec};
    std::vector<double> lds(bmpc::L_SIZE, 0.0), scr(sc.size, 0.0);
    for (int b = 0; b < B; b++) {
        if (poison) { std::fill(lds.begin(), lds.end(), std::nan("")); std::fill(scr.begin(), scr.end(), std::nan("")); }
        bmpc::Wave W; W.N = N; W.S = S; W.h = h; W.o = *opts; W.L = lds.data(); W.G = bmpc::make_gptr(scr.data()); W.wv = 0; W.it_base = 0;
        for (int i = 0; i < 64; i++) W.order[i] = lane_order == 0 ? i : (lane_order == 1 ? 63 - i : (i * 37 + 11) % 64);
        const bmpc::SensIn d = a.problem(N, S, b);
        if (N <= 11 && S <= bmpc::SMAX_ZLDS) bmpc::wave_sensitivity<true>(W, d); else bmpc::wave_sensitivity<false>(W, d);
    }
    return 0;
}
