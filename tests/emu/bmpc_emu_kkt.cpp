// TEST-ONLY: CPU build of the KKT certificate (boundmpc_amd/csrc/bmpc_kkt.inl) over the lane emulator of the wave program (the same text the
// GPU kernel bmpc_service_kernel<ZLDS, KktBatch> runs, its slicing of the batch included; phases as loops over the 64 lanes in a caller-chosen order).  Used by tests/test_kkt_certificate.py; never
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
#include "../../boundmpc_amd/csrc/bmpc_kkt.inl"

extern "C" int bmpc_emu_kkt_len(void) { return bmpc::KKT_LEN; }

// cert [B][8] (and g [B][43 N], lam_g [B][43 N], rj [B][8 N] where not NULL) of the points (p, x, lam_g0, lam_x0) of B problems; lam_g0 / lam_x0
// may be NULL.  poison: LDS and workspace hold NaN before every problem (a read of a word the certificate has not written shows up in the record)
extern "C" int bmpc_emu_kkt(int N, int S, double h, const bmpc::Opts *opts, int B, const double *p, const double *x, const double *lam_g0,
                            const double *lam_x0, double *cert, double *g, double *lam_g, double *rj, int lane_order, int poison) {
    if (S > bmpc::SMAX || S < 2 || N < 1 || N > bmpc::NMAX) return 1;
    const bmpc::Scr sc = bmpc::make_scr(N);
    const bmpc::KktBatch a{p, x, lam_g0, lam_x0, cert, g, lam_g, rj};
    std::vector<double> lds(bmpc::L_SIZE, 0.0), scr(sc.size, 0.0);
    for (int b = 0; b < B; b++) {
        if (poison) { std::fill(lds.begin(), lds.end(), std::nan("")); std::fill(scr.begin(), scr.end(), std::nan("")); }
        bmpc::Wave W; W.N = N; W.S = S; W.h = h; W.o = *opts; W.L = lds.data(); W.G = bmpc::make_gptr(scr.data()); W.wv = 0; W.it_base = 0;
        for (int i = 0; i < 64; i++) W.order[i] = lane_order == 0 ? i : (lane_order == 1 ? 63 - i : (i * 37 + 11) % 64);
        const bmpc::KktIn d = a.problem(N, S, b);
        if (N <= 11 && S <= bmpc::SMAX_ZLDS) bmpc::wave_certify<true>(W, d); else bmpc::wave_certify<false>(W, d);
    }
    return 0;
}
