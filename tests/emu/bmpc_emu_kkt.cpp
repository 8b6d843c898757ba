// TEST-ONLY: CPU build of the KKT certificate (boundmpc_amd/csrc/bmpc_kkt.inl) over the lane emulator of the wave program (the same text the
// GPU kernel bmpc_service_kernel<ZLDS, KktBatch> runs, its slicing of the batch included; phases as loops over the 64 lanes in a caller-chosen order).  Used by tests/test_kkt_certificate.py; never
// built, loaded or fallen back to by the product.
#include <cstdio>
#include <cstring>
#include <vector>

#include "bmpc_emu_host.h"
#include "../../boundmpc_amd/csrc/bmpc_dual.inl"
#include "../../boundmpc_amd/csrc/bmpc_kkt.inl"

extern "C" int bmpc_emu_kkt_len(void) { return bmpc::KKT_LEN; }

// cert [B][8] (and g [B][43 N], lam_g [B][43 N], rj [B][8 N] where not NULL) of the points (p, x, lam_g0, lam_x0) of B problems; lam_g0 / lam_x0
// may be NULL.  poison: LDS and workspace hold NaN before every problem (a read of a word the certificate has not written shows up in the record)
extern "C" int bmpc_emu_kkt(int N, int S, double h, const bmpc::Opts *opts, int B, const double *p, const double *x, const double *lam_g0,
                            const double *lam_x0, double *cert, double *g, double *lam_g, double *rj, int lane_order, int poison) {
    if (!bmpc::emu_shape_ok(N, S)) return 1;
    std::vector<double> lds(bmpc::L_SIZE, 0.0), scr(bmpc::make_scr(N).size, 0.0);
    const ServiceArgsT<bmpc::Opts, bmpc::KktBatch> a{N, S, B, h, *opts, scr.data(), 0, {p, x, lam_g0, lam_x0, cert, g, lam_g, rj}};
    for (int b = 0; b < B; b++) {
        bmpc::Wave W = bmpc::emu_wave(a, lds, scr, lane_order, 0, poison);
        const bmpc::KktIn d = a.job.problem(N, S, b);
        if (bmpc::emu_zlds(N, S)) bmpc::wave_certify<true>(W, d); else bmpc::wave_certify<false>(W, d);
    }
    return 0;
}
