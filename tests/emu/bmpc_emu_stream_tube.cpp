// TEST-ONLY: CPU build of the tube measurement (boundmpc_amd/csrc/bmpc_stream_tube.inl), the same text the GPU kernel bmpc_stream_tube_kernel and
// the rollouts with the audit run, with one lane.  Used by tests/test_stream_tube.py and tests/test_gpu_stream_tube.py; never built, loaded or
// fallen back to by the product.
// With -DBMPC_EMU_STREAM_TUBE_MAIN a stand-alone program for a sanitizer build: it reads a case file (tests/emu/emu_stream_tube.py write_case) and
// prints the tube row of every parameter vector in it.
#include <cstdio>

#include "bmpc_emu_host.h"
#include "../../boundmpc_amd/csrc/bmpc_stream.inl"
#include "../../boundmpc_amd/csrc/bmpc_stream_tube.inl"

extern "C" int bmpc_emu_stream_tube_len() { return bmpcs::TUBE_LEN; }
extern "C" int bmpc_emu_stream_audit_len() { return bmpcs::AUDIT_LEN; }
// B streams: p [B][141 + 91 S], ss [B][ss_len(N)] or NULL -> tube [B][16].  Returns 1 where the C ABI returns BMPC_ERR_ARG.
extern "C" int bmpc_emu_stream_tube(int N, int S, int B, const double *p, const double *ss, double *tube) {
    if (!bmpc::emu_shape_ok(N, S) || N > bmpcs::STREAM_NMAX || B < 1 || !p || !tube) return 1;
    for (int b = 0; b < B; b++)
        bmpcs::stream_tube(N, S, p + (long long)b * (141 + 91 * S), ss ? ss + (long long)b * bmpcs::ss_len(N) : nullptr, tube + (long long)b * bmpcs::TUBE_LEN, 0, 1);
    return 0;
}
// the verdict of one stream over its tube rows [T][16] (NaN rows = ticks not run, behind the rows of the ticks run) -> audit [12]
extern "C" void bmpc_emu_stream_audit(int T, const double *rows, double tol, double *audit) {
    bmpcs::stream_audit_init(audit);
    for (int t = 0; t < T; t++) {
        const double *row = rows + (long long)t * bmpcs::TUBE_LEN;
        if (row[bmpcs::TUBE_SEG] != row[bmpcs::TUBE_SEG]) break;
        bmpcs::stream_audit(row, audit, t, tol);
    }
}

#ifdef BMPC_EMU_STREAM_TUBE_MAIN
// case file (doubles): N S B with_state | p [B][141 + 91 S] | ss [B][ss_len(N)] (with_state only).  Every array is exactly as long as the text may
// index it, so that an access outside is seen.
int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s case.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    double hd[4];
    if (fread(hd, sizeof(double), 4, f) != 4) return 2;
    const int N = (int)hd[0], S = (int)hd[1], B = (int)hd[2], with_state = (int)hd[3];
    std::vector<double> p((size_t)B * (141 + 91 * S)), ss(with_state ? (size_t)B * bmpcs::ss_len(N) : 0), tube((size_t)B * bmpcs::TUBE_LEN), audit(bmpcs::AUDIT_LEN);
    for (std::vector<double> *v : {&p, &ss}) if (fread(v->data(), sizeof(double), v->size(), f) != v->size()) return 2;
    fclose(f);
    const int rc = bmpc_emu_stream_tube(N, S, B, p.data(), with_state ? ss.data() : nullptr, tube.data());
    bmpc_emu_stream_audit(B, tube.data(), 1e-6, audit.data());
    for (int b = 0; b < B; b++) {
        const double *t = tube.data() + (size_t)b * bmpcs::TUBE_LEN;
        printf("row %d seg %g phi %.6g ex_pos %.6g ex_rot %.6g ex_q %.6g ex_dq %.6g\n", b, t[bmpcs::TUBE_SEG], t[bmpcs::TUBE_PHI], t[bmpcs::TUBE_EX_POS], t[bmpcs::TUBE_EX_ROT],
               t[bmpcs::TUBE_EX_Q], t[bmpcs::TUBE_EX_DQ]);
    }
    printf("rc %d samples %g first_out %g\n", rc, audit[bmpcs::AUDIT_SAMPLES], audit[bmpcs::AUDIT_FIRST_OUT]);
    return rc;
}
#endif
