// TEST-ONLY: CPU build of the rollout (boundmpc_amd/csrc/bmpc_rollout_kernel.inl), the same text the GPU kernels bmpc_stream_rollout_kernel<ZLDS, RESTO>
// run, in the host's entry words (bmpc_emu_host.h: the stream functions with one lane, the wave program inside with its phases as loops over the 64
// lanes), one stream per call.
// Used by tests/test_stream_rollout.py and tests/test_gpu_stream_rollout.py; never built, loaded or fallen back to by the product.
// With -DBMPC_EMU_ROLLOUT_MAIN a stand-alone program for a sanitizer build: it reads a case file (tests/emu/emu_rollout.py write_case), runs the
// fused tick's text (bmpc_emu.cpp, compiled beside this file) and the rollout and prints ticks_run and a checksum.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "bmpc_emu_host.h"
#include "../../boundmpc_amd/csrc/bmpc_stream.inl"

typedef KArgsT<bmpc::Opts> KArgs;
#include "../../boundmpc_amd/csrc/bmpc_rollout_kernel.inl"

extern "C" int bmpc_emu_stream_rollout_len() { return bmpcs::RH_LEN; }
// One stream: the arguments of bmpc_stream_rollout with B = 1 (path [cap][48]), behind the solver options and in front of what the handle holds
// (real-time tolerance, position-row cap, level rule).  Returns 1 where the C ABI returns BMPC_ERR_ARG (but for the time budget: no handle here).
// The instantiation is chosen as the library chooses it: iterate in LDS by the horizon rule, the restoration phase by the option record.
extern "C" int bmpc_emu_stream_rollout(int N, int S, double h, const bmpc::Opts *opts, int ticks, const double *path, int cap, double *ss, double *rb, double *p,
                                       double *x0, double *dual, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                                       double goal_tol, double *hist, double *traj_hist, int *ticks_run, double rt_tol, double rt_row_cap, double lvl_c, double lvl_lo,
                                       double lvl_hi, int lane_order) {
    if (!bmpc::emu_shape_ok(N, S) || N > bmpcs::STREAM_NMAX || cap < S + 1 || max_iter < 0 || !path || !ss || !rb || !p || !x0 || !x || !g || !status || !traj) return 1;
    if (ticks < 1 || !(flags & 1) || !(goal_tol >= 0.0) || !std::isfinite(goal_tol)) return 1;
    KArgs a = bmpc::emu_args(N, S, 1, h, *opts);
    if (max_iter > 0) a.o.max_iter = max_iter;
    a.o.verbose = 0; a.o.retry_cap = 0;
    a.p = p; a.x0 = x0; a.state = dual; a.x = x; a.g = g; a.iters = iters; a.status = status; a.kkt = kkt;
    SArgs s; s.path = path; s.path_stride = cap * bmpcs::PT_LEN; s.ss = ss; s.rb = rb; s.traj = traj; s.flags = flags; s.rt_tol = rt_tol; s.rt_row_cap = rt_row_cap;
    s.lvl_c = lvl_c; s.lvl_lo = lvl_lo; s.lvl_hi = lvl_hi;
    const RArgs r{ticks, goal_tol, hist, traj_hist, ticks_run};
    std::vector<double> scr(bmpc::make_scr(N).size, 0.0);
    a.scratch = scr.data(); a.scr_stride = (long long)scr.size();
    emu_launch = EmuLaunch{0, 1, lane_order, 0};      // one workgroup
    const bool zl = bmpc::emu_zlds(N, S), resto = opts->restoration != 0;
    if (zl && resto) bmpc_stream_rollout_kernel<true, true>(a, s, r);
    else if (zl) bmpc_stream_rollout_kernel<true, false>(a, s, r);
    else if (resto) bmpc_stream_rollout_kernel<false, true>(a, s, r);
    else bmpc_stream_rollout_kernel<false, false>(a, s, r);
    return 0;
}

#ifdef BMPC_EMU_ROLLOUT_MAIN
// case file (doubles): N S h ticks cap flags goal_tol max_iter tick0_cap | path [cap][48] | ss | rb.  Tick 0 is solved with tick0_cap by the fused tick's
// text, then `ticks` ticks with max_iter by the rollout's; every array is exactly as long as the kernel text may index it, so that an access outside is seen.
extern "C" int bmpc_emu_stream_tick(int N, int S, double h, const bmpc::Opts *opts, int B, const double *path, int path_entries, double *ss, double *rb, double *p, double *x0,
                                    double *dual, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags, double rt_tol,
                                    double rt_row_cap, double lvl_c, double lvl_lo, double lvl_hi, int lane_order, int wave_order);
int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s case.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    double hd[9];
    if (fread(hd, sizeof(double), 9, f) != 9) return 2;
    const int N = (int)hd[0], S = (int)hd[1], ticks = (int)hd[3], cap = (int)hd[4], flags = (int)hd[5], max_iter = (int)hd[7], cap0 = (int)hd[8];
    const int TRN = bmpcs::tr_len(N);
    std::vector<double> path((size_t)cap * bmpcs::PT_LEN), ss(bmpcs::ss_len(N)), rb(bmpcs::RB_LEN);
    if (fread(path.data(), sizeof(double), path.size(), f) != path.size() || fread(ss.data(), sizeof(double), ss.size(), f) != ss.size()
        || fread(rb.data(), sizeof(double), rb.size(), f) != rb.size()) return 2;
    fclose(f);
    bmpc::Opts o; bmpc_opts_for(N, o); o.start_rollout = 0;
    std::vector<double> p(141 + 91 * S), x0(44 * N), dual(57 * N + 2, 0.0), x(44 * N), g(43 * N), traj(TRN), hist((size_t)ticks * bmpcs::RH_LEN), th((size_t)ticks * TRN);
    int iters = 0, status = 0, run = 0; double kkt = 0.0;
    int rc = bmpc_emu_stream_tick(N, S, hd[2], &o, 1, path.data(), cap, ss.data(), rb.data(), p.data(), x0.data(), dual.data(), cap0, x.data(), g.data(), &iters, &status,
                                  &kkt, traj.data(), 1, 1e-4, 0.0, 0.0, 0.0, 0.0, 0, 0);
    if (rc == 0) rc = bmpc_emu_stream_rollout(N, S, hd[2], &o, ticks, path.data(), cap, ss.data(), rb.data(), p.data(), x0.data(), dual.data(), max_iter, x.data(), g.data(),
                                              &iters, &status, &kkt, traj.data(), flags, hd[6], hist.data(), th.data(), &run, 1e-4, 0.0, 0.0, 0.0, 0.0, 0);
    double sum = 0.0;
    for (int t = 0; t < run; t++) for (int i = 0; i < bmpcs::RH_LEN; i++) sum += hist[(size_t)t * bmpcs::RH_LEN + i];
    printf("rc %d ticks_run %d of %d status %d iters %d phi %.17g checksum %.17g\n", rc, run, ticks, status, iters, ss[bmpcs::SS_PHI], sum);
    return rc;
}
#endif
