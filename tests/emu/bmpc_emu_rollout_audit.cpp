// TEST-ONLY: CPU build of the rollout WITH THE AUDIT (boundmpc_amd/csrc/bmpc_rollout_kernel.inl, EV and AU), the same text the GPU kernels
// bmpc_stream_rollout_kernel<ZLDS, RESTO, true, true> run, in the host's entry words (bmpc_emu_host.h).  One workgroup serves the B streams of a call,
// one after the other -- the kernel's own stride.  Used by tests/test_stream_tube.py and tests/test_gpu_stream_tube.py; never built, loaded or fallen
// back to by the product.
// With -DBMPC_EMU_ROLLOUT_AUDIT_MAIN a stand-alone program for a sanitizer build: it reads a case file of the rollout with events
// (tests/emu/emu_rollout_events.py write_case), runs the rollout with events and audit and prints ticks_run and the audit record.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "bmpc_emu_host.h"
#include "../../boundmpc_amd/csrc/bmpc_stream.inl"

typedef KArgsT<bmpc::Opts> KArgs;
#include "../../boundmpc_amd/csrc/bmpc_rollout_kernel.inl"

// B streams: the arguments of bmpc_stream_rollout_audit (path [B][cap][48]), behind the solver options and in front of what the handle holds.  Returns 1
// where the C ABI returns BMPC_ERR_ARG (but for the time budget: no handle here).  With tube_hist and audit both NULL the instantiation without the
// audit code runs, as the entry calls the rollout with events then.
extern "C" int bmpc_emu_stream_rollout_audit(int N, int S, double h, const bmpc::Opts *opts, int B, int ticks, double *path, int cap, double *ss, double *rb, double *p,
                                             double *x0, double *dual, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                                             double goal_tol, double *hist, double *traj_hist, int *ticks_run, double *replan, const int *replan_tick, int *replan_info,
                                             int update_flags, const double *disturb, double *tube_hist, double *audit, double audit_tol, double rt_tol, double rt_row_cap,
                                             double lvl_c, double lvl_lo, double lvl_hi, int lane_order) {
    if (!(audit_tol >= 0.0) || !std::isfinite(audit_tol)) return 1;
    if (!bmpc::emu_shape_ok(N, S) || N > bmpcs::STREAM_NMAX || cap < S + 1 || max_iter < 0 || B < 1 || !path || !ss || !rb || !p || !x0 || !x || !g || !status || !traj) return 1;
    if (ticks < 1 || !(flags & 1) || !(goal_tol >= 0.0) || !std::isfinite(goal_tol)) return 1;
    if ((replan && !replan_tick) || (update_flags & ~7) || ((update_flags & 4) && !(update_flags & 2))) return 1;
    KArgs a = bmpc::emu_args(N, S, B, h, *opts);
    if (max_iter > 0) a.o.max_iter = max_iter;
    a.o.verbose = 0; a.o.retry_cap = 0;
    a.p = p; a.x0 = x0; a.state = dual; a.x = x; a.g = g; a.iters = iters; a.status = status; a.kkt = kkt;
    SArgs s; s.path = path; s.path_stride = cap * bmpcs::PT_LEN; s.ss = ss; s.rb = rb; s.traj = traj; s.flags = flags; s.rt_tol = rt_tol; s.rt_row_cap = rt_row_cap;
    s.lvl_c = lvl_c; s.lvl_lo = lvl_lo; s.lvl_hi = lvl_hi;
    const RArgs r{ticks, goal_tol, hist, traj_hist, ticks_run, replan, replan_tick, replan_info, update_flags, disturb, tube_hist, audit, audit_tol};
    std::vector<double> scr(bmpc::make_scr(N).size, 0.0);
    a.scratch = scr.data(); a.scr_stride = (long long)scr.size();
    emu_launch = EmuLaunch{0, 1, lane_order, 0};      // one workgroup strides over the B streams
    const bool zl = bmpc::emu_zlds(N, S), resto = opts->restoration != 0;
    if (tube_hist || audit) {
        if (zl && resto) bmpc_stream_rollout_kernel<true, true, true, true>(a, s, r);
        else if (zl) bmpc_stream_rollout_kernel<true, false, true, true>(a, s, r);
        else if (resto) bmpc_stream_rollout_kernel<false, true, true, true>(a, s, r);
        else bmpc_stream_rollout_kernel<false, false, true, true>(a, s, r);
    } else {
        if (zl && resto) bmpc_stream_rollout_kernel<true, true, true>(a, s, r);
        else if (zl) bmpc_stream_rollout_kernel<true, false, true>(a, s, r);
        else if (resto) bmpc_stream_rollout_kernel<false, true, true>(a, s, r);
        else bmpc_stream_rollout_kernel<false, false, true>(a, s, r);
    }
    return 0;
}

#ifdef BMPC_EMU_ROLLOUT_AUDIT_MAIN
// case file (doubles): N S h ticks cap flags goal_tol max_iter replan_tick update_flags | path [cap][48] | ss | rb | replan [replan_len] | disturb [ticks][21].
// One stream from its cold start; every array is exactly as long as the kernel text may index it, so that an access outside is seen.
int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s case.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    double hd[10];
    if (fread(hd, sizeof(double), 10, f) != 10) return 2;
    const int N = (int)hd[0], S = (int)hd[1], ticks = (int)hd[3], cap = (int)hd[4], flags = (int)hd[5], max_iter = (int)hd[7], rtick = (int)hd[8], uflags = (int)hd[9];
    const int TRN = bmpcs::tr_len(N);
    std::vector<double> path((size_t)cap * bmpcs::PT_LEN), ss(bmpcs::ss_len(N)), rb(bmpcs::RB_LEN), rec(bmpcs::replan_len(S, cap)), dist((size_t)ticks * bmpcs::DIST_LEN);
    for (std::vector<double> *v : {&path, &ss, &rb, &rec, &dist}) if (fread(v->data(), sizeof(double), v->size(), f) != v->size()) return 2;
    fclose(f);
    bmpc::Opts o; bmpc_opts_for(N, o); o.start_rollout = 0;
    std::vector<double> p(141 + 91 * S), x0(44 * N), dual(57 * N + 2, 0.0), x(44 * N), g(43 * N), traj(TRN), hist((size_t)ticks * bmpcs::RH_LEN),
        tube((size_t)ticks * bmpcs::TUBE_LEN), audit(bmpcs::AUDIT_LEN);
    int iters = 0, status = 0, run = 0, info = -7; double kkt = 0.0;
    const int rc = bmpc_emu_stream_rollout_audit(N, S, hd[2], &o, 1, ticks, path.data(), cap, ss.data(), rb.data(), p.data(), x0.data(), dual.data(), max_iter, x.data(),
                                                 g.data(), &iters, &status, &kkt, traj.data(), flags, hd[6], hist.data(), nullptr, &run, rec.data(), &rtick, &info, uflags,
                                                 dist.data(), tube.data(), audit.data(), 1e-6, 1e-4, 0.0, 0.0, 0.0, 0.0, 0);
    printf("rc %d ticks_run %d of %d samples %g max_pos %.6g at %g max_rot %.6g at %g max_q %.6g max_dq %.6g n_pos %g n_rot %g n_joint %g first_out %g\n", rc, run, ticks,
           audit[bmpcs::AUDIT_SAMPLES], audit[bmpcs::AUDIT_MAX_POS], audit[bmpcs::AUDIT_TICK_POS], audit[bmpcs::AUDIT_MAX_ROT], audit[bmpcs::AUDIT_TICK_ROT],
           audit[bmpcs::AUDIT_MAX_Q], audit[bmpcs::AUDIT_MAX_DQ], audit[bmpcs::AUDIT_N_POS], audit[bmpcs::AUDIT_N_ROT], audit[bmpcs::AUDIT_N_JOINT], audit[bmpcs::AUDIT_FIRST_OUT]);
    return rc;
}
#endif
