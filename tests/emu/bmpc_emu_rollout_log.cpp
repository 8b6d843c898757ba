// TEST-ONLY: CPU build of the rollout WITH THE LOG (boundmpc_amd/csrc/bmpc_rollout_kernel.inl, EV, AU and LG), the same text the GPU kernels
// bmpc_stream_rollout_kernel<ZLDS, RESTO, true, true, true> run, in the host's entry words (bmpc_emu_host.h).  One workgroup serves the B streams of a
// call, one after the other -- the kernel's own stride.  Used by tests/test_stream_rollout_log.py and tests/test_gpu_stream_rollout_log.py; never built,
// loaded or fallen back to by the product.
// With -DBMPC_EMU_ROLLOUT_LOG_MAIN a stand-alone program for a sanitizer build: it reads a case file of the rollout with events
// (tests/emu/emu_rollout_events.py write_case), runs the rollout with events, audit and log on exact-size buffers and prints ticks_run and the tracking
// record.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "bmpc_emu_host.h"
#include "../../boundmpc_amd/csrc/bmpc_stream.inl"

typedef KArgsT<bmpc::Opts> KArgs;
#include "../../boundmpc_amd/csrc/bmpc_rollout_kernel.inl"

extern "C" int bmpc_emu_stream_track_len(void) { return bmpcs::TRACK_LEN; }
extern "C" int bmpc_emu_stream_rollout_log_len(int N, int log_stages) { return (log_stages >= 1 && log_stages <= N) ? bmpcs::LOG_STAGE * log_stages + 4 : -1; }

// B streams: the arguments of bmpc_stream_rollout_log (path [B][cap][48]), behind the solver options and in front of what the handle holds.  Returns 1
// where the C ABI returns BMPC_ERR_ARG (but for the time budget: no handle here).  *ran (may be NULL) says which instantiation ran: 3 with the log code,
// 2 with events and audit, 1 with events alone -- with log_hist and track both NULL the entry IS the rollout with the audit, and that one without its
// arrays the rollout with events.
extern "C" int bmpc_emu_stream_rollout_log(int N, int S, double h, const bmpc::Opts *opts, int B, int ticks, double *path, int cap, double *ss, double *rb, double *p,
                                           double *x0, double *dual, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                                           double goal_tol, double *hist, double *traj_hist, int *ticks_run, double *replan, const int *replan_tick, int *replan_info,
                                           int update_flags, const double *disturb, double *tube_hist, double *audit, double audit_tol, double *log_hist, int log_stages,
                                           double *track, double rt_tol, double rt_row_cap, double lvl_c, double lvl_lo, double lvl_hi, int lane_order, int *ran) {
    if (ran) *ran = 0;
    if ((log_hist || track) && (log_stages < 1 || log_stages > N)) return 1;
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
    const RArgs r{ticks, goal_tol, hist, traj_hist, ticks_run, replan, replan_tick, replan_info, update_flags, disturb, tube_hist, audit, audit_tol, log_hist, log_stages, track};
    std::vector<double> scr(bmpc::make_scr(N).size, 0.0);
    a.scratch = scr.data(); a.scr_stride = (long long)scr.size();
    emu_launch = EmuLaunch{0, 1, lane_order, 0};      // one workgroup strides over the B streams
    const bool zl = bmpc::emu_zlds(N, S), resto = opts->restoration != 0;
    if (log_hist || track) {
        if (ran) *ran = 3;
        if (zl && resto) bmpc_stream_rollout_kernel<true, true, true, true, true>(a, s, r);
        else if (zl) bmpc_stream_rollout_kernel<true, false, true, true, true>(a, s, r);
        else if (resto) bmpc_stream_rollout_kernel<false, true, true, true, true>(a, s, r);
        else bmpc_stream_rollout_kernel<false, false, true, true, true>(a, s, r);
    } else if (tube_hist || audit) {
        if (ran) *ran = 2;
        if (zl && resto) bmpc_stream_rollout_kernel<true, true, true, true>(a, s, r);
        else if (zl) bmpc_stream_rollout_kernel<true, false, true, true>(a, s, r);
        else if (resto) bmpc_stream_rollout_kernel<false, true, true, true>(a, s, r);
        else bmpc_stream_rollout_kernel<false, false, true, true>(a, s, r);
    } else {
        if (ran) *ran = 1;
        if (zl && resto) bmpc_stream_rollout_kernel<true, true, true>(a, s, r);
        else if (zl) bmpc_stream_rollout_kernel<true, false, true>(a, s, r);
        else if (resto) bmpc_stream_rollout_kernel<false, true, true>(a, s, r);
        else bmpc_stream_rollout_kernel<false, false, true>(a, s, r);
    }
    return 0;
}

#ifdef BMPC_EMU_ROLLOUT_LOG_MAIN
// case file (doubles): N S h ticks cap flags goal_tol max_iter replan_tick update_flags | path [cap][48] | ss | rb | replan [replan_len] | disturb [ticks][21].
// One stream from its cold start, twice: rows of all N stages with the record, then the record alone (its stage-0 row in the kernel's own words).  Every
// array is exactly as long as the kernel text may index it, so that an access outside is seen.
int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s case.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    double hd[10];
    if (fread(hd, sizeof(double), 10, f) != 10) return 2;
    const int N = (int)hd[0], S = (int)hd[1], ticks = (int)hd[3], cap = (int)hd[4], flags = (int)hd[5], max_iter = (int)hd[7], rtick = (int)hd[8], uflags = (int)hd[9];
    const int TRN = bmpcs::tr_len(N);
    std::vector<double> path0((size_t)cap * bmpcs::PT_LEN), ss0(bmpcs::ss_len(N)), rb0(bmpcs::RB_LEN), rec0(bmpcs::replan_len(S, cap)), dist((size_t)ticks * bmpcs::DIST_LEN);
    for (std::vector<double> *v : {&path0, &ss0, &rb0, &rec0, &dist}) if (fread(v->data(), sizeof(double), v->size(), f) != v->size()) return 2;
    fclose(f);
    bmpc::Opts o; bmpc_opts_for(N, o); o.start_rollout = 0;
    int rc = 0;
    for (int pass = 0; pass < 2 && rc == 0; pass++) {
        const int stages = pass == 0 ? N : 1;
        std::vector<double> path(path0), ss(ss0), rb(rb0), rec(rec0);
        std::vector<double> p(141 + 91 * S), x0(44 * N), dual(57 * N + 2, 0.0), x(44 * N), g(43 * N), traj(TRN), hist((size_t)ticks * bmpcs::RH_LEN),
            tube((size_t)ticks * bmpcs::TUBE_LEN), audit(bmpcs::AUDIT_LEN), log((size_t)ticks * (bmpcs::LOG_STAGE * stages + 4)), track(bmpcs::TRACK_LEN);
        int iters = 0, status = 0, run = 0, info = -7, ran = 0; double kkt = 0.0;
        rc = bmpc_emu_stream_rollout_log(N, S, hd[2], &o, 1, ticks, path.data(), cap, ss.data(), rb.data(), p.data(), x0.data(), dual.data(), max_iter, x.data(), g.data(),
                                         &iters, &status, &kkt, traj.data(), flags, hd[6], hist.data(), nullptr, &run, rec.data(), &rtick, &info, uflags, dist.data(),
                                         tube.data(), audit.data(), 1e-6, pass == 0 ? log.data() : nullptr, stages, track.data(), 1e-4, 0.0, 0.0, 0.0, 0.0, 0, &ran);
        printf("%src %d ran %d ticks_run %d of %d stages %d samples %g max_ep_orth %.6g at %g max_ep_par %.6g at %g max_er %.6g at %g replayed %g", pass ? " | " : "", rc, ran, run,
               ticks, stages, track[bmpcs::TRACK_SAMPLES], track[bmpcs::TRACK_MAX_EP_ORTH], track[bmpcs::TRACK_TICK_EP_ORTH], track[bmpcs::TRACK_MAX_EP_PAR],
               track[bmpcs::TRACK_TICK_EP_PAR], track[bmpcs::TRACK_MAX_ER], track[bmpcs::TRACK_TICK_ER], track[bmpcs::TRACK_REPLAYED]);
    }
    printf("\n");
    return rc;
}
#endif
