// TEST-ONLY: CPU build of the TEAM rollout (boundmpc_amd/csrc/bmpc_rollout_kernel.inl with BMPC_NW cooperating waves per stream, namespace bmpct), the
// same text the GPU kernels of boundmpc_amd/csrc/bmpc_team_rollout.hip run, in the host's entry words (bmpc_emu_host.h: the stream functions with one
// lane on wave 0, the team program inside with its wide phases as loops over the waves in a caller-chosen order).  Both instantiations of that unit: the
// plain one and the one with the event, audit and log code.  One workgroup serves the B streams of a call, one after the other -- the kernel's own stride.
// Used by tests/test_stream_team_rollout.py and tests/test_gpu_stream_team_rollout.py; never built, loaded or fallen back to by the product.
// With -DBMPC_EMU_TEAM_ROLLOUT_MAIN a stand-alone program for a sanitizer build: it reads a case file (tests/emu/emu_rollout.py write_case), runs the
// team tick's text (bmpc_emu.cpp compiled with the same BMPC_NW beside this file) for tick 0, then the plain team rollout and, on copies, the
// fully-featured one with exact-size audit and log buffers, under both wave orders, and prints ticks_run and a checksum.
#include <cmath>
#include <cstdio>
#include <cstring>

#ifndef BMPC_NW
#define BMPC_NW 4
#endif
#define BMPC_NAMESPACE bmpct
#include "bmpc_emu_host.h"
#include "../../boundmpc_amd/csrc/bmpc_stream.inl"

typedef KArgsT<bmpct::Opts> KArgs;
#include "../../boundmpc_amd/csrc/bmpc_rollout_kernel.inl"

extern "C" int bmpc_emu_team_rollout_waves() { return BMPC_NW; }
extern "C" int bmpc_emu_team_rollout_len() { return bmpcs::RH_LEN; }

// B streams: the arguments of bmpc_stream_rollout_log (path [B][cap][48]), behind the solver options and in front of what the handle holds and the lane
// and wave orders.  full = 0: the plain kernel (every event, audit and log pointer must be NULL), 1: the kernel with EV, AU and LG, which the library
// launches for the events, audit and log entries alike.  Returns 1 where the C ABI returns BMPC_ERR_ARG (but for the time budget: no handle here) and
// for a horizon the teams do not take.
extern "C" int bmpc_emu_team_stream_rollout(int N, int S, double h, const bmpct::Opts *opts, int B, int ticks, double *path, int cap, double *ss, double *rb, double *p,
                                            double *x0, double *dual, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                                            double goal_tol, double *hist, double *traj_hist, int *ticks_run, double *replan, const int *replan_tick, int *replan_info,
                                            int update_flags, const double *disturb, double *tube_hist, double *audit, double audit_tol, double *log_hist, int log_stages,
                                            double *track, double rt_tol, double rt_row_cap, double lvl_c, double lvl_lo, double lvl_hi, int lane_order, int wave_order,
                                            int full) {
    if (!full && (replan || replan_tick || replan_info || disturb || tube_hist || audit || log_hist || track)) return 1;
    if ((log_hist || track) && (log_stages < 1 || log_stages > N)) return 1;
    if (!(audit_tol >= 0.0) || !std::isfinite(audit_tol)) return 1;
    if (!bmpct::emu_shape_ok(N, S) || N > bmpcs::STREAM_NMAX || N > bmpct::TEAM_NMAX || !bmpct::emu_zlds(N, S) || cap < S + 1 || max_iter < 0 || B < 1
        || !path || !ss || !rb || !p || !x0 || !x || !g || !status || !traj) return 1;
    if (ticks < 1 || !(flags & 1) || !(goal_tol >= 0.0) || !std::isfinite(goal_tol)) return 1;
    if ((replan && !replan_tick) || (update_flags & ~7) || ((update_flags & 4) && !(update_flags & 2))) return 1;
    KArgs a = bmpct::emu_args(N, S, B, h, *opts);
    if (max_iter > 0) a.o.max_iter = max_iter;
    a.o.verbose = 0; a.o.retry_cap = 0;
    a.p = p; a.x0 = x0; a.state = dual; a.x = x; a.g = g; a.iters = iters; a.status = status; a.kkt = kkt;
    SArgs s; s.path = path; s.path_stride = cap * bmpcs::PT_LEN; s.ss = ss; s.rb = rb; s.traj = traj; s.flags = flags; s.rt_tol = rt_tol; s.rt_row_cap = rt_row_cap;
    s.lvl_c = lvl_c; s.lvl_lo = lvl_lo; s.lvl_hi = lvl_hi;
    const RArgs r{ticks, goal_tol, hist, traj_hist, ticks_run, replan, replan_tick, replan_info, update_flags, disturb, tube_hist, audit, audit_tol, log_hist, log_stages, track};
    std::vector<double> scr(bmpct::make_scr(N).size, 0.0);
    a.scratch = scr.data(); a.scr_stride = (long long)scr.size();
    emu_launch = EmuLaunch{0, 1, lane_order, wave_order};      // one workgroup strides over the B streams
    const bool resto = opts->restoration != 0;
    if (full && resto) bmpc_stream_rollout_kernel<true, true, true, true, true>(a, s, r);
    else if (full) bmpc_stream_rollout_kernel<true, false, true, true, true>(a, s, r);
    else if (resto) bmpc_stream_rollout_kernel<true, true>(a, s, r);
    else bmpc_stream_rollout_kernel<true, false>(a, s, r);
    return 0;
}

#ifdef BMPC_EMU_TEAM_ROLLOUT_MAIN
// case file (doubles): N S h ticks cap flags goal_tol max_iter tick0_cap | path [cap][48] | ss | rb.  Tick 0 is solved with tick0_cap by the team tick's
// text, then `ticks` ticks with max_iter by the team rollout's; every array is exactly as long as the kernel text may index it, so that an access outside is seen.
extern "C" int bmpc_emu_team_stream_tick(int N, int S, double h, const bmpct::Opts *opts, int B, const double *path, int path_entries, double *ss, double *rb, double *p,
                                         double *x0, double *dual, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                                         double rt_tol, double rt_row_cap, double lvl_c, double lvl_lo, double lvl_hi, int lane_order, int wave_order);
int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s case.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    double hd[9];
    if (fread(hd, sizeof(double), 9, f) != 9) return 2;
    const int N = (int)hd[0], S = (int)hd[1], ticks = (int)hd[3], cap = (int)hd[4], flags = (int)hd[5], max_iter = (int)hd[7], cap0 = (int)hd[8];
    const int TRN = bmpcs::tr_len(N);
    std::vector<double> path0((size_t)cap * bmpcs::PT_LEN), ss0(bmpcs::ss_len(N)), rb0(bmpcs::RB_LEN);
    if (fread(path0.data(), sizeof(double), path0.size(), f) != path0.size() || fread(ss0.data(), sizeof(double), ss0.size(), f) != ss0.size()
        || fread(rb0.data(), sizeof(double), rb0.size(), f) != rb0.size()) return 2;
    fclose(f);
    bmpct::Opts o; bmpc_opts_for(N, o); o.start_rollout = 0;
    int rc = 0; double first = 0.0;
    for (int pass = 0; pass < 4 && rc == 0; pass++) {      // plain and full, each under wave orders 0 and 1
        const int full = pass & 1, wo = pass >> 1;
        std::vector<double> path(path0), ss(ss0), rb(rb0);
        std::vector<double> p(141 + 91 * S), x0(44 * N), dual(57 * N + 2, 0.0), x(44 * N), g(43 * N), traj(TRN), hist((size_t)ticks * bmpcs::RH_LEN), th((size_t)ticks * TRN),
            tube((size_t)ticks * bmpcs::TUBE_LEN), audit(bmpcs::AUDIT_LEN), log((size_t)ticks * (bmpcs::LOG_STAGE * N + 4)), track(bmpcs::TRACK_LEN);
        int iters = 0, status = 0, run = 0; double kkt = 0.0;
        rc = bmpc_emu_team_stream_tick(N, S, hd[2], &o, 1, path.data(), cap, ss.data(), rb.data(), p.data(), x0.data(), dual.data(), cap0, x.data(), g.data(), &iters, &status,
                                       &kkt, traj.data(), 1, 1e-4, 0.0, 0.0, 0.0, 0.0, 0, wo);
        if (rc == 0) rc = bmpc_emu_team_stream_rollout(N, S, hd[2], &o, 1, ticks, path.data(), cap, ss.data(), rb.data(), p.data(), x0.data(), dual.data(), max_iter, x.data(),
                                                       g.data(), &iters, &status, &kkt, traj.data(), flags, hd[6], hist.data(), th.data(), &run, nullptr, nullptr, nullptr, 0,
                                                       nullptr, full ? tube.data() : nullptr, full ? audit.data() : nullptr, 1e-6, full ? log.data() : nullptr, N,
                                                       full ? track.data() : nullptr, 1e-4, 0.0, 0.0, 0.0, 0.0, 0, wo, full);
        double sum = 0.0;
        for (int t = 0; t < run; t++) for (int i = 0; i < bmpcs::RH_LEN; i++) sum += hist[(size_t)t * bmpcs::RH_LEN + i];
        printf("%s%s order %d: rc %d ticks_run %d of %d status %d iters %d phi %.17g checksum %.17g", pass ? " | " : "", full ? "full" : "plain", wo, rc, run, ticks, status,
               iters, ss[bmpcs::SS_PHI], sum);
        if (pass == 0) first = sum;
        else if (rc == 0 && !(sum == first)) { printf(" DIFFERS"); rc = 3; }      // (the four runs compute the same rows)
    }
    printf("\n");
    return rc;
}
#endif
