// TEST-ONLY: CPU build of the rollout (boundmpc_amd/csrc/bmpc_rollout_kernel.inl), the same text the GPU kernels bmpc_stream_rollout_kernel<ZLDS, RESTO,
// EV, AU, LG> run, in the host's entry words (bmpc_emu_host.h: the stream functions with one lane on wave 0, the wave program inside with its phases as
// loops over the 64 lanes and, for a team, its wide phases as loops over the waves in a caller-chosen order).  One source for every variant, built once
// per BMPC_NW as bmpc_emu.cpp is: one wave per stream (namespace bmpc; the four levels plain, EV, EV + AU, EV + AU + LG of the four one-wave units) or a
// team of BMPC_NW waves (-DBMPC_NW=4, namespace bmpct; the two levels of bmpc_team_rollout.hip, plain and everything).  One workgroup serves the B
// streams of a call, one after the other -- the kernel's own stride.  What the entry refuses and which level runs is the library's own rule
// (bmpc_rollout_level, csrc/bmpc_args.h), the instantiation is picked by the library's own piece (bmpc_rollout_run, bmpc_rollout_kernel.inl).
// Used by the tests/test_stream_*rollout*.py, tests/test_stream_tube.py and their GPU twins; never built, loaded or fallen back to by the product.
// With -DBMPC_EMU_ROLLOUT_MAIN a stand-alone program for a sanitizer build (tests/emu/emu_rollout.py run_sanitized, write_case; bmpc_emu.cpp with the
// same BMPC_NW is compiled beside this file for the tick text of tick 0).
#include <cmath>
#include <cstdio>
#include <cstring>

#ifndef BMPC_NW
#define BMPC_NW 1
#endif
#if BMPC_NW > 1
#define BMPC_NAMESPACE bmpct
#endif
#include "bmpc_emu_host.h"
#include "../../boundmpc_amd/csrc/bmpc_stream.inl"
namespace ns = BMPC_NAMESPACE;
typedef KArgsT<ns::Opts> KArgs;
#include "../../boundmpc_amd/csrc/bmpc_rollout_kernel.inl"

extern "C" int bmpc_emu_rollout_waves() { return BMPC_NW; }
extern "C" int bmpc_emu_stream_rollout_len() { return bmpcs::RH_LEN; }
extern "C" int bmpc_emu_stream_track_len() { return bmpcs::TRACK_LEN; }
extern "C" int bmpc_emu_stream_rollout_log_len(int N, int log_stages) { return (log_stages >= 1 && log_stages <= N) ? bmpcs::LOG_STAGE * log_stages + 4 : -1; }

// B streams: the arguments of bmpc_stream_rollout_log (path [B][cap][48]) behind the solver options, then what the handle holds (real-time tolerance,
// position-row cap, level rule), the lane and wave orders, the C ABI entry this call stands for (0 bmpc_stream_rollout, 1 _events, 2 _audit, 3 _log: what
// that entry has no argument for must be 0 / NULL), a forced level (-1: the library's rule; else that instantiation on the same arguments, which looks at
// nothing above its level) and *ran (may be NULL): the level that ran.  Teams hold levels 0 and 3 and run 3 for any level above 0, as the library does; a
// forced 1 or 2 is refused.  Returns 1 where the C ABI returns BMPC_ERR_ARG (but for the time budget: no handle here) and for a horizon the teams do not take.
extern "C" int bmpc_emu_stream_rollout(int N, int S, double h, const ns::Opts *opts, int B, int ticks, double *path, int cap, double *ss, double *rb, double *p, double *x0,
                                       double *dual, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags, double goal_tol,
                                       double *hist, double *traj_hist, int *ticks_run, double *replan, const int *replan_tick, int *replan_info, int update_flags,
                                       const double *disturb, double *tube_hist, double *audit, double audit_tol, double *log_hist, int log_stages, double *track,
                                       double rt_tol, double rt_row_cap, double lvl_c, double lvl_lo, double lvl_hi, int lane_order, int wave_order, int entry, int level,
                                       int *ran) {
    if (ran) *ran = -1;
    if (!ns::emu_shape_ok(N, S) || N > bmpcs::STREAM_NMAX || cap < S + 1 || max_iter < 0 || B < 1 || !path || !ss || !rb || !p || !x0 || !x || !g || !status || !traj) return 1;
#if BMPC_NW > 1
    if (N > ns::TEAM_NMAX || !ns::emu_zlds(N, S)) return 1;
#endif
    if (entry < 0 || entry > 3 || (entry < 1 && (replan || replan_tick || replan_info || disturb)) || (entry < 2 && (tube_hist || audit))
        || (entry < 3 && (log_hist || track))) return 1;
    const RArgs r{ticks, goal_tol, hist, traj_hist, ticks_run, replan, replan_tick, replan_info, update_flags, disturb, tube_hist, audit, audit_tol, log_hist, log_stages, track};
    const int ruled = bmpc_rollout_level(entry, r, N, flags, rb);
    if (ruled == BMPC_ROLLOUT_REFUSED) return 1;
    if (BMPC_NW > 1 && (level == 1 || level == 2)) return 1;
    if (level < 0) level = (BMPC_NW > 1 && ruled > 0) ? 3 : ruled;      // (teams: one kernel with everything serves every level above 0)
    KArgs a = ns::emu_args(N, S, B, h, *opts);
    if (max_iter > 0) a.o.max_iter = max_iter;
    a.o.verbose = 0; a.o.retry_cap = 0;
    a.p = p; a.x0 = x0; a.state = dual; a.x = x; a.g = g; a.iters = iters; a.status = status; a.kkt = kkt;
    const SArgs s{path, cap * bmpcs::PT_LEN, ss, rb, traj, flags, rt_tol, rt_row_cap, lvl_c, lvl_lo, lvl_hi};
    std::vector<double> scr(ns::make_scr(N).size, 0.0);
    a.scratch = scr.data(); a.scr_stride = (long long)scr.size();
    emu_launch = EmuLaunch{0, 1, lane_order, wave_order};      // one workgroup strides over the B streams
    const bool zl = ns::emu_zlds(N, S), resto = opts->restoration != 0;
    if (level == 0) bmpc_rollout_run<false, false, false>(zl, resto, &a, s, r, 1, 0);
    else if (level == 3) bmpc_rollout_run<true, true, true>(zl, resto, &a, s, r, 1, 0);
#if BMPC_NW == 1
    else if (level == 1) bmpc_rollout_run<true, false, false>(zl, resto, &a, s, r, 1, 0);
    else if (level == 2) bmpc_rollout_run<true, true, false>(zl, resto, &a, s, r, 1, 0);
#endif
    else return 1;
    if (ran) *ran = level;
    return 0;
}

#ifdef BMPC_EMU_ROLLOUT_MAIN
// case file (doubles): N S h ticks cap flags goal_tol max_iter tick0_cap replan_tick update_flags levels | path [cap][48] | ss | rb and, where `levels`
// names a level above 0 and has bit 4, | replan [replan_len] | disturb [ticks][21].  One stream, run once per level named by bits 0..3 of `levels`
// (teams: under wave orders 0 and 1 each) through the entry of that number, every run on fresh copies: with tick0_cap > 0 tick 0 is solved with that
// cap by the fused tick's text (bmpc_emu.cpp), then `ticks` ticks with max_iter by the rollout's.  On one wave level 3 runs twice: rows of all N stages
// with the tracking record, then the record alone (its stage-0 row in the kernel's own words).  Every array is exactly as long as the kernel text may
// index it, so that an access outside is seen; traj_hist is given at levels 0 and 1 and to the teams, NULL at levels 2 and 3 on one wave.  All runs of a case compute the same history rows: their checksums must agree.
#if BMPC_NW > 1
#define EMU_STREAM_TICK bmpc_emu_team_stream_tick
#else
#define EMU_STREAM_TICK bmpc_emu_stream_tick
#endif
extern "C" int EMU_STREAM_TICK(int N, int S, double h, const ns::Opts *opts, int B, const double *path, int path_entries, double *ss, double *rb, double *p, double *x0,
                               double *dual, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags, double rt_tol,
                               double rt_row_cap, double lvl_c, double lvl_lo, double lvl_hi, int lane_order, int wave_order);
int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s case.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    double hd[12];
    if (fread(hd, sizeof(double), 12, f) != 12) return 2;
    const int N = (int)hd[0], S = (int)hd[1], ticks = (int)hd[3], cap = (int)hd[4], flags = (int)hd[5], max_iter = (int)hd[7], cap0 = (int)hd[8], rtick = (int)hd[9],
              uflags = (int)hd[10], levels = (int)hd[11];
    const bool events = (levels & 16) != 0;
    const int TRN = bmpcs::tr_len(N);
    std::vector<double> path0((size_t)cap * bmpcs::PT_LEN), ss0(bmpcs::ss_len(N)), rb0(bmpcs::RB_LEN), rec0(events ? bmpcs::replan_len(S, cap) : 0),
        dist(events ? (size_t)ticks * bmpcs::DIST_LEN : 0);
    for (std::vector<double> *v : {&path0, &ss0, &rb0, &rec0, &dist}) if (fread(v->data(), sizeof(double), v->size(), f) != v->size()) return 2;
    fclose(f);
    ns::Opts o; bmpc_opts_for(N, o); o.start_rollout = 0;
    int rc = 0, runs = 0; double first = 0.0;
    for (int level = 0; level < 4; level++)
        for (int wo = 0; wo < (BMPC_NW > 1 ? 2 : 1); wo++)
            for (int pass = 0; pass < (level == 3 && BMPC_NW == 1 ? 2 : 1) && (levels >> level & 1) && rc == 0; pass++) {
                const int stages = pass == 0 ? N : 1;
                const bool ev = events && level >= 1, au = level >= 2, lg = level == 3;
                const bool want_th = BMPC_NW > 1 || level < 2;      // (one wave with the audit: traj_hist NULL, the other shape of that argument)
                std::vector<double> path(path0), ss(ss0), rb(rb0), rec(rec0);
                std::vector<double> p(141 + 91 * S), x0(44 * N), dual(57 * N + 2, 0.0), x(44 * N), g(43 * N), traj(TRN), hist((size_t)ticks * bmpcs::RH_LEN), th(want_th ? (size_t)ticks * TRN : 0),
                    tube(au ? (size_t)ticks * bmpcs::TUBE_LEN : 0), audit(au ? bmpcs::AUDIT_LEN : 0), log(lg && pass == 0 ? (size_t)ticks * (bmpcs::LOG_STAGE * stages + 4) : 0),
                    track(lg ? bmpcs::TRACK_LEN : 0);
                int iters = 0, status = 0, run = 0, info = -7, ran = -7; double kkt = 0.0;
                if (cap0 > 0) rc = EMU_STREAM_TICK(N, S, hd[2], &o, 1, path.data(), cap, ss.data(), rb.data(), p.data(), x0.data(), dual.data(), cap0, x.data(), g.data(), &iters,
                                                   &status, &kkt, traj.data(), 1, 1e-4, 0.0, 0.0, 0.0, 0.0, 0, wo);
                if (rc == 0) rc = bmpc_emu_stream_rollout(N, S, hd[2], &o, 1, ticks, path.data(), cap, ss.data(), rb.data(), p.data(), x0.data(), dual.data(), max_iter, x.data(),
                                                          g.data(), &iters, &status, &kkt, traj.data(), flags, hd[6], hist.data(), want_th ? th.data() : nullptr, &run, ev ? rec.data() : nullptr,
                                                          ev ? &rtick : nullptr, ev ? &info : nullptr, ev ? uflags : 0, ev ? dist.data() : nullptr, au ? tube.data() : nullptr,
                                                          au ? audit.data() : nullptr, 1e-6, lg && pass == 0 ? log.data() : nullptr, stages, lg ? track.data() : nullptr, 1e-4, 0.0,
                                                          0.0, 0.0, 0.0, 0, wo, level, -1, &ran);
                double sum = 0.0;
                for (int t = 0; t < run; t++) for (int i = 0; i < bmpcs::RH_LEN; i++) sum += hist[(size_t)t * bmpcs::RH_LEN + i];
                printf("%src %d ran %d order %d ticks_run %d of %d status %d iters %d phi %.17g phi_max %.17g checksum %.17g", runs ? " | " : "", rc, ran, wo, run, ticks, status, iters,
                       ss[bmpcs::SS_PHI], ss[bmpcs::SS_PHIMAX], sum);
                if (ev) printf(" replan_info %d flag %g", info, rec[bmpcs::RP_FLAG]);
                if (au) printf(" audit samples %g max_pos %.6g at %g max_rot %.6g at %g first_out %g", audit[bmpcs::AUDIT_SAMPLES], audit[bmpcs::AUDIT_MAX_POS],
                               audit[bmpcs::AUDIT_TICK_POS], audit[bmpcs::AUDIT_MAX_ROT], audit[bmpcs::AUDIT_TICK_ROT], audit[bmpcs::AUDIT_FIRST_OUT]);
                if (lg) printf(" stages %d track samples %g max_ep_orth %.6g at %g max_ep_par %.6g at %g max_er %.6g at %g replayed %g", stages, track[bmpcs::TRACK_SAMPLES],
                               track[bmpcs::TRACK_MAX_EP_ORTH], track[bmpcs::TRACK_TICK_EP_ORTH], track[bmpcs::TRACK_MAX_EP_PAR], track[bmpcs::TRACK_TICK_EP_PAR],
                               track[bmpcs::TRACK_MAX_ER], track[bmpcs::TRACK_TICK_ER], track[bmpcs::TRACK_REPLAYED]);
                if (runs++ == 0) first = sum;
                else if (rc == 0 && !(sum == first)) { printf(" DIFFERS"); rc = 3; }
            }
    printf("\n");
    return rc;
}
#endif
