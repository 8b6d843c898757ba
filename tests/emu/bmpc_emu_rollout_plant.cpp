// TEST-ONLY: CPU build of the rollout with a table of actuator models per stream (boundmpc_amd/csrc/bmpc_rollout_kernel.inl with PL), the same text the GPU
// kernels bmpc_stream_rollout_kernel<ZLDS, RESTO, true, true, true, 3> of bmpc_rollout_plant.hip and bmpc_team_rollout_plant.hip run, in the host's entry
// words (bmpc_emu_host.h), built once per BMPC_NW as its siblings are: one wave per stream (namespace bmpc) or a team of BMPC_NW waves (-DBMPC_NW=4,
// namespace bmpct).  One workgroup serves the B streams of a call, one after the other -- the kernel's own stride.  What the entry refuses and which
// level runs is the library's own rule (bmpc_rollout_level with entry 6, csrc/bmpc_args.h), the validity of a row is the library's own function
// (bmpc_plant_check, the same file), the step on its own is the library's own text (stream_plant, csrc/bmpc_stream_plant.inl), the instantiation is
// picked by the library's own piece (bmpc_rollout_run).  Used by tests/test_stream_rollout_plant.py and its GPU twin; never built, loaded or fallen back
// to by the product.
// With -DBMPC_EMU_ROLLOUT_PLANT_MAIN a stand-alone program for a sanitizer build (tests/emu/emu_rollout_plant.py run_sanitized, write_case).
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

extern "C" int bmpc_emu_rollout_plant_waves() { return BMPC_NW; }
// the kernel text's enums (tests: against the header's and stream.PLANT, PLANT_STATE, PLANT_REC): what = 0 row, 1 state, 2 record; k = -1: the length
extern "C" int bmpc_emu_plant_slot(int what, int k) {
    const int row[] = {bmpcpl::GAIN, bmpcpl::BIAS, bmpcpl::LAG, bmpcpl::SAT, bmpcpl::DELAY}, st[] = {bmpcpl::ST_ACT, bmpcpl::ST_CMD},
              rec[] = {bmpcpl::REC_SAMPLES, bmpcpl::REC_N_SAT, bmpcpl::REC_MAX_DU, bmpcpl::REC_TICK_DU, bmpcpl::REC_JOINT_DU, bmpcpl::REC_SUMSQ_DU};
    if (what == 0) return k == -1 ? bmpcpl::LEN : (k >= 0 && k < 5) ? row[k] : -1;
    if (what == 1) return k == -1 ? bmpcpl::ST_LEN : (k >= 0 && k < 2) ? st[k] : -1;
    if (what == 2) return k == -1 ? bmpcpl::REC_LEN : (k >= 0 && k < 6) ? rec[k] : -1;
    return -1;
}
// the compiled validity rule on one row: the mask the device stores in plant_info, and the row as resolved
extern "C" int bmpc_emu_plant_check(const double *row, double *used) { return bmpc_plant_check(row, used); }
// what bmpc_stream_plant does with ONE stream (in place): the mask of an invalid row (nothing touched), -1 for a stream without a plan (skipped), else 0
// behind the step; rec NULL or accumulated
extern "C" int bmpc_emu_stream_plant(int N, double h, double *rb, const double *ss, const double *row, double *state, double *rec, int tick) {
    const int bad = bmpc_plant_check(row, nullptr);
    if (bad) return bad;
    if (!(ss[bmpcs::SS_ERRCNT] < (double)N)) return -1;
    bmpcs::stream_plant(h, row, state, rb, rec, tick, 0, 1);
    return 0;
}
extern "C" void bmpc_emu_stream_plant_init(double *rec) { bmpcs::stream_plant_init(rec); }
// the tracking record over the log rows of ONE stream [T][row_len] (row_len = 88 stages + 4; a NaN row: a tick it did not run) and the using_previous word of
// every tick's trajectory record: the record text itself (stream_track_init, stream_track), for a loop that has the rows
extern "C" void bmpc_emu_stream_track_rows(int T, int row_len, const double *rows, const double *using_prev, double *track) {
    bmpcs::stream_track_init(track);
    for (int t = 0; t < T; t++) bmpcs::stream_track(rows + (size_t)t * row_len, rows[(size_t)t * row_len + row_len - 4], using_prev[t], track, t);
}

// B streams: the arguments of bmpc_stream_rollout_plant (path [B][cap][48]) behind the solver options, then what the handle holds (real-time tolerance,
// position-row cap, level rule), the lane and wave orders and *ran (may be NULL): the level that ran -- 6 with a plant table; without one what the sweeps
// entry runs on the same arguments.  Returns 1 where the C ABI returns BMPC_ERR_ARG (but for the time budget: no handle here) and for a horizon the teams
// do not take.
extern "C" int bmpc_emu_stream_rollout_plant(int N, int S, double h, const ns::Opts *opts, int B, int ticks, double *path, int cap, double *ss, double *rb, double *p, double *x0,
                                             double *dual, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags, double goal_tol,
                                             double *hist, double *traj_hist, int *ticks_run, double *replan, int *replan_info, int update_flags, const double *disturb,
                                             double *tube_hist, double *audit, double audit_tol, double *log_hist, int log_stages, double *track, int legs, const int *leg_tick,
                                             const int *leg_on, const double *leg_tol, int *legs_done, int *leg_fired, int *leg_why, const double *tune, int *tune_info,
                                             double *tune_used, const double *plant, double *plant_state, int *plant_info, double *plant_rec, double rt_tol, double rt_row_cap,
                                             double lvl_c, double lvl_lo, double lvl_hi, int lane_order, int wave_order, int *ran) {
    if (ran) *ran = -1;
    if (!ns::emu_shape_ok(N, S) || N > bmpcs::STREAM_NMAX || cap < S + 1 || max_iter < 0 || B < 1 || !path || !ss || !rb || !p || !x0 || !x || !g || !status || !traj) return 1;
#if BMPC_NW > 1
    if (N > ns::TEAM_NMAX || !ns::emu_zlds(N, S)) return 1;
#endif
    const RArgs r{ticks, goal_tol, hist, traj_hist, ticks_run, replan, nullptr, replan_info, update_flags, disturb, tube_hist, audit, audit_tol, log_hist, log_stages, track,
                  legs, leg_tick, leg_on, leg_tol, legs_done, leg_fired, leg_why, tune, tune_info, tune_used, plant, plant_state, plant_info, plant_rec};
    int level = bmpc_rollout_level(6, r, N, flags, rb);
    if (level == BMPC_ROLLOUT_REFUSED) return 1;
    if (BMPC_NW > 1 && level > 0 && level < 4) level = 3;      // (teams: one kernel with everything serves every level from 1 to 3)
    KArgs a = ns::emu_args(N, S, B, h, *opts);
    if (max_iter > 0) a.o.max_iter = max_iter;
    a.o.verbose = 0; a.o.retry_cap = 0;
    SArgs s{path, cap * bmpcs::PT_LEN, ss, rb, traj, flags, rt_tol, rt_row_cap, lvl_c, lvl_lo, lvl_hi};
    a.p = p; a.x0 = x0; a.state = dual; a.x = x; a.g = g; a.iters = iters; a.status = status; a.kkt = kkt;
    std::vector<double> scr(ns::make_scr(N).size, 0.0);
    a.scratch = scr.data(); a.scr_stride = (long long)scr.size();
    emu_launch = EmuLaunch{0, 1, lane_order, wave_order};      // one workgroup strides over the B streams
    const bool zl = ns::emu_zlds(N, S), resto = opts->restoration != 0;
    if (level == 6) bmpc_rollout_run<true, true, true, true, true, true>(zl, resto, &a, s, r, 1, 0);
    else if (level == 5) bmpc_rollout_run<true, true, true, true, true>(zl, resto, &a, s, r, 1, 0);
    else if (level == 4) bmpc_rollout_run<true, true, true, true>(zl, resto, &a, s, r, 1, 0);
    else if (level == 3) bmpc_rollout_run<true, true, true>(zl, resto, &a, s, r, 1, 0);
    else if (level == 0) bmpc_rollout_run<false, false, false>(zl, resto, &a, s, r, 1, 0);
#if BMPC_NW == 1
    else if (level == 1) bmpc_rollout_run<true, false, false>(zl, resto, &a, s, r, 1, 0);
    else if (level == 2) bmpc_rollout_run<true, true, false>(zl, resto, &a, s, r, 1, 0);
#endif
    else return 1;
    if (ran) *ran = level;
    return 0;
}

#ifdef BMPC_EMU_ROLLOUT_PLANT_MAIN
// case file (doubles): N S h B ticks cap flags goal_tol max_iter | path [B][cap][48] | ss | rb | p | x0 | dual | x | g | traj (each [B][its length]) | iters
// | status | kkt (each [B]) | plant [B][20] | plant_state [B][16] | disturb [ticks][B][21].  The batch is run once (teams: under wave orders 0 and 1) on
// fresh copies with every output array on, no queue and no settings table, the log rows of all N stages.  Every array is exactly as long as the kernel
// text may index it, so that an access outside is seen.  The runs of a case must agree.
template <class T>
static bool take(FILE *f, std::vector<T> &v, size_t n) {
    std::vector<double> d(n);
    if (fread(d.data(), sizeof(double), n, f) != n) return false;
    v.assign(d.begin(), d.end());
    return true;
}
int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s case.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    double hd[9];
    if (fread(hd, sizeof(double), 9, f) != 9) return 2;
    const int N = (int)hd[0], S = (int)hd[1], B = (int)hd[3], ticks = (int)hd[4], cap = (int)hd[5], flags = (int)hd[6], max_iter = (int)hd[8];
    const size_t TRN = bmpcs::tr_len(N), LR = (size_t)bmpcs::LOG_STAGE * N + 4, nb = (size_t)B;
    std::vector<double> path0, ss0, rb0, p0, x00, dual0, x0_, g0, traj0, kkt0, plant, pst0, dist;
    std::vector<int> iters0, status0;
    bool ok = take(f, path0, nb * cap * bmpcs::PT_LEN) && take(f, ss0, nb * bmpcs::ss_len(N)) && take(f, rb0, nb * bmpcs::RB_LEN) && take(f, p0, nb * (141 + 91 * S))
              && take(f, x00, nb * 44 * N) && take(f, dual0, nb * (57 * N + 2)) && take(f, x0_, nb * 44 * N) && take(f, g0, nb * 43 * N) && take(f, traj0, nb * TRN)
              && take(f, iters0, nb) && take(f, status0, nb) && take(f, kkt0, nb) && take(f, plant, nb * bmpcpl::LEN) && take(f, pst0, nb * bmpcpl::ST_LEN)
              && take(f, dist, (size_t)ticks * nb * bmpcs::DIST_LEN);
    fclose(f);
    if (!ok) return 2;
    ns::Opts o; bmpc_opts_for(N, o); o.start_rollout = 0;
    int rc = 0; double first = 0.0;
    for (int wo = 0; wo < (BMPC_NW > 1 ? 2 : 1) && rc == 0; wo++) {
        std::vector<double> path(path0), ss(ss0), rb(rb0), p(p0), x0(x00), dual(dual0), x(x0_), g(g0), traj(traj0), kkt(kkt0), pst(pst0), prec(nb * bmpcpl::REC_LEN, -7.0);
        std::vector<int> iters(iters0), status(status0), run(nb, -7), info(nb, -7);
        std::vector<double> hist((size_t)ticks * nb * bmpcs::RH_LEN), th((size_t)ticks * nb * TRN), tube((size_t)ticks * nb * bmpcs::TUBE_LEN), audit(nb * bmpcs::AUDIT_LEN),
            log((size_t)ticks * nb * LR), track(nb * bmpcs::TRACK_LEN);
        int ran = -7;
        rc = bmpc_emu_stream_rollout_plant(N, S, hd[2], &o, B, ticks, path.data(), cap, ss.data(), rb.data(), p.data(), x0.data(), dual.data(), max_iter, x.data(), g.data(),
                                           iters.data(), status.data(), kkt.data(), traj.data(), flags, hd[7], hist.data(), th.data(), run.data(), nullptr, nullptr, 3, dist.data(),
                                           tube.data(), audit.data(), 1e-6, log.data(), N, track.data(), 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                           nullptr, nullptr, plant.data(), pst.data(), info.data(), prec.data(), 1e-4, 0.0, 0.0, 0.0, 0.0, 0, wo, &ran);
        double sum = 0.0;
        for (int t = 0; t < ticks; t++) for (int b = 0; b < B; b++) if (t < run[b]) for (int i = 0; i < bmpcs::RH_LEN; i++) sum += hist[((size_t)t * nb + b) * bmpcs::RH_LEN + i];
        printf("%src %d ran %d order %d checksum %.17g", wo ? " | " : "", rc, ran, wo, sum);
        for (int b = 0; b < B; b++) printf(" [stream %d ticks_run %d plant_info %d samples %g n_sat %g]", b, run[b], info[b], prec[b * bmpcpl::REC_LEN + bmpcpl::REC_SAMPLES],
                                           prec[b * bmpcpl::REC_LEN + bmpcpl::REC_N_SAT]);
        if (wo == 0) first = sum;
        else if (rc == 0 && !(sum == first)) { printf(" DIFFERS"); rc = 3; }
    }
    printf("\n");
    return rc;
}
#endif
