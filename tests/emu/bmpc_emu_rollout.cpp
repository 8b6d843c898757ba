// TEST-ONLY: CPU build of the rollout (boundmpc_amd/csrc/bmpc_rollout_kernel.inl), the same text the GPU kernels bmpc_stream_rollout_kernel<ZLDS, RESTO,
// EV, AU, LG, QU, TU, PL> run, in the host's entry words (bmpc_emu_host.h: the stream functions with one lane on wave 0, the wave program inside with its
// phases as loops over the 64 lanes and, for a team, its wide phases as loops over the waves in a caller-chosen order).  One source for every variant and
// every C ABI entry (0 bmpc_stream_rollout, 1 _events, 2 _audit, 3 _log, 4 _legs, 5 _tuned, 6 _plant), built once per BMPC_NW as bmpc_emu.cpp is: one
// wave per stream (namespace bmpc; the seven levels of the one-wave units) or a team of BMPC_NW waves (-DBMPC_NW=4, namespace bmpct; level 0, the level
// with everything for 1 to 3, and 4 to 6).  One workgroup serves the B streams of a call, one after the other -- the kernel's own stride.  What the entry
// refuses and which level runs is the library's own rule (bmpc_rollout_level, csrc/bmpc_args.h), the validity of a settings or plant row is the library's
// own function (bmpc_tune_check, bmpc_plant_check, the same file), the plant step on its own is the library's own text (stream_plant,
// csrc/bmpc_stream_plant.inl), the instantiation is picked by the library's own piece (bmpc_rollout_run, bmpc_rollout_kernel.inl).
// Used by the tests/test_stream_*rollout*.py, tests/test_stream_tube.py and their GPU twins; never built, loaded or fallen back to by the product.
// With -DBMPC_EMU_ROLLOUT_MAIN a stand-alone program for a sanitizer build (tests/emu/emu_rollout.py run_sanitized, write_case; bmpc_emu.cpp with the
// same BMPC_NW is compiled beside this file for the tick text of tick 0).
#include <cmath>
#include <cstdio>
#include <cstddef>
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
extern "C" int bmpc_emu_leg_bits() { return bmpcs::LEG_AT_GOAL | bmpcs::LEG_ON_LOST << 4 | bmpcs::LEG_WHY_GOAL << 8 | bmpcs::LEG_WHY_LOST << 12 | bmpcs::LEG_WHY_TICK << 16; }
// slot k of the kernel text's row (tests: against the header's enum and stream.TUNE); k = -1: LEN, -2: the bit of the cross-slot test
extern "C" int bmpc_emu_tune_slot(int k) {
    const int slots[] = {bmpctu::MAX_ITER, bmpctu::TOL, bmpctu::MU_INIT, bmpctu::MU_WARM, bmpctu::MU_MIN_FAC, bmpctu::SLACK_PUSH, bmpctu::BOUND_MARGIN, bmpctu::HOLD,
                         bmpctu::LVL_C, bmpctu::LVL_LO, bmpctu::LVL_HI, bmpctu::RT_TOL, bmpctu::RT_ROW_CAP, bmpctu::STALL_WINDOW};
    return k == -1 ? bmpctu::LEN : k == -2 ? bmpctu::CROSS : (k >= 0 && k < bmpctu::SLOTS) ? slots[k] : -1;
}
// the kernel text's enums (tests: against the header's and stream.PLANT, PLANT_STATE, PLANT_REC): what = 0 row, 1 state, 2 record; k = -1: the length
extern "C" int bmpc_emu_plant_slot(int what, int k) {
    const int row[] = {bmpcpl::GAIN, bmpcpl::BIAS, bmpcpl::LAG, bmpcpl::SAT, bmpcpl::DELAY}, st[] = {bmpcpl::ST_ACT, bmpcpl::ST_CMD},
              rec[] = {bmpcpl::REC_SAMPLES, bmpcpl::REC_N_SAT, bmpcpl::REC_MAX_DU, bmpcpl::REC_TICK_DU, bmpcpl::REC_JOINT_DU, bmpcpl::REC_SUMSQ_DU};
    if (what == 0) return k == -1 ? bmpcpl::LEN : (k >= 0 && k < 5) ? row[k] : -1;
    if (what == 1) return k == -1 ? bmpcpl::ST_LEN : (k >= 0 && k < 2) ? st[k] : -1;
    if (what == 2) return k == -1 ? bmpcpl::REC_LEN : (k >= 0 && k < 6) ? rec[k] : -1;
    return -1;
}
// the library's RArgs record as this build lays it out (tests: against its ctypes mirror, emu_rollout.RArgs): the size, and the offset of a member by name (-1: none)
#define EMU_RARGS_MEMBERS(X) \
    X(ticks) X(goal_tol) X(hist) X(traj_hist) X(ticks_run) X(replan) X(replan_tick) X(replan_info) X(update_flags) X(disturb) X(tube_hist) X(audit) X(audit_tol) X(log_hist) \
    X(log_stages) X(track) X(legs) X(leg_tick) X(leg_on) X(leg_tol) X(legs_done) X(leg_fired) X(leg_why) X(tune) X(tune_info) X(tune_used) X(plant) X(plant_state) \
    X(plant_info) X(plant_rec)
extern "C" int bmpc_emu_rargs_size() { return (int)sizeof(RArgs); }
extern "C" int bmpc_emu_rargs_offset(const char *member) {
#define X(m) if (!strcmp(member, #m)) return (int)offsetof(RArgs, m);
    EMU_RARGS_MEMBERS(X)
#undef X
    return -1;
}

// the launch's settings as the entry below reads them: the options with the cap of the launch, the handle's stream words
static void launch_settings(int N, int S, double h, const ns::Opts *opts, int max_iter, double rt_tol, double rt_row_cap, double lvl_c, double lvl_lo, double lvl_hi, KArgs &a, SArgs &s) {
    a = ns::emu_args(N, S, 1, h, *opts);
    if (max_iter > 0) a.o.max_iter = max_iter;
    a.o.verbose = 0; a.o.retry_cap = 0;
    s = SArgs{nullptr, 0, nullptr, nullptr, nullptr, 0, rt_tol, rt_row_cap, lvl_c, lvl_lo, lvl_hi};
}
// the compiled validity rule on one row against those settings: the mask the device stores in tune_info, and the row as resolved
extern "C" int bmpc_emu_tune_check(int N, const ns::Opts *opts, int max_iter, double rt_tol, double rt_row_cap, double lvl_c, double lvl_lo, double lvl_hi, const double *row,
                                   double *used) {
    KArgs a; SArgs s;
    launch_settings(N, 2, 0.1, opts, max_iter, rt_tol, rt_row_cap, lvl_c, lvl_lo, lvl_hi, a, s);
    return bmpc_tune_check(row, a.o, s, used);
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

// B streams: the tick arrays behind the solver options (path [B][cap][48]), then what the handle holds (real-time tolerance, position-row cap, level rule),
// the lane and wave orders, the C ABI entry this call stands for (0 to 6), a forced level (-1: the library's rule; else that instantiation on the same
// arguments, which looks at nothing above its level), *ran (may be NULL): the level that ran, and the library's own RArgs record: what the entry has no
// argument for must be 0 / NULL in it.  Teams hold levels 0 and 3 to 6 and run 3 for any level from 1 to 3, as the library does; a forced 1 or 2 is refused.
// Returns 1 where the C ABI returns BMPC_ERR_ARG (but for the time budget: no handle here) and for a horizon the teams do not take.
extern "C" int bmpc_emu_stream_rollout(int N, int S, double h, const ns::Opts *opts, int B, double *path, int cap, double *ss, double *rb, double *p, double *x0, double *dual,
                                       int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags, double rt_tol, double rt_row_cap,
                                       double lvl_c, double lvl_lo, double lvl_hi, int lane_order, int wave_order, int entry, int level, int *ran, const RArgs *args) {
    if (ran) *ran = -1;
    if (!args || !ns::emu_shape_ok(N, S) || N > bmpcs::STREAM_NMAX || cap < S + 1 || max_iter < 0 || B < 1 || !path || !ss || !rb || !p || !x0 || !x || !g || !status || !traj) return 1;
#if BMPC_NW > 1
    if (N > ns::TEAM_NMAX || !ns::emu_zlds(N, S)) return 1;
#endif
    const RArgs &r = *args;
    if (entry < 0 || entry > 6 || (entry < 1 && (r.replan || r.replan_info || r.disturb)) || ((entry < 1 || entry > 3) && r.replan_tick) || (entry < 2 && (r.tube_hist || r.audit))
        || (entry < 3 && (r.log_hist || r.track)) || (entry < 4 && (r.legs || r.leg_tick || r.leg_on || r.leg_tol || r.legs_done || r.leg_fired || r.leg_why))
        || (entry < 5 && (r.tune || r.tune_info || r.tune_used)) || (entry < 6 && (r.plant || r.plant_state || r.plant_info || r.plant_rec))) return 1;
    const int ruled = bmpc_rollout_level(entry, r, N, flags, rb);
    if (ruled == BMPC_ROLLOUT_REFUSED) return 1;
    if (BMPC_NW > 1 && (level == 1 || level == 2)) return 1;
    if (level < 0) level = (BMPC_NW > 1 && ruled > 0 && ruled < 4) ? 3 : ruled;      // (teams: one kernel with everything serves every level from 1 to 3)
    KArgs a; SArgs s;
    launch_settings(N, S, h, opts, max_iter, rt_tol, rt_row_cap, lvl_c, lvl_lo, lvl_hi, a, s);
    a.B = B; a.p = p; a.x0 = x0; a.state = dual; a.x = x; a.g = g; a.iters = iters; a.status = status; a.kkt = kkt;
    s.path = path; s.path_stride = cap * bmpcs::PT_LEN; s.ss = ss; s.rb = rb; s.traj = traj; s.flags = flags;
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

#ifdef BMPC_EMU_ROLLOUT_MAIN
// case file (doubles): N S h B ticks cap flags goal_tol max_iter update_flags sections levels tick0_cap replan_tick legs | path [B][cap][48] | ss | rb, then
// the sections `sections` names, in this order: bit 0 the other tick arrays p | x0 | dual | x | g | traj (each [B][its length]) | iters | status | kkt (each [B])
// -- a batch behind its tick 0; without them fresh arrays as a handle allocates them --, bit 1 ONE re-plan record per stream [B][replan_len], due behind
// replan_tick, or bit 2 a queue [B][legs][replan_len] | leg_tick | leg_on [B][legs] and with bit 3 | leg_tol [B][legs]; bit 4 the settings table [B][16];
// bit 5 the plant table [B][20] | plant_state [B][16]; bit 6 disturb [ticks][B][21].  The batch is run once per level named by the bits of `levels`, through
// the entry of that number (teams: under wave orders 0 and 1 each), every run on fresh copies: with tick0_cap > 0 tick 0 is solved with that cap by the
// fused tick's text (bmpc_emu.cpp), then `ticks` ticks with max_iter by the rollout's.  A run is given what its entry has an argument for and the file a
// section of, and every output array of that entry; on one wave level 3 runs twice: rows of all N stages with the tracking record, then the record alone
// (its stage-0 row in the kernel's own words).  Every array is exactly as long as the kernel text may index it, so that an access outside is seen;
// traj_hist is NULL at levels 2 and 3 on one wave (the other shape of that argument).  All runs of a case compute the same history rows: their checksums
// must agree.  One line per case: per run the words of the one stream (a case without section 0) or of every stream.
#if BMPC_NW > 1
#define EMU_STREAM_TICK bmpc_emu_team_stream_tick
#else
#define EMU_STREAM_TICK bmpc_emu_stream_tick
#endif
extern "C" int EMU_STREAM_TICK(int N, int S, double h, const ns::Opts *opts, int B, const double *path, int path_entries, double *ss, double *rb, double *p, double *x0,
                               double *dual, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags, double rt_tol,
                               double rt_row_cap, double lvl_c, double lvl_lo, double lvl_hi, int lane_order, int wave_order);
template <class T>
static bool take(FILE *f, std::vector<T> &v, size_t n, bool given = true) {
    std::vector<double> d(given ? n : 0);
    if (fread(d.data(), sizeof(double), d.size(), f) != d.size()) return false;
    v.assign(d.begin(), d.end());
    return true;
}
template <class T>
static T *ptr(std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }
int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s case.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    double hd[15];
    if (fread(hd, sizeof(double), 15, f) != 15) return 2;
    const int N = (int)hd[0], S = (int)hd[1], B = (int)hd[3], ticks = (int)hd[4], cap = (int)hd[5], flags = (int)hd[6], max_iter = (int)hd[8], uflags = (int)hd[9], sec = (int)hd[10],
              levels = (int)hd[11], cap0 = (int)hd[12], rtick = (int)hd[13], legs = (int)hd[14];
    enum { ARRAYS = 1, RECORD = 2, QUEUE = 4, TOL = 8, TUNE = 16, PLANT = 32, DIST = 64 };
    const bool batch = (sec & ARRAYS) != 0;
    const size_t TRN = bmpcs::tr_len(N), RL = bmpcs::replan_len(S, cap), nb = (size_t)B, Q = nb * legs;
    std::vector<double> path0, ss0, rb0, p0(nb * (141 + 91 * S)), x00(nb * 44 * N), dual0(nb * (57 * N + 2), 0.0), x0_(nb * 44 * N), g0(nb * 43 * N), traj0(nb * TRN), kkt0(nb, 0.0),
        rec0, tol, tune, plant, pst0, dist;
    std::vector<int> iters0(nb, 0), status0(nb, 0), ltick, lon;
    bool ok = take(f, path0, nb * cap * bmpcs::PT_LEN) && take(f, ss0, nb * bmpcs::ss_len(N)) && take(f, rb0, nb * bmpcs::RB_LEN);
    if (batch) ok = ok && take(f, p0, p0.size()) && take(f, x00, x00.size()) && take(f, dual0, dual0.size()) && take(f, x0_, x0_.size()) && take(f, g0, g0.size())
                    && take(f, traj0, traj0.size()) && take(f, iters0, nb) && take(f, status0, nb) && take(f, kkt0, nb);
    ok = ok && !((sec & RECORD) && (sec & QUEUE)) && take(f, rec0, (sec & QUEUE) ? Q * RL : nb * RL, sec & (RECORD | QUEUE)) && take(f, ltick, Q, sec & QUEUE)
         && take(f, lon, Q, sec & QUEUE) && take(f, tol, Q, sec & TOL) && take(f, tune, nb * bmpctu::LEN, sec & TUNE) && take(f, plant, nb * bmpcpl::LEN, sec & PLANT)
         && take(f, pst0, nb * bmpcpl::ST_LEN, sec & PLANT) && take(f, dist, (size_t)ticks * nb * bmpcs::DIST_LEN, sec & DIST);
    fclose(f);
    if (!ok) return 2;
    ns::Opts o; bmpc_opts_for(N, o); o.start_rollout = 0;
    int rc = 0, runs = 0; double first = 0.0;
    for (int level = 0; level < 7; level++)
        for (int wo = 0; wo < (BMPC_NW > 1 ? 2 : 1); wo++)
            for (int pass = 0; pass < (level == 3 && BMPC_NW == 1 ? 2 : 1) && (levels >> level & 1) && rc == 0; pass++) {
                const int stages = pass == 0 ? N : 1;
                const bool qu = level >= 4 && (sec & QUEUE), re = qu || (level >= 1 && level <= 3 && (sec & RECORD)), ev = level >= 1 && (re || (sec & DIST)), au = level >= 2,
                           lg = level >= 3, tu = level >= 5 && (sec & TUNE), pl = level >= 6 && (sec & PLANT);
                const bool want_th = BMPC_NW > 1 || level < 2 || level >= 4;      // (one wave with the audit or the log alone: traj_hist NULL, the other shape of that argument)
                std::vector<double> path(path0), ss(ss0), rb(rb0), p(p0), x0(x00), dual(dual0), x(x0_), g(g0), traj(traj0), kkt(kkt0), rec(rec0), pst(pst0),
                    used(tu ? nb * bmpctu::LEN : 0, -7.0), prec(pl ? nb * bmpcpl::REC_LEN : 0, -7.0);
                std::vector<int> iters(iters0), status(status0), run(nb, -7), rt(re && !qu ? nb : 0, rtick), info(re ? (qu ? Q : nb) : 0, -7), done(qu ? nb : 0, -7), fired(qu ? Q : 0, -7),
                    why(qu ? Q : 0, -7), tinfo(tu ? nb : 0, -7), pinfo(pl ? nb : 0, -7);
                std::vector<double> hist((size_t)ticks * nb * bmpcs::RH_LEN), th(want_th ? (size_t)ticks * nb * TRN : 0), tube(au ? (size_t)ticks * nb * bmpcs::TUBE_LEN : 0),
                    audit(au ? nb * bmpcs::AUDIT_LEN : 0), log(lg && pass == 0 ? (size_t)ticks * nb * (bmpcs::LOG_STAGE * stages + 4) : 0), track(lg ? nb * bmpcs::TRACK_LEN : 0);
                int ran = -7;
                if (cap0 > 0) rc = EMU_STREAM_TICK(N, S, hd[2], &o, B, path.data(), cap, ss.data(), rb.data(), p.data(), x0.data(), dual.data(), cap0, x.data(), g.data(), iters.data(),
                                                   status.data(), kkt.data(), traj.data(), 1, 1e-4, 0.0, 0.0, 0.0, 0.0, 0, wo);
                RArgs r{ticks, hd[7], hist.data(), ptr(th), run.data()};
                if (ev) { r.replan = re ? rec.data() : nullptr; r.replan_tick = ptr(rt); r.replan_info = ptr(info); r.update_flags = uflags; r.disturb = ptr(dist); }
                r.tube_hist = ptr(tube); r.audit = ptr(audit); r.audit_tol = 1e-6; r.log_hist = ptr(log); r.log_stages = stages; r.track = ptr(track);
                if (qu) { r.legs = legs; r.leg_tick = ltick.data(); r.leg_on = lon.data(); r.leg_tol = ptr(tol); r.legs_done = done.data(); r.leg_fired = fired.data(); r.leg_why = why.data(); }
                if (tu) { r.tune = tune.data(); r.tune_info = tinfo.data(); r.tune_used = used.data(); }
                if (pl) { r.plant = plant.data(); r.plant_state = pst.data(); r.plant_info = pinfo.data(); r.plant_rec = prec.data(); }
                if (rc == 0) rc = bmpc_emu_stream_rollout(N, S, hd[2], &o, B, path.data(), cap, ss.data(), rb.data(), p.data(), x0.data(), dual.data(), max_iter, x.data(), g.data(),
                                                          iters.data(), status.data(), kkt.data(), traj.data(), flags, 1e-4, 0.0, 0.0, 0.0, 0.0, 0, wo, level, -1, &ran, &r);
                double sum = 0.0;
                for (int t = 0; t < ticks; t++) for (int b = 0; b < B; b++) if (t < run[b]) for (int i = 0; i < bmpcs::RH_LEN; i++) sum += hist[((size_t)t * nb + b) * bmpcs::RH_LEN + i];
                printf("%src %d ran %d order %d", runs ? " | " : "", rc, ran, wo);
                if (!batch) printf(" ticks_run %d of %d status %d iters %d phi %.17g phi_max %.17g", run[0], ticks, status[0], iters[0], ss[bmpcs::SS_PHI], ss[bmpcs::SS_PHIMAX]);
                printf(" checksum %.17g", sum);
                if (!batch) {
                    if (re) printf(" replan_info %d flag %g", info[0], rec[bmpcs::RP_FLAG]);
                    if (au) printf(" audit samples %g max_pos %.6g at %g max_rot %.6g at %g first_out %g", audit[bmpcs::AUDIT_SAMPLES], audit[bmpcs::AUDIT_MAX_POS],
                                   audit[bmpcs::AUDIT_TICK_POS], audit[bmpcs::AUDIT_MAX_ROT], audit[bmpcs::AUDIT_TICK_ROT], audit[bmpcs::AUDIT_FIRST_OUT]);
                    if (lg) printf(" stages %d track samples %g max_ep_orth %.6g at %g max_ep_par %.6g at %g max_er %.6g at %g replayed %g", stages, track[bmpcs::TRACK_SAMPLES],
                                   track[bmpcs::TRACK_MAX_EP_ORTH], track[bmpcs::TRACK_TICK_EP_ORTH], track[bmpcs::TRACK_MAX_EP_PAR], track[bmpcs::TRACK_TICK_EP_PAR],
                                   track[bmpcs::TRACK_MAX_ER], track[bmpcs::TRACK_TICK_ER], track[bmpcs::TRACK_REPLAYED]);
                }
                for (int b = 0; b < B && batch; b++) {
                    printf(" [stream %d ticks_run %d", b, run[b]);
                    if (qu) {
                        printf(" legs_done %d fired", done[b]);
                        for (int k = 0; k < legs; k++) printf(" %d", fired[(size_t)b * legs + k]);
                        printf(" why");
                        for (int k = 0; k < legs; k++) printf(" %d", why[(size_t)b * legs + k]);
                        printf(" info");
                        for (int k = 0; k < legs; k++) printf(" %d", info[(size_t)b * legs + k]);
                    }
                    if (tu) printf(" tune_info %d iters %d", tinfo[b], iters[b]);
                    if (pl) printf(" plant_info %d samples %g n_sat %g", pinfo[b], prec[b * bmpcpl::REC_LEN + bmpcpl::REC_SAMPLES], prec[b * bmpcpl::REC_LEN + bmpcpl::REC_N_SAT]);
                    printf("]");
                }
                if (runs++ == 0) first = sum;
                else if (rc == 0 && !(sum == first)) { printf(" DIFFERS"); rc = 3; }
            }
    printf("\n");
    return rc;
}
#endif
