// TEST-ONLY: CPU build of the rollout WITH A STATE OBSERVER (boundmpc_amd/csrc/bmpc_rollout_kernel.inl, the kernels bmpc_stream_rollout_observer_kernel<ZLDS,
// RESTO>: the loop text of bmpc_rollout_body.inl with SE and OB), the same text the GPU kernels of bmpc_rollout_observer.hip and
// bmpc_team_rollout_observer.hip run, in the host's entry words (bmpc_emu_host.h), beside bmpc_emu_rollout_sensor.cpp, which builds the sensor's kernels from
// the same lines.  Built once per BMPC_NW: one wave per stream (namespace bmpc) or a team of BMPC_NW waves (-DBMPC_NW=4, namespace bmpct).  One workgroup
// serves the B streams of a call, one after the other.  What the entry refuses is the library's own rule (bmpc_rollout_level with entry 6,
// bmpc_rollout_sensor_ok, bmpc_rollout_observer_ok; csrc/bmpc_args.h), the validity of a row the library's own function (bmpc_observer_check), the step on its
// own the library's own text (stream_observe; csrc/bmpc_stream_observer.inl) under the guards of the kernel of bmpc_rollout_observer.hip, the instantiation
// is picked by the library's own piece (bmpc_rollout_observer_run).  Without an observer table the entry IS the sensors': bmpc_rollout_sensor_run, or the
// level bmpc_rollout_level names through bmpc_rollout_run.
// Used by tests/test_stream_rollout_observer.py and its GPU twin; never built, loaded or fallen back to by the product.
// With -DBMPC_EMU_OBSERVER_MAIN a stand-alone program for a sanitizer build (tests/emu/emu_rollout_observer.py run_sanitized, write_case).
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

extern "C" int bmpc_emu_observer_waves() { return BMPC_NW; }
// the kernel text's enums (tests: against the header's and stream.OBSERVER, OBSERVER_STATE, OBSERVER_REC): what = 0 row, 1 state, 2 record; k = -1: the length
extern "C" int bmpc_emu_observer_slot(int what, int k) {
    const int row[] = {bmpcob::LQ, bmpcob::LDQ, bmpcob::LDDQ, bmpcob::LEAD, bmpcob::GATE}, st[] = {bmpcob::ST_POST, bmpcob::ST_JP, bmpcob::ST_JL, bmpcob::ST_HAS, bmpcob::ST_LAGS},
              rec[] = {bmpcob::REC_SAMPLES, bmpcob::REC_N_REJ, bmpcob::REC_MAX_DQ, bmpcob::REC_TICK_DQ, bmpcob::REC_JOINT_DQ, bmpcob::REC_MAX_DP, bmpcob::REC_TICK_DP, bmpcob::REC_SUMSQ_DQ};
    if (what == 0) return k == -1 ? bmpcob::LEN : k == -2 ? bmpcob::SLOTS : (k >= 0 && k < 5) ? row[k] : -1;
    if (what == 1) return k == -1 ? bmpcob::ST_LEN : (k >= 0 && k < 5) ? st[k] : -1;
    if (what == 2) return k == -1 ? bmpcob::REC_LEN : (k >= 0 && k < 8) ? rec[k] : -1;
    return -1;
}
// the library's records as this build lays them out (tests: against the ctypes mirrors): sizes, and the offset of a member of OArgs by name (-1: none)
extern "C" int bmpc_emu_observer_rargs_size() { return (int)sizeof(RArgs); }
extern "C" int bmpc_emu_observer_nargs_size() { return (int)sizeof(NArgs); }
extern "C" int bmpc_emu_oargs_size() { return (int)sizeof(OArgs); }
extern "C" int bmpc_emu_oargs_offset(const char *member) {
#define X(m) if (!strcmp(member, #m)) return (int)offsetof(OArgs, m);
    X(observer) X(observer_state) X(observer_info) X(observer_rec) X(sample_hist)
#undef X
    return -1;
}
// the compiled validity rule on one row: the mask the device stores in observer_info, and the row as resolved
extern "C" int bmpc_emu_observer_check(const double *row, double *used) { return bmpc_observer_check(row, used); }
extern "C" int bmpc_emu_rollout_observer_ok(const NArgs *n, const OArgs *o) { return bmpc_rollout_observer_ok(*n, *o) ? 1 : 0; }
extern "C" void bmpc_emu_stream_observer_init(double *rec) { bmpcs::stream_observer_init(rec); }
// what bmpc_stream_observe does with ONE stream (in place): -2 for an invalid sensor or observer row (nothing touched; the masks in *info and *oinfo), -1 for a
// stream without a plan (no sample, no estimate, SAME = 1), else 0 behind the estimate; noise [21] or NULL; rec, orec NULL or accumulated; meas [RB_LEN] or
// NULL; sample [21] or NULL
extern "C" int bmpc_emu_stream_observe(int N, double h, double *rb, const double *ss, const double *row, const double *noise, double *state, double *rec, double *meas, int tick,
                                       const double *orow, double *ostate, double *orec, double *sample, int *info, int *oinfo) {
    const int bad = bmpc_sensor_check(row, nullptr), obad = bmpc_observer_check(orow, nullptr);
    if (info) *info = bad;
    if (oinfo) *oinfo = obad;
    if (bad || obad) return -2;
    if (!(ss[bmpcs::SS_ERRCNT] < (double)N)) { state[bmpcse::ST_SAME] = 1.0; return -1; }
    bmpcs::stream_observe(h, row, noise, state, orow, ostate, rb, rec, orec, sample, tick, 0, 1);
    if (meas) for (int i = 0; i < bmpcs::RB_LEN; i++) meas[i] = rb[i];
    return 0;
}

// B streams: the arguments of bmpc_emu_stream_rollout_sensor (bmpc_emu_rollout_sensor.cpp) with the library's own OArgs record behind its NArgs; *ran (may be
// NULL): 8 where the observer kernels ran, 7 where the sensor kernels did, else the level of the text without a sensor that did.
// Returns 1 where the C ABI returns BMPC_ERR_ARG (but for the time budget: no handle here) and for a horizon the teams do not take.
extern "C" int bmpc_emu_stream_rollout_observer(int N, int S, double h, const ns::Opts *opts, int B, double *path, int cap, double *ss, double *rb, double *p, double *x0, double *dual,
                                                int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags, double rt_tol, double rt_row_cap,
                                                double lvl_c, double lvl_lo, double lvl_hi, int lane_order, int wave_order, int *ran, const RArgs *args, const NArgs *nargs,
                                                const OArgs *oargs) {
    if (ran) *ran = -1;
    if (!args || !nargs || !oargs || !ns::emu_shape_ok(N, S) || N > bmpcs::STREAM_NMAX || cap < S + 1 || max_iter < 0 || B < 1 || !path || !ss || !rb || !p || !x0 || !x || !g || !status || !traj) return 1;
#if BMPC_NW > 1
    if (N > ns::TEAM_NMAX || !ns::emu_zlds(N, S)) return 1;
#endif
    const RArgs &r = *args;
    if (r.replan_tick) return 1;      // (the entry has no such argument)
    int level = bmpc_rollout_level(6, r, N, flags, rb);
    if (level == BMPC_ROLLOUT_REFUSED || (nargs->sensor && !bmpc_rollout_sensor_ok(*nargs)) || !bmpc_rollout_observer_ok(*nargs, *oargs)) return 1;
    if (BMPC_NW > 1 && level > 0 && level < 4) level = 3;      // (teams: one kernel with everything serves every level from 1 to 3)
    KArgs a = ns::emu_args(N, S, 1, h, *opts);
    if (max_iter > 0) a.o.max_iter = max_iter;
    a.o.verbose = 0; a.o.retry_cap = 0;
    SArgs s{nullptr, 0, nullptr, nullptr, nullptr, 0, rt_tol, rt_row_cap, lvl_c, lvl_lo, lvl_hi};
    a.B = B; a.p = p; a.x0 = x0; a.state = dual; a.x = x; a.g = g; a.iters = iters; a.status = status; a.kkt = kkt;
    s.path = path; s.path_stride = cap * bmpcs::PT_LEN; s.ss = ss; s.rb = rb; s.traj = traj; s.flags = flags;
    std::vector<double> scr(ns::make_scr(N).size, 0.0);
    a.scratch = scr.data(); a.scr_stride = (long long)scr.size();
    emu_launch = EmuLaunch{0, 1, lane_order, wave_order};      // one workgroup strides over the B streams
    const bool zl = ns::emu_zlds(N, S), resto = opts->restoration != 0;
    if (oargs->observer) { bmpc_rollout_observer_run(zl, resto, &a, s, r, *nargs, *oargs, 1, 0); level = 8; }
    else if (nargs->sensor) { bmpc_rollout_sensor_run(zl, resto, &a, s, r, *nargs, 1, 0); level = 7; }
    else if (level == 6) bmpc_rollout_run<true, true, true, true, true, true>(zl, resto, &a, s, r, 1, 0);
    else if (level == 5) bmpc_rollout_run<true, true, true, true, true>(zl, resto, &a, s, r, 1, 0);
    else if (level == 4) bmpc_rollout_run<true, true, true, true>(zl, resto, &a, s, r, 1, 0);
    else if (level == 3) bmpc_rollout_run<true, true, true>(zl, resto, &a, s, r, 1, 0);
#if BMPC_NW == 1
    else if (level == 1) bmpc_rollout_run<true, false, false>(zl, resto, &a, s, r, 1, 0);
    else if (level == 2) bmpc_rollout_run<true, true, false>(zl, resto, &a, s, r, 1, 0);
#endif
    else return 1;
    if (ran) *ran = level;
    return 0;
}

#ifdef BMPC_EMU_OBSERVER_MAIN
// case file (doubles): N S h B ticks cap flags max_iter sections | path [B][cap][48] | ss | rb | p | x0 | dual | x | g | traj (each [B][its length]) | iters |
// status | kkt (each [B]) -- a batch behind its tick 0 -- | sensor [B][16] | sensor_state [B][64] | observer [B][8] | observer_state [B][40], then the sections
// `sections` names: bit 0 sensor_noise [ticks][B][21]; bit 1 the plant table [B][20] | plant_state [B][16]; bit 2 disturb [ticks][B][21].  The batch is run
// through the observer entry (teams: under wave orders 0 and 1, each on fresh copies) with every output array of the entry, each exactly as long as the kernel
// text may index it, so that an access outside is seen.  The runs of a case compute the same rows: their checksums must agree.  One line per case.
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
    double hd[9];
    if (fread(hd, sizeof(double), 9, f) != 9) return 2;
    const int N = (int)hd[0], S = (int)hd[1], B = (int)hd[3], ticks = (int)hd[4], cap = (int)hd[5], flags = (int)hd[6], max_iter = (int)hd[7], sec = (int)hd[8];
    enum { NOISE = 1, PLANT = 2, DIST = 4 };
    const size_t TRN = bmpcs::tr_len(N), nb = (size_t)B;
    std::vector<double> path0, ss0, rb0, p0, x00, dual0, x0_, g0, traj0, kkt0, sen, sst0, obs, ost0, noise, plant, pst0, dist;
    std::vector<int> iters0, status0;
    bool ok = take(f, path0, nb * cap * bmpcs::PT_LEN) && take(f, ss0, nb * bmpcs::ss_len(N)) && take(f, rb0, nb * bmpcs::RB_LEN) && take(f, p0, nb * (141 + 91 * S))
              && take(f, x00, nb * 44 * N) && take(f, dual0, nb * (57 * N + 2)) && take(f, x0_, nb * 44 * N) && take(f, g0, nb * 43 * N) && take(f, traj0, nb * TRN)
              && take(f, iters0, nb) && take(f, status0, nb) && take(f, kkt0, nb) && take(f, sen, nb * bmpcse::LEN) && take(f, sst0, nb * bmpcse::ST_LEN)
              && take(f, obs, nb * bmpcob::LEN) && take(f, ost0, nb * bmpcob::ST_LEN)
              && take(f, noise, (size_t)ticks * nb * bmpcs::DIST_LEN, sec & NOISE) && take(f, plant, nb * bmpcpl::LEN, sec & PLANT) && take(f, pst0, nb * bmpcpl::ST_LEN, sec & PLANT)
              && take(f, dist, (size_t)ticks * nb * bmpcs::DIST_LEN, sec & DIST);
    fclose(f);
    if (!ok) return 2;
    ns::Opts o; bmpc_opts_for(N, o); o.start_rollout = 0;
    int rc = 0, runs = 0; double first = 0.0;
    for (int wo = 0; wo < (BMPC_NW > 1 ? 2 : 1) && rc == 0; wo++) {
        std::vector<double> path(path0), ss(ss0), rb(rb0), p(p0), x0(x00), dual(dual0), x(x0_), g(g0), traj(traj0), kkt(kkt0), pst(pst0), sst(sst0), ost(ost0),
            prec(plant.empty() ? 0 : nb * bmpcpl::REC_LEN, -7.0), srec(nb * bmpcse::REC_LEN, -7.0), meas((size_t)ticks * nb * bmpcs::RB_LEN, -7.0),
            orec(nb * bmpcob::REC_LEN, -7.0), smp((size_t)ticks * nb * bmpcs::DIST_LEN, -7.0);
        std::vector<int> iters(iters0), status(status0), run(nb, -7), pinfo(plant.empty() ? 0 : nb, -7), sinfo(nb, -7), oinfo(nb, -7);
        std::vector<double> hist((size_t)ticks * nb * bmpcs::RH_LEN), th((size_t)ticks * nb * TRN), tube((size_t)ticks * nb * bmpcs::TUBE_LEN), audit(nb * bmpcs::AUDIT_LEN),
            log((size_t)ticks * nb * (bmpcs::LOG_STAGE * N + 4)), track(nb * bmpcs::TRACK_LEN);
        int ran = -7;
        RArgs r{ticks, 0.0, hist.data(), th.data(), run.data()};
        r.update_flags = 3; r.disturb = ptr(dist);
        r.tube_hist = tube.data(); r.audit = audit.data(); r.audit_tol = 1e-6; r.log_hist = log.data(); r.log_stages = N; r.track = track.data();
        r.plant = ptr(plant); r.plant_state = ptr(pst); r.plant_info = ptr(pinfo); r.plant_rec = ptr(prec);
        NArgs n{sen.data(), sst.data(), sinfo.data(), srec.data(), ptr(noise), meas.data()};
        OArgs oa{obs.data(), ost.data(), oinfo.data(), orec.data(), smp.data()};
        rc = bmpc_emu_stream_rollout_observer(N, S, hd[2], &o, B, path.data(), cap, ss.data(), rb.data(), p.data(), x0.data(), dual.data(), max_iter, x.data(), g.data(), iters.data(),
                                              status.data(), kkt.data(), traj.data(), flags, 1e-4, 0.0, 0.0, 0.0, 0.0, 0, wo, &ran, &r, &n, &oa);
        double sum = 0.0;
        for (int t = 0; t < ticks; t++) for (int b = 0; b < B; b++) if (t < run[b]) {
            for (int i = 0; i < bmpcs::RH_LEN; i++) sum += hist[((size_t)t * nb + b) * bmpcs::RH_LEN + i];
            for (int i = 0; i < bmpcs::RB_LEN; i++) sum += meas[((size_t)t * nb + b) * bmpcs::RB_LEN + i];
            for (int i = 0; i < bmpcs::DIST_LEN; i++) sum += smp[((size_t)t * nb + b) * bmpcs::DIST_LEN + i];
        }
        printf("%src %d ran %d order %d checksum %.17g", runs ? " | " : "", rc, ran, wo, sum);
        for (int b = 0; b < B; b++) printf(" [stream %d ticks_run %d sensor_info %d observer_info %d estimates %g rejected %g]", b, run[b], sinfo[b], oinfo[b],
                                           orec[b * bmpcob::REC_LEN + bmpcob::REC_SAMPLES], orec[b * bmpcob::REC_LEN + bmpcob::REC_N_REJ]);
        if (runs++ == 0) first = sum;
        else if (rc == 0 && !(sum == first)) { printf(" DIFFERS"); rc = 3; }
    }
    printf("\n");
    return rc;
}
#endif
