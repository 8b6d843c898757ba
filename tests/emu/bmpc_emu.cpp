// TEST-ONLY lane emulator of the wave program (boundmpc_amd/csrc/bmpc_wave.inl), one wave per problem (BMPC_NW = 1, the default) or a team of
// BMPC_NW cooperating waves (-DBMPC_NW=4, -DBMPC_NW=2; with -DBMPC_WSG the pair of csrc/bmpc_pair.hip).
//
// Compiles the SAME kernel text with g++ and executes each phase as a loop over the 64 lanes in a caller-chosen order, a wide phase of a team
// as a loop over its waves in a caller-chosen order (bmpc_emu_host.h), and runs per problem the lines the kernel entries run: the argument
// record, the wave initialiser and the slicers of csrc/bmpc_args.h.  It exists so the kernel's indexing, phase structure and numerics can be
// unit-tested in a container without a GPU (pytest -m "not gpu"), and so that intra-phase cross-lane (and cross-wave) dependences show up as
// order-dependent results.  The fused tick is run as its kernel entry text (csrc/bmpc_tick_kernel.inl, both of its instantiations), launched as a
// loop over the blocks.  It is NOT part of the product: boundmpc_amd never builds, loads or falls back to it.
#include <cstring>
#include <cstdio>
#ifdef _OPENMP
#include <omp.h>
#endif

#ifndef BMPC_NW
#define BMPC_NW 1
#endif
#if BMPC_NW > 1
#define BMPC_NAMESPACE bmpct
#endif
#include "bmpc_emu_host.h"
namespace ns = BMPC_NAMESPACE;
typedef KArgsT<ns::Opts> KArgs;

#if BMPC_NW > 1
#define EMU_SOLVE bmpc_emu_team_solve
extern "C" int bmpc_emu_team_waves() { return BMPC_NW; }
extern "C" int bmpc_emu_team_lds_doubles() { return ns::L_SIZE; }
#else
#define EMU_SOLVE bmpc_emu_solve
#endif
// A batch of B problems, each on a workgroup of its own.  mode bit 0 (poison): LDS and workspace hold NaN before every problem (emu_wave).
// One wave: what the one-wave batch kernel and the restoration kernel behind it compute (bmpc_hip.hip bmpc_solve_kernel, bmpc_resto.hip).
// One wave with mode bit 1 (in-kernel): the solve of a fused tick on raw (p, x0) -- the instantiation the tick calls (real-time text, no deadline),
// with the restoration phase inside and only the outputs a tick has -- x, g, kkt, iters, status; x, g and status must be given.
// Teams: the multi-wave batch kernel's call (bmpc_multi_batch.inl) on the text with the restoration phase inside, as the fused team tick runs
// it; the team BATCH kernel hands jammed problems to the one-wave restoration kernel, which no emulator build runs behind a team.
extern "C" int EMU_SOLVE(int N, int S, double h, const ns::Opts *opts, int B, const double *p, const double *x0, double *state, double *x, double *g,
                         double *lam_g, double *lam_x, double *f, int *iters, int *status, double *kkt, int lane_order, int wave_order, int nthreads, int mode) {
    const bool poison = mode & 1, inkernel = mode & 2;
    if (!ns::emu_shape_ok(N, S) || (inkernel && (BMPC_NW > 1 || !x || !g || !status))) return 1;
    KArgs a = ns::emu_args(N, S, B, h, *opts);
    a.p = p; a.x0 = x0; a.state = state; a.x = x; a.g = g; a.lam_g = lam_g; a.lam_x = lam_x; a.f = f; a.iters = iters; a.status = status; a.kkt = kkt;
    const ns::Scr sc = ns::make_scr(N);
    const bool zl = ns::emu_zlds(N, S);
    BMPC_STRIDES(a);
#ifdef _OPENMP
    if (nthreads > 0) omp_set_num_threads(nthreads);
#endif
#if BMPC_NW == 1
    // The batch kernel leaves a jammed problem (internal status 4) with its iterate in x, and the restoration kernel continues it from there: for
    // both, x, iters and status are always there -- private ones here, copied to the caller's (where given) behind the hand-over.
    std::vector<double> xb((size_t)B * nw); std::vector<int> itb(B, 0), stb(B, 0);
    if (!inkernel) { a.x = xb.data(); a.iters = itb.data(); a.status = stb.data(); }
#endif
#pragma omp parallel
    {
        std::vector<double> lds(ns::L_SIZE, 0.0), scr(sc.size, 0.0);
#pragma omp for schedule(dynamic, 1)
        for (int b = 0; b < B; b++) {
            ns::Wave W = ns::emu_wave(a, lds, scr, lane_order, wave_order, poison);
#if BMPC_NW > 1
            BMPC_PROBLEM(pr, a, b);
            if (zl) ns::wave_solve_retry<true, false, true>(W, pr); else ns::wave_solve_retry<false, false, true>(W, pr);
#else
            if (inkernel) {
                BMPC_TICK_PROBLEM(pr, a, b, p + (size_t)b * np, x0 + (size_t)b * nw, state ? state + (size_t)b * (N * ns::NI + 2) : nullptr);
                if (zl) ns::wave_solve<true, true, true>(W, pr); else ns::wave_solve<false, true, true>(W, pr);
                continue;
            }
            BMPC_PROBLEM(pr, a, b);
            if (zl) ns::wave_solve_retry<true>(W, pr); else ns::wave_solve_retry<false>(W, pr);
            if (stb[b] == 4) {
                BMPC_RESTO_PROBLEM(rp, a, b, false);
                const std::vector<double> x0b(rp.x0, rp.x0 + nw); rp.x0 = x0b.data();      // (a copy: the lanes of a phase run one after the other here, and x is rewritten while x0 is still read)
                if (zl) ns::wave_solve_retry<true, false, true>(W, rp, BMPC_RESTO_X0_RETRY(a, b, false)); else ns::wave_solve_retry<false, false, true>(W, rp, BMPC_RESTO_X0_RETRY(a, b, false));
            }
            if (x) memcpy(x + (size_t)b * nw, pr.x, sizeof(double) * nw);
            if (iters) iters[b] = itb[b];
            if (status) status[b] = stb[b];
#endif
        }
    }
    return 0;
}

#ifndef BMPC_WSG      // (the pair has no stream kernels)
#include "../../boundmpc_amd/csrc/bmpc_stream.inl"
#include "../../boundmpc_amd/csrc/bmpc_tick_kernel.inl"

// ONE fused tick of B streams as the kernel entry text runs it: the arguments of bmpc_stream_tick (path [B][path_entries][48]), behind the option record
// and in front of what the handle holds (real-time tolerance, position-row cap, level rule) and the lane and wave orders.  Returns 1 where the C ABI
// returns BMPC_ERR_ARG (tick_args_ok).  The launch is a loop over the blocks 0 ... B -- one more than there are streams: that one meets the kernel's own
// guard -- on one workspace slab; the instantiation is chosen as bmpc_tick_launch / bmpc_team_launch_tick are called: the iterate in LDS by the horizon
// rule (teams: always), the restoration phase by the option record.  No clock here: no time budget.
#if BMPC_NW > 1
#define EMU_STREAM_TICK bmpc_emu_team_stream_tick
#else
#define EMU_STREAM_TICK bmpc_emu_stream_tick
#endif
extern "C" int EMU_STREAM_TICK(int N, int S, double h, const ns::Opts *opts, int B, const double *path, int path_entries, double *ss, double *rb, double *p, double *x0,
                               double *dual, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags, double rt_tol,
                               double rt_row_cap, double lvl_c, double lvl_lo, double lvl_hi, int lane_order, int wave_order) {
    if (!ns::emu_shape_ok(N, S) || B < 0 || max_iter < 0 || path_entries < S + 1 || N > bmpcs::STREAM_NMAX) return 1;
    if (B > 0 && (!path || !ss || !rb || !p || !x0 || !x || !g || !status || !traj)) return 1;
#if BMPC_NW > 1
    if (N > ns::TEAM_NMAX) return 1;      // (the library ticks such a horizon with one wave per stream)
#endif
    KArgs a = ns::emu_args(N, S, B, h, *opts);
    if (max_iter > 0) a.o.max_iter = max_iter;
    a.o.verbose = 0; a.o.retry_cap = 0;
    a.p = p; a.x0 = x0; a.state = dual; a.x = x; a.g = g; a.iters = iters; a.status = status; a.kkt = kkt;
    const SArgs s{path, path_entries * bmpcs::PT_LEN, ss, rb, traj, flags, rt_tol, rt_row_cap, lvl_c, lvl_lo, lvl_hi};
    std::vector<double> scr(ns::make_scr(N).size, 0.0);
    a.scratch = scr.data(); a.scr_stride = 0;
    const bool resto = a.o.restoration != 0;
    for (int b = 0; b <= B; b++) {
        emu_launch = EmuLaunch{b, B + 1, lane_order, wave_order};
#if BMPC_NW > 1
        if (resto) bmpc_team_tick_kernel<true>(a, s); else bmpc_team_tick_kernel<false>(a, s);
#else
        const bool zl = ns::emu_zlds(N, S);
        if (zl && resto) bmpc_stream_tick_kernel<true, true>(a, s);
        else if (zl) bmpc_stream_tick_kernel<true, false>(a, s);
        else if (resto) bmpc_stream_tick_kernel<false, true>(a, s);
        else bmpc_stream_tick_kernel<false, false>(a, s);
#endif
    }
    return 0;
}
#endif

// debug: ONE Newton direction at (x, t, nu, mu) with the regularisation delta, through the calls of wave_solve's Newton system in its order
// (evaluation, adjoint, row data, QP gradient, stage data, team_backward, wave_forward on wave 0, teams: wave_dz_wide) on the instantiation the
// solve entries choose.  Every wave program: one wave (any shape), teams and pairs (N <= TEAM_NMAX, S <= 4: their kernels' shapes).  Out: the gains
// kt [N][8][35], the feed-forward kf [N][8], the direction dz [N][44].  Returns 0, 3 (a stage block is not positive definite) or 1 (shape).
#if BMPC_NW > 1
#define EMU_NEWTON bmpc_emu_team_newton
#else
#define EMU_NEWTON bmpc_emu_newton
#endif
extern "C" int EMU_NEWTON(int N, int S, double h, const ns::Opts *opts, const double *p, const double *x, const double *t, const double *nu, double mu, double delta,
                          double *kt, double *kf, double *dz, int lane_order, int wave_order) {
    using namespace ns;
    if (!emu_shape_ok(N, S)) return 1;
    const bool zl = emu_zlds(N, S);
#if BMPC_NW > 1
    if (N > TEAM_NMAX || !zl) return 1;
#endif
    const Scr sc = make_scr(N); const POff po = make_poff_lds(S, L_ZL);
    std::vector<double> lds(L_SIZE, 0.0), scr(sc.size, 0.0);
    Wave W = emu_wave(emu_args(N, S, 1, h, *opts), lds, scr, lane_order, wave_order, true);      // (poisoned: the entry reads only what it wrote)
    double *L = W.L; const GPtr G = W.G; const LPtr WL = BMPC_WL(W);
    for (int i = 0; i < po.size; i++) L[L_PAR + (zl ? i : lds_index_of_p(S, i, L_ZL))] = p[i];
    wave_init_tables(W, po);
    W.Zc = zl ? L + L_ZL : (G + sc.Z).ptr(); W.Zt = zl ? L + L_PB : (G + sc.ZT).ptr(); W.Dz = zl ? L + L_PB + 512 : (G + sc.DZ).ptr();
    for (int i = 0; i < N * NZ; i++) W.Zc[i] = x[i];
    wave_eval(W, po, sc, W.Zc, sc.G, sc.HIN, false);
    BMPC_LANE_REGS(LRs);
    for (int i = 0; i < N * NI; i++) {      // row pass A of wave_solve on the caller's slacks and multipliers
        const double tt = t[i], nn = nu[i], ti = 1.0 / tt;
        WL[sc.T + i] = tt; WL[sc.NUm + i] = nn; WL[sc.SG + i] = nn * ti; WL[sc.TI + i] = ti; WL[sc.SR + i] = nn * ti * (WL[sc.HIN + i] + tt);
    }
    wave_adjoint(W, po, sc, sc.NUm, false, 0.0, LRs);
    wave_adjoint(W, po, sc, sc.NUm, true, mu, LRs);
    wave_stage_data_wide(W, po, sc);
    const bool ok = team_backward(W, po, sc, mu, delta, LRs);
    if (ok) {
        SOLO_BEGIN(0)
        wave_forward(W, sc, LRs);
        SOLO_END
        TEAM_SYNC();
#if BMPC_NW > 1
        wave_dz_wide(W, sc, LRs);
#endif
        for (int i = 0; i < N * NS * NU; i++) kt[i] = G[sc.KT + i];
        for (int i = 0; i < N * NU; i++) kf[i] = G[sc.KF + i];
        for (int i = 0; i < N * NZ; i++) dz[i] = W.Dz[i];
    }
    return ok ? 0 : 3;
}

#if BMPC_NW == 1
// CPU build of the stream functions (same text as the device kernels), one call per stream
extern "C" void bmpc_emu_stream_lengths(int N, int *out) { out[0] = bmpcs::PT_LEN; out[1] = bmpcs::ss_len(N); out[2] = bmpcs::RB_LEN; out[3] = bmpcs::tr_len(N); }
extern "C" void bmpc_emu_stream_pack(int N, int S, const double *path, double *ss, const double *rb, double *p, double *x0, double *dual, const double *xlast, double lvl_c, double lvl_lo, double lvl_hi) {
    double sh[bmpcs::SH_LEN];
    bmpcs::stream_pack(N, S, path, (int)ss[bmpcs::SS_NENT], ss, rb, p, x0, dual, xlast, sh, 0, 1, lvl_c, lvl_lo, lvl_hi);
}
extern "C" void bmpc_emu_stream_post(int N, int S, double h, const double *path, double *ss, double *rb, const double *x, const double *g, int status,
                                     double *traj, int simulate, double rt_tol, double rt_row_cap) {
    double sh[bmpcs::SH_LEN];
    bmpcs::stream_post(N, S, h, path, (int)ss[bmpcs::SS_NENT], ss, rb, x, g, status, traj, simulate, rt_tol, sh, 0, 1, rt_row_cap);
}

extern "C" void bmpc_emu_jacobian_lin_ddot(const double *q, const double *dq, const double *ddq, double *out) { bmpcs::jacobian_lin_ddot(q, dq, ddq, out); }
// fk_motion: out = [p 6 | v 6 | a 6 | jk 3]
extern "C" void bmpc_emu_fk_motion(const double *q, const double *dq, const double *ddq, const double *u, double *out) {
    bmpcs::FkMotion M; bmpcs::fk_motion(q, dq, ddq, u, M);
    for (int c = 0; c < 6; c++) { out[c] = M.p[c]; out[6 + c] = M.v[c]; out[12 + c] = M.a[c]; }
    for (int c = 0; c < 3; c++) out[18 + c] = M.jk[c];
}

extern "C" void bmpc_emu_sincos(int n, const double *x, double *s, double *c) { for (int i = 0; i < n; i++) bmpc::bmpc_sincos(x[i], s + i, c + i); }
// the library's horizon rule (csrc/bmpc_args.h): the option record of a handle of horizon N, its size, the longest short horizon
extern "C" void bmpc_emu_opts_for(int N, bmpc::Opts *o) { bmpc_opts_for(N, *o); }
extern "C" int bmpc_emu_opts_size() { return (int)sizeof(bmpc::Opts); }
extern "C" int bmpc_emu_short_nmax() { return BMPC_SHORT_NMAX; }
extern "C" int bmpc_emu_lds_doubles() { return bmpc::L_SIZE; }
extern "C" int bmpc_emu_scratch_doubles(int N) { return bmpc::make_scr(N).size; }
#endif
