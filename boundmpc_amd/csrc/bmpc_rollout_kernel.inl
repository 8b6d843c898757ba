// bmpc_rollout_kernel.inl -- a ROLLOUT of closed-loop streams: `ticks` whole ticks {pack, solve, post} of every stream in ONE launch, one wave
// per stream (bmpc_rollout.hip: bmpc_stream_rollout_kernel<ZLDS, RESTO>).  Included after the wave program and the stream functions; the unit
// defines KArgs.
// A loop of fused ticks (bmpc_tick_kernel.inl) joins the whole grid once per tick: "a tick lasts as long as its slowest stream", so a batch of
// closed loops costs the sum over the ticks of the slowest stream's solve.  The streams of a batch are independent -- with the plant in the loop
// (flags bit 0) tick t + 1 of stream b needs only what tick t of stream b left behind -- so here every stream runs at its own pace and the batch
// costs the slowest stream's SUM.  Workgroup w serves streams w, w + grid, w + 2 grid, ... on workspace slab w: a plain stride (no queue word, no
// atomic, no reset kernel; the streams have comparable total work, and the result does not depend on scheduling), so any B is served.
// The body of a tick is the fused tick's, line for line, with the same arguments (xlast = x under flags bit 1, no time budget, no second attempt);
// what one tick stores -- ss, rb, x, the dual state -- the pack of the next one reads back from global memory behind a workgroup barrier, the
// hand-over the fused tick already uses between its own three steps (p, x0 -> solver -> x, g -> post).
// Behind every tick's post the stream's history row is written; the stop rules of the node's loop are applied per stream:
//   lost plan   ss[SS_ERRCNT] >= N at the start of a tick: what the fused tick writes for a skipped stream (status 3, iters 0, kkt 0) is written
//               once, everything else keeps its last value, the stream stops;
//   goal        goal_tol > 0 and phi_max - phi <= goal_tol behind a post (NodeLoop.run, the reference's experiment runners): the stream stops.
// The history rows of the ticks a stream did not run are NaN.  With goal_tol = 0 every tick array holds afterwards what `ticks` launches of the
// one-wave fused tick leave, bit for bit.
// EVENTS (the instantiations with EV, bmpc_stream_rollout_events; bmpc_stream_events.inl, bmpc_stream_update.inl): behind the history rows of tick t
// and ahead of the goal test, the plant of a stream may be disturbed (r.disturb[t][b]) and, behind tick r.replan_tick[b], the stream re-planned from
// its record, the measured state spliced in on the device -- what only the device knows inside a rollout.  The goal test and the next tick's lost-plan
// test see what the re-plan left: a new phi_max lets a stream that has reached its old goal go on (a second leg), an error count back at N - 1
// rescues a stream whose plan the post has just exhausted.  A stream that stops first never consumes its record.  With goal_tol = 0 the arrays hold
// what the loop {one-wave fused tick, bmpc_stream_disturb, bmpc_stream_update of the records due} leaves, bit for bit.  Without EV no event line is
// compiled and the kernels are the ones from before the events.
// AUDIT (the instantiations with AU, bmpc_stream_rollout_audit; bmpc_stream_tube.inl): behind the pack of tick t and its barrier the tube row of the
// stream's p -- the state tick t STARTS from: the plant behind tick t - 1 with that tick's disturbance and re-plan applied, what a host loop measures
// on the p of every tick -- goes to r.tube_hist[t][b] and into the stream's record r.audit[b].  The record lives in global memory and the row in
// global memory or LDS: nothing of the audit is carried in a register across the solve.  Without AU no audit line is compiled.
// LOG (the instantiations with LG, bmpc_stream_rollout_log; bmpc_stream_log.inl): behind the post of tick t and its barrier, beside the history rows and
// AHEAD of that tick's events -- a disturbance changes rb, a re-plan rewrites the path table and the state row --, the logging record of the tick: what
// bmpc_stream_log writes when it is called right behind bmpc_stream_tick, cut to its first r.log_stages stages, to r.log_hist[t][b]; stage 0 of it, the
// state the plant is in behind the tick in the path frame, goes into the stream's tracking record r.track[b].  The window exists on the device only: the
// next pack overwrites p.  The record lives in global memory and the row in global memory or (without log_hist: stage 0 alone) in LDS, behind the log's
// own LDS words: nothing of the log is carried in a register across the solve.  Without LG no log line is compiled.
// TEAMS (bmpc_team_rollout.hip: BMPC_NW waves per stream, namespace bmpct, ZLDS always): the same text, as bmpc_tick_kernel.inl serves a team -- wave 0
// runs the stream functions and stores the rows, the workgroup solves, BMPCK_SYNC is a workgroup barrier.  The tick loop holds those barriers and
// leaves through data-dependent exits (lost plan, goal, replan_tick[b] == t), so all waves must take every exit together: each wave reads every
// such decision itself from memory that does not change between the last barrier ahead of the read and the first barrier behind it -- ss[SS_ERRCNT],
// ss[SS_PHI], ss[SS_PHIMAX] (written by wave 0 in stream_post and stream_update, each followed by a barrier; the only word of ss the next pack writes
// is SS_SECTOR, and the post behind it sits behind the solve's barriers, which need every wave), r.replan_tick (never written), under QU the trigger
// arrays (never written) and r.legs_done[b] (written by wave 0 at the start of the stream and ahead of the barrier behind stream_update), and the kernel
// arguments.  No decision is taken from a value that only wave 0 holds.
// MISSIONS (the instantiations with QU, bmpc_stream_rollout_legs; bmpc_rollout_legs.hip, bmpc_team_rollout_legs.hip): in the place of the one scheduled
// re-plan a QUEUE of r.legs records per stream, r.replan[b][k], each with a trigger -- a tick number (at or after it), the goal of the leg the stream
// is on (phi_max - phi <= its own tolerance), the lost plan (the post of this tick exhausted it) --, facts of the stream's own state that only the
// device knows and that every stream meets on another tick.  Only the head of the queue, record r.legs_done[b], can fire, at most one record per tick,
// where the single re-plan sits: behind the tick's rows and disturbance, ahead of the goal test and of the next tick's lost-plan test, so a
// goal-triggered record gives the stream its next phi_max before the goal test sees the old one, and an on-lost record rescues the stream.  The head
// lives in memory (it IS the output legs_done), not in a register: nothing of the queue is carried across the solve, and on a team every wave reads the
// same word behind a barrier.  Without QU no queue line is compiled and the kernels are the ones from before.
// SWEEPS (the instantiations with TU, bmpc_stream_rollout_tuned; bmpc_rollout_tune.hip, bmpc_team_rollout_tune.hip): a table r.tune[b][bmpctu::LEN] of
// controller settings per stream -- iteration cap, tolerance, barrier start and hold, level rule, acceptance threshold and position-row cap, joint-limit
// margin, stall window --, every slot NaN ("the launch's value") or a value that replaces, for every tick of stream b and nothing else, what `a.o` and `s`
// carry for the whole launch: a grid over settings is one launch of as many streams, not as many handles.  The table lives on the device, so a row is
// validated here, once per stream ahead of its tick loop, by the rule the host states (bmpc_tune_check, bmpc_args.h): a row with an invalid slot does
// not run -- no tick, no status word, NaN history rows, its mask in r.tune_info[b] -- and no stream ever runs on a default it did not ask for.  EVERY
// wave of a team takes that decision itself, from the read-only table and the kernel arguments.  A valid row is resolved AT EVERY TICK, three times, each
// where its words are consumed: the level rule onto a copy of the stream arguments ahead of the pack, the solver's words onto W.o behind BMPC_WAVE_INIT
// (which has just rebuilt it from a.o), the acceptance words onto a copy of the stream arguments ahead of the post.  Each is a handful of loads of a
// wave-uniform row made scalar (BMPCR_UNIFORM_F64), behind an opaque stream index: nothing of the table is carried in a register across the solve but
// what the solve itself reads, W.o, which it holds in any instantiation.  Without TU no tune line is compiled.
// PLANTS (the instantiations with PL, bmpc_stream_rollout_plant; bmpc_rollout_plant.hip, bmpc_team_rollout_plant.hip; bmpc_stream_plant.inl): a table
// r.plant[b][bmpcpl::LEN] of an actuator model per stream -- gain and offset per joint, a first-order lag, a clip, one tick of dead time -- between the
// first planned jerk of a tick and the plant, which without it IS the model: stream_post moves the robot record with the model's own chain and the
// planned jerk.  Such a plant responds to the command, and inside a rollout the command exists on the device only.  The step sits right behind the
// barrier behind stream_post, AHEAD of the history, trajectory and log rows and of the tick's disturbance and re-plan, and only where the post stepped
// the plant (ss[SS_ERRCNT] < N behind it, a word every wave reads there; the barrier behind the step is unconditional): hist[t][b] shows the TRUE plant
// behind tick t, a disturbance acts on it, a spliced re-plan takes it, the next pack and the audit row of tick t + 1 measure it.  The log and the
// tracking record keep describing the PLAN (stage 0 of traj is the plan's): the measurement of the plant is the audit.  The row is validated once per
// stream ahead of its tick loop by the rule the host states (bmpc_plant_check, bmpc_args.h), by EVERY wave from the read-only row; an invalid row gets the
// treatment of an invalid settings row -- no tick, NaN history rows, its mask in r.plant_info[b], plant_state untouched.  Row, state (r.plant_state[b],
// in and out: rollouts chain) and record (r.plant_rec[b]) live in global memory, behind opaque stream and tick indices: nothing of the plant is carried
// in a register across the solve.  Without PL no plant line is compiled.
// Written in the entry words of bmpc_gpu_common.h (BMPCK_*): g++ compiles the same text for the CPU tests (tests/emu/bmpc_emu_rollout.cpp:
// one source and one entry for every variant, built once per BMPC_NW).  The eleven units (bmpc_rollout.hip,
// bmpc_rollout_events.hip, bmpc_rollout_audit.hip, bmpc_rollout_log.hip, bmpc_rollout_legs.hip, bmpc_rollout_tune.hip, bmpc_rollout_plant.hip,
// bmpc_team_rollout.hip, bmpc_team_rollout_legs.hip, bmpc_team_rollout_tune.hip, bmpc_team_rollout_plant.hip) and those builds launch through bmpc_rollout_run at the end of this file, the
// one place that picks <ZLDS, RESTO>.
#pragma once

#include "bmpc_stream_events.inl"
#include "bmpc_stream_plant.inl"
#include "bmpc_stream_tube.inl"
#include "bmpc_stream_log.inl"

namespace bmpcs {
// trigger word of a queued re-plan record (BMPC_LEG_* of include/boundmpc_hip.h) and the conditions that held when it fired (BMPC_LEG_WHY_*)
enum { LEG_AT_GOAL = 1, LEG_ON_LOST = 2, LEG_WHY_GOAL = 1, LEG_WHY_LOST = 2, LEG_WHY_TICK = 4 };
// history row of one tick of one stream (BMPC_ROLL_* of include/boundmpc_hip.h): the robot record behind the post, then the named scalars, then the
// four trailer words of the tick's trajectory record
enum { RH_ROBOT = 0, RH_PHI = RB_LEN, RH_ERRCNT, RH_ITERS, RH_STATUS, RH_KKT, RH_NVALID, RH_USINGPREV, RH_SUCCESS, RH_GVIOL, RH_LEN };
}  // namespace bmpcs

// The tick loop must not become a reason to hoist: what the solver derives from the wave's and the problem's scalars (strides, table offsets, address
// arithmetic) is invariant over the ticks of a stream, and hoisted out of the loop it would stay live across the whole solve (the register pressure
// LANES_BEGIN guards against per phase).  Opaque per tick, the body allocates like the fused tick's.  Code generation of this kernel on the GPU only.
#ifndef BMPC_EMU
#define BMPCR_OPAQUE(...) asm volatile("" : __VA_ARGS__)
#define BMPCR_UNIFORM_F64(x) __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)))
#else
#define BMPCR_OPAQUE(...)
#define BMPCR_UNIFORM_F64(x) (x)
#endif
// (TU) the row of stream b_ as wave-uniform scalars: every lane loads the same words of the read-only table, the first lane's go to scalar registers.
// Expanded where the words are consumed; the slots a site does not read are dead loads.
#define BMPCR_TUNE_ROW(tr_, b_) \
    double tr_[bmpctu::SLOTS]; \
    { const double *g_ = r.tune + (long long)(b_) * bmpctu::LEN; \
      _Pragma("unroll") for (int k_ = 0; k_ < bmpctu::SLOTS; k_++) tr_[k_] = BMPCR_UNIFORM_F64(g_[k_]); }
// (PL) the four plant members of r, read where they are consumed THROUGH THE KERNEL-ARGUMENT SEGMENT behind an opaque pointer, not as r.plant: the compiler
// loads every member of a by-value argument it names at the kernel's entry and keeps it -- eight more scalar registers spilled across the whole solve, which
// on the team kernel with the restoration phase is one more spill register than the file holds.  So the plant lines never name those members, and what they
// address is loaded behind the solve and dead before the next one, as the stream and tick indices are.  BMPCR_RARGS_AT: where r lies in the segment, the
// arguments in their order at their natural alignment (tests/kernel_resources.py reads the same offset from the code object's metadata).
#ifndef BMPC_EMU
#define BMPCR_RARGS_AT ((((sizeof(KArgs) + alignof(SArgs) - 1) / alignof(SArgs) * alignof(SArgs) + sizeof(SArgs)) + alignof(RArgs) - 1) / alignof(RArgs) * alignof(RArgs))
#define BMPCR_PLANT_ARGS(pa_) \
    const RArgs *pa_; \
    { const char *k_ = (const char *)__builtin_amdgcn_kernarg_segment_ptr(); BMPCR_OPAQUE("+s"(k_)); pa_ = (const RArgs *)(k_ + BMPCR_RARGS_AT); }
#else
#define BMPCR_PLANT_ARGS(pa_) const RArgs *pa_ = &r
#endif
// (the body of a tick in the kernel itself, as in bmpc_tick_kernel.inl: behind a function that takes `a` the argument loads lose their no-clobber
// property -- bmpc_args.h, BMPC_PROBLEM)
// (QT: the sixth argument counts what sits on top of the log -- 0 nothing, 1 the queue QU, 2 the queue and the table TU, 3 the queue, the table and the
// plant PL, each only ever compiled with everything below it on.  One argument for both keeps the kernels' mangled names at the length they had: tests/kernel_resources.py tells a team kernel
// from a one-wave kernel by the namespace inside the first 70 characters.)
template <bool ZLDS, bool RESTO, bool EV = false, bool AU = false, bool LG = false, int QT = 0>
BMPCK_KERNEL bmpc_stream_rollout_kernel(KArgs a, SArgs s, RArgs r) {
    constexpr bool QU = QT >= 1, TU = QT >= 2, PL = QT == 3;
    static_assert(BMPC_NW == 1 || ZLDS, "a team keeps the iterate in LDS");
    BMPCK_LDS double lds[BMPC_NAMESPACE::L_SIZE];
    BMPC_STRIDES(a);
    const int wv = BMPCK_WAVE;
    const bool w0 = BMPC_NW == 1 || wv == 0;      // the wave that runs the stream functions and stores the rows (a team: wave 0)
    double *sh = lds + BMPC_NAMESPACE::L_RED;
    static_assert(bmpcs::SH_LEN <= 6 * 64, "the stream functions' LDS words must fit into the solver's reduction area");
    static_assert(bmpcs::TUBE_LEN <= 6 * 64, "and so must a tube row");
    static_assert(bmpcs::LSH_LEN + bmpcs::LOG_STAGE + 4 <= 6 * 64, "and the log's LDS words with one stage row and its trailer behind them");
    const int TRN = bmpcs::tr_len(a.N);
    const double nan_ = __builtin_nan("");
    for (int b = BMPCK_BLOCK; b < a.B; b += BMPCK_GRID) {
        BMPC_STREAM_SLICES(a, s, b);
        long long busy = 0;      // counts of the 100 MHz clock spent in the stream's solves
        int t = 0;
        if (EV && !QU) { if (r.replan_info && BMPCK_LANE == 0) r.replan_info[b] = -1; }
        if (QU) {
            // (the head of the queue lives in memory, legs_done[b]: wave 0 writes it here and behind a consumed record, every wave reads it behind the
            // barrier of a tick's post; the per-record outputs start as "never")
            if (r.replan && w0 && BMPCK_LANE == 0) {
                r.legs_done[b] = 0;
                for (int k = 0; k < r.legs; k++) {
                    const long long q = (long long)b * r.legs + k;
                    if (r.replan_info) r.replan_info[q] = -1;
                    if (r.leg_fired) r.leg_fired[q] = -1;
                    if (r.leg_why) r.leg_why[q] = 0;
                }
            }
        }
        if (AU) { if (r.audit && BMPCK_LANE == 0) bmpcs::stream_audit_init(r.audit + (long long)b * bmpcs::AUDIT_LEN); }
        if (LG) { if (r.track && BMPCK_LANE == 0) bmpcs::stream_track_init(r.track + (long long)b * bmpcs::TRACK_LEN); }
        int bad = 0;      // (TU) the invalid slots of the stream's row: such a stream runs no tick
        if constexpr (TU) {
            // (every wave reads the row and the kernel arguments itself; lane 0 of wave 0 stores the mask and the row as resolved)
            if (r.tune) {
                const bool out_ = w0 && BMPCK_LANE == 0;
                bad = BMPCK_UNIFORM(bmpc_tune_check(r.tune + (long long)b * bmpctu::LEN, a.o, s, out_ && r.tune_used ? r.tune_used + (long long)b * bmpctu::LEN : nullptr));
                if (out_ && r.tune_info) r.tune_info[b] = bad;
            }
        }
        if constexpr (PL) {
            // (a PL kernel is launched with a table only -- bmpc_rollout_level --, so no line here asks whether there is one.  Every wave reads the row
            // itself; lane 0 of wave 0 stores the mask and starts the record)
            BMPCR_PLANT_ARGS(pl_);
            int b_ = b; BMPCR_OPAQUE("+s"(b_));
            const int pbad = BMPCK_UNIFORM(bmpc_plant_check(pl_->plant + (long long)b_ * bmpcpl::LEN, nullptr));
            if (w0 && BMPCK_LANE == 0) {
                if (pl_->plant_info) pl_->plant_info[b_] = pbad;
                if (pl_->plant_rec) bmpcs::stream_plant_init(pl_->plant_rec + (long long)b_ * bmpcpl::REC_LEN);
            }
            bad |= pbad;      // (an invalid plant row keeps the stream from running as an invalid settings row does: one word decides)
        }
        if (!TU || !bad) for (; t < r.ticks; t++) {
            // (the lost-plan test of the fused tick: BoundMPC.step() returns five Nones there and the reference node stops)
            if (BMPCK_UNIFORM((int)(ss[bmpcs::SS_ERRCNT] >= (double)a.N))) {
                if (BMPCK_LANE == 0) { a.status[b] = 3; if (a.iters) a.iters[b] = 0; if (a.kkt) a.kkt[b] = 0.0; }
                break;
            }
            int N_ = a.N, S_ = a.S;
            BMPCR_OPAQUE("+s"(N_), "+s"(S_));      // (what the stream functions are given)
            if constexpr (!TU) {
                if (w0) bmpcs::stream_pack(N_, S_, path, s.path_stride / bmpcs::PT_LEN, ss, rb, p, x0, dual, (s.flags & 2) ? a.x + (long long)b * nw : nullptr, sh, BMPCK_LANE, BMPCK_NL, s.lvl_c, s.lvl_lo, s.lvl_hi);
            } else {
                SArgs sp = s;      // (what the pack is given: the launch's level rule, or the stream's)
                if (r.tune) { int b_ = b; BMPCR_OPAQUE("+s"(b_)); BMPCR_TUNE_ROW(tr_, b_); bmpc_tune_sargs(tr_, sp); }
                if (w0) bmpcs::stream_pack(N_, S_, path, s.path_stride / bmpcs::PT_LEN, ss, rb, p, x0, dual, (s.flags & 2) ? a.x + (long long)b * nw : nullptr, sh, BMPCK_LANE, BMPCK_NL, sp.lvl_c, sp.lvl_lo, sp.lvl_hi);
            }
            BMPCK_SYNC();
            if (AU) {
                // (the stream and the tick opaque, as for the events: what the audit addresses is computed here and dead before the solve)
                int b_ = b, t_ = t;
                BMPCR_OPAQUE("+s"(b_), "+s"(t_), "+s"(N_), "+s"(S_));
                double *row = r.tube_hist ? r.tube_hist + ((long long)t_ * a.B + b_) * bmpcs::TUBE_LEN : sh;
                if (w0) bmpcs::stream_tube(N_, S_, p, nullptr, row, BMPCK_LANE, BMPCK_NL);      // (no state row: the lost-plan test has just passed)
                if (r.audit && BMPCK_LANE == 0) bmpcs::stream_audit(row, r.audit + (long long)b_ * bmpcs::AUDIT_LEN, t_, r.audit_tol);
                BMPCK_SYNC();      // the solver's reductions reuse the LDS words of the row
            }
            BMPC_WAVE_INIT(W, a, lds, a.scratch + (long long)BMPCK_BLOCK * a.scr_stride, wv); BMPCK_WAVE_HOOK(W);
            if constexpr (TU) { if (r.tune) { int b_ = b; BMPCR_OPAQUE("+s"(b_)); BMPCR_TUNE_ROW(tr_, b_); bmpc_tune_opts(tr_, W.o); } }      // (W.o has just been rebuilt from a.o)
            BMPC_TICK_PROBLEM(pr, a, b, p, x0, dual);
            BMPCR_OPAQUE("+s"(W.N), "+s"(W.S), "+s"(W.h), "+s"(W.G.b), "+s"(pr.p), "+s"(pr.x0), "+s"(pr.x), "+s"(pr.g), "+s"(pr.state));
            const long long t0_ = a.latency_us ? BMPC_NOW() : 0;
            BMPC_NAMESPACE::wave_solve<ZLDS, true, RESTO>(W, pr);
            BMPCK_SYNC();
            if (a.latency_us) busy += BMPC_NOW() - t0_;
            BMPCR_OPAQUE("+s"(N_), "+s"(S_));
            if constexpr (!TU) {
                if (w0) bmpcs::stream_post(N_, S_, a.h, path, s.path_stride / bmpcs::PT_LEN, ss, rb, pr.x, pr.g, a.status[b], traj, s.flags, s.rt_tol, sh, BMPCK_LANE, BMPCK_NL, s.rt_row_cap);
            } else {
                SArgs sq = s;      // (what the post is given: the launch's acceptance words, or the stream's, loaded here, behind the solve)
                if (r.tune) { int b_ = b; BMPCR_OPAQUE("+s"(b_)); BMPCR_TUNE_ROW(tr_, b_); bmpc_tune_sargs(tr_, sq); }
                if (w0) bmpcs::stream_post(N_, S_, a.h, path, s.path_stride / bmpcs::PT_LEN, ss, rb, pr.x, pr.g, a.status[b], traj, s.flags, sq.rt_tol, sh, BMPCK_LANE, BMPCK_NL, sq.rt_row_cap);
            }
            BMPCK_SYNC();      // the history and the next pack read ss, rb, x, traj and the dual state that other lanes have just stored
            if constexpr (PL) {
                // The drive between the command the post has just stored and the plant it has just stepped: only where it did step it (every wave reads the
                // error count behind the post's barrier; the pack of the next tick does not write it).  The stream and the tick opaque, as for the events.
                BMPCR_PLANT_ARGS(pl_);
                int b_ = b, t_ = t;
                BMPCR_OPAQUE("+s"(b_), "+s"(t_));
                if (BMPCK_UNIFORM((int)(ss[bmpcs::SS_ERRCNT] < (double)N_))) {
                    if (w0) bmpcs::stream_plant(a.h, pl_->plant + (long long)b_ * bmpcpl::LEN, pl_->plant_state + (long long)b_ * bmpcpl::ST_LEN, rb,
                                                pl_->plant_rec ? pl_->plant_rec + (long long)b_ * bmpcpl::REC_LEN : nullptr, t_, BMPCK_LANE, BMPCK_NL);
                }
                BMPCK_SYNC();      // the rows, the events and the next pack read the TRUE plant
            }
            const long long row = (long long)t * a.B + b;
            if (r.hist && w0) {
                double *hr = r.hist + row * bmpcs::RH_LEN;
                for (int i = BMPCK_LANE; i < bmpcs::RB_LEN; i += BMPCK_NL) hr[bmpcs::RH_ROBOT + i] = rb[i];
                for (int i = BMPCK_LANE; i < 4; i += BMPCK_NL) hr[bmpcs::RH_NVALID + i] = traj[TRN - 4 + i];
                if (BMPCK_LANE == 0) {
                    hr[bmpcs::RH_PHI] = ss[bmpcs::SS_PHI]; hr[bmpcs::RH_ERRCNT] = ss[bmpcs::SS_ERRCNT]; hr[bmpcs::RH_STATUS] = (double)a.status[b];
                    hr[bmpcs::RH_ITERS] = nan_; hr[bmpcs::RH_KKT] = nan_;
                    if (a.iters) hr[bmpcs::RH_ITERS] = (double)a.iters[b];
                    if (a.kkt) hr[bmpcs::RH_KKT] = a.kkt[b];
                }
            }
            if (r.traj_hist && w0) { double *th = r.traj_hist + row * TRN; for (int i = BMPCK_LANE; i < TRN; i += BMPCK_NL) th[i] = traj[i]; }
            if (LG) {
                // (the stream and the tick opaque, as for the audit: what the log addresses is computed here, behind the solve, and dead before the next one)
                int b_ = b, t_ = t, cap_ = s.path_stride / bmpcs::PT_LEN;
                BMPCR_OPAQUE("+s"(b_), "+s"(t_), "+s"(cap_), "+s"(N_), "+s"(S_));
                // the row: the caller's, or stage 0 alone behind the log's own LDS words
                const int K_ = r.log_hist ? r.log_stages : 1;
                double *lrow = r.log_hist ? r.log_hist + ((long long)t_ * a.B + b_) * (K_ * bmpcs::LOG_STAGE + 4) : sh + bmpcs::LSH_LEN;
                if (w0) bmpcs::stream_log_rows<true>(N_, S_, a.h, path, cap_, ss, p, traj, lrow, K_, sh, BMPCK_LANE, BMPCK_NL);
                // (lane 0 wrote stage 0 and the trailer itself)
                if (r.track && BMPCK_LANE == 0) bmpcs::stream_track(lrow, lrow[K_ * bmpcs::LOG_STAGE], traj[TRN - 3], r.track + (long long)b_ * bmpcs::TRACK_LEN, t_);
                BMPCK_SYNC();      // the events and the next pack reuse the LDS words of the log
            }
            if (EV) {
                // (the stream and the tick opaque: what the events address is computed here, behind the solve, not carried across it)
                int b_ = b, t_ = t, cap_ = s.path_stride / bmpcs::PT_LEN;
                BMPCR_OPAQUE("+s"(b_), "+s"(t_), "+s"(cap_), "+s"(S_));
                if (r.disturb) {
                    if (w0) bmpcs::stream_disturb(rb, r.disturb + ((long long)t_ * a.B + b_) * bmpcs::DIST_LEN, BMPCK_LANE, BMPCK_NL);
                    BMPCK_SYNC();
                }
                if (!QU) {
                    if (r.replan && BMPCK_UNIFORM((int)(r.replan_tick[b_] == t_))) {
                        double *rec = r.replan + (long long)b_ * bmpcs::replan_len(S_, cap_);
                        if (r.update_flags & 2) { if (w0) bmpcs::stream_splice(a.h, S_, cap_, rec, rb, r.update_flags, BMPCK_LANE, BMPCK_NL); BMPCK_SYNC(); }
                        if (w0) bmpcs::stream_update(N_, S_, rec, const_cast<double *>(path), cap_, ss, rb, r.replan_info ? r.replan_info + b_ : nullptr, r.update_flags & 1,
                                             BMPCK_LANE, BMPCK_NL);
                        BMPCK_SYNC();      // the goal test, the lost-plan test and the next pack read what the re-plan stored
                    }
                } else if (r.replan) {
                    // The head record of the stream's queue, legs_done[b], and whether it is due behind this tick: EVERY wave decides for itself, from words
                    // that do not change between the barrier ahead (the post's, the log's or the disturbance's) and the first barrier behind the decision --
                    // the three ss words the stops read, the read-only trigger arrays, and legs_done[b], which wave 0 writes at the start of the stream and
                    // ahead of the last barrier of a consumed record.  Bit 0 of `why`: the record's goal, bit 1: the post of this tick exhausted the plan,
                    // bit 2: at or after its tick.  A word with an unknown bit, or without any condition, is never due: it ends the queue.
                    int L_ = r.legs;
                    BMPCR_OPAQUE("+s"(L_));
                    const int k_ = BMPCK_UNIFORM(r.legs_done[b_]);
                    int why_ = 0;
                    if (k_ < L_) {
                        const long long q_ = (long long)b_ * L_ + k_;
                        const int on_ = r.leg_on[q_], tk_ = r.leg_tick[q_];
                        const double tol_ = r.leg_tol ? r.leg_tol[q_] : r.goal_tol;
                        if (!(on_ & ~(bmpcs::LEG_AT_GOAL | bmpcs::LEG_ON_LOST))) {
                            if ((on_ & bmpcs::LEG_AT_GOAL) && ss[bmpcs::SS_PHIMAX] - ss[bmpcs::SS_PHI] <= tol_) why_ |= bmpcs::LEG_WHY_GOAL;
                            if ((on_ & bmpcs::LEG_ON_LOST) && ss[bmpcs::SS_ERRCNT] >= (double)a.N) why_ |= bmpcs::LEG_WHY_LOST;
                            if (tk_ >= 0 && t_ >= tk_) why_ |= bmpcs::LEG_WHY_TICK;
                        }
                    }
                    why_ = BMPCK_UNIFORM(why_);
                    if (why_) {
                        const long long q_ = (long long)b_ * L_ + k_;
                        double *rec = r.replan + q_ * bmpcs::replan_len(S_, cap_);
                        // (a barrier between the decision, which reads ss, and stream_update, which writes it: the splice's, or one of its own)
                        if (r.update_flags & 2) { if (w0) bmpcs::stream_splice(a.h, S_, cap_, rec, rb, r.update_flags, BMPCK_LANE, BMPCK_NL); }
                        BMPCK_SYNC();
                        // (every wave has read the head ahead of that barrier: it advances here, ahead of the barrier behind stream_update)
                        if (w0 && BMPCK_LANE == 0) {
                            if (r.leg_fired) r.leg_fired[q_] = t_;
                            if (r.leg_why) r.leg_why[q_] = why_;
                            r.legs_done[b_] = k_ + 1;
                        }
                        if (w0) bmpcs::stream_update(N_, S_, rec, const_cast<double *>(path), cap_, ss, rb, r.replan_info ? r.replan_info + q_ : nullptr, r.update_flags & 1,
                                             BMPCK_LANE, BMPCK_NL);
                        BMPCK_SYNC();      // the goal test, the lost-plan test, the next tick's head and the next pack read what the re-plan stored
                    }
                }
            }
            if (BMPCK_UNIFORM((int)(r.goal_tol > 0.0 && ss[bmpcs::SS_PHIMAX] - ss[bmpcs::SS_PHI] <= r.goal_tol))) { t++; break; }
        }
        // t ticks were run; the rows behind them stay without a tick
        for (int u = t; w0 && u < r.ticks; u++) {
            const long long row = (long long)u * a.B + b;
            if (r.hist) for (int i = BMPCK_LANE; i < bmpcs::RH_LEN; i += BMPCK_NL) r.hist[row * bmpcs::RH_LEN + i] = nan_;
            if (r.traj_hist) for (int i = BMPCK_LANE; i < TRN; i += BMPCK_NL) r.traj_hist[row * TRN + i] = nan_;
            if (AU) { if (r.tube_hist) for (int i = BMPCK_LANE; i < bmpcs::TUBE_LEN; i += BMPCK_NL) r.tube_hist[row * bmpcs::TUBE_LEN + i] = nan_; }
            if (LG) {
                const int LR = r.log_stages * bmpcs::LOG_STAGE + 4;
                if (r.log_hist) for (int i = BMPCK_LANE; i < LR; i += BMPCK_NL) r.log_hist[row * LR + i] = nan_;
            }
        }
        if (BMPCK_LANE == 0) {
            if (r.ticks_run) r.ticks_run[b] = t;
            if (a.latency_us) a.latency_us[b] = (double)busy * 0.01;
        }
        BMPCK_SYNC();      // the next stream's pack reuses the LDS words this stream's last phase read
    }
}

// Host: the one place that picks the instantiation <ZLDS, RESTO> of a unit's <EV, AU, LG, QU, TU, PL> (the kernel's sixth argument counts QU, TU and PL) and launches it on `grid` workgroups (BMPCK_LAUNCH: the GPU
// launch on stream `st`, or the host build's call).  kargs points at a KArgsT<...> record (the layouts are identical across instantiations).  A team
// keeps the iterate in LDS: its units hold no instantiation without ZLDS.  `static`: every unit has its own -- the name says nothing of the unit's KArgs
// and BMPC_NW, and the linker would fold the one-wave units' and the team unit's into one.
template <bool EV, bool AU, bool LG, bool QU = false, bool TU = false, bool PL = false, class STREAM>
static void bmpc_rollout_run(bool zlds, bool resto, const void *kargs, const SArgs &s, const RArgs &r, int grid, STREAM st) {
    static_assert((QU || !TU) && (TU || !PL), "the table sits on top of the queue, the plant on top of the table");
    constexpr int QT = PL ? 3 : TU ? 2 : QU ? 1 : 0;
    KArgs a; memcpy(&a, kargs, sizeof(a));
    if (zlds && resto) BMPCK_LAUNCH((bmpc_stream_rollout_kernel<true, true, EV, AU, LG, QT>), grid, st, a, s, r);
    else if (zlds) BMPCK_LAUNCH((bmpc_stream_rollout_kernel<true, false, EV, AU, LG, QT>), grid, st, a, s, r);
    else if constexpr (BMPC_NW == 1) {
        if (resto) BMPCK_LAUNCH((bmpc_stream_rollout_kernel<false, true, EV, AU, LG, QT>), grid, st, a, s, r);
        else BMPCK_LAUNCH((bmpc_stream_rollout_kernel<false, false, EV, AU, LG, QT>), grid, st, a, s, r);
    }
}

