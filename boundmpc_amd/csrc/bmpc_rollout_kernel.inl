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
// SENSORS (the kernels bmpc_stream_rollout_sensor_kernel, SE; bmpc_stream_rollout_sensor; bmpc_rollout_sensor.hip, bmpc_team_rollout_sensor.hip;
// bmpc_stream_sensor.inl): a table n.sensor[b][bmpcse::LEN] of a measurement model per stream -- an encoder offset per joint, a quantisation step, noise on
// q, dq and ddq scaled from the caller's unit draws n.sensor_noise[t][b], a sample one tick old -- between the plant and what pack, solve and post of a
// tick read.  Every tick's pack reads the robot record, and the record IS the plant: the controller always measures the true state exactly, and a
// disturbance cannot stand in for a sensor -- it moves the plant, and the next pack measures the moved plant perfectly.  Here the record is the SAMPLE from
// stream_sense (behind the lost-plan test, ahead of the pack; the truth waits in n.sensor_state[b]) to stream_truth (behind the barrier behind
// stream_post, ahead of the plant step), and the TRUTH everywhere else: in hist[t][b], in the caller's robot array behind the launch, for the disturbance,
// the plant step, a spliced re-plan and a chained launch.  p, the audit row and the audit (taken from the pack's p), traj, the log and the tracking record
// describe the MEASUREMENT and the plan made from it -- what the controller's own monitor would report; n.meas_hist[t][b] is the record the pack of tick t
// read, and the record's largest ||p_m - p|| bounds what the audit's position excess can miss.  Where the sample equals the truth (SAME) the record keeps
// every bit and the post steps the truth itself: an identity row leaves what the plants' entry leaves.  Else the truth takes the post's step under the
// same planned jerk, or comes back as it was where the post exhausted the plan and did not step.  The barrier behind stream_truth is unconditional; EVERY
// wave of a team reads SAME and the error count itself, from words that do not change between the barrier ahead and the first barrier behind, wave 0 does
// the work.  The row is validated as a plant row is (bmpc_sensor_check; sensor_info, state untouched).  Row, state, record and noise live in global
// memory behind opaque stream and tick indices, and the members of n are read through the kernel-argument segment (BMPCR_SENSOR_ARGS): nothing of the
// sensor is carried in a register across the solve.  The SE kernels compile everything below them on and ask at run time whether there is a plant table.
// OBSERVERS (the kernels bmpc_stream_rollout_observer_kernel, OB; bmpc_stream_rollout_observer; bmpc_rollout_observer.hip, bmpc_team_rollout_observer.hip;
// bmpc_stream_observer.inl): a table o.observer[b][bmpcob::LEN] of a state estimator per stream -- a correction gain on q, dq and ddq, one step of lead for a
// sample that is one tick old, an innovation gate -- between the sensor's sample and the pack, which without it takes the noisy sample unfiltered.  The
// estimate is made in the lane-0 section of the sample (stream_observe in the place of stream_sense: the tick gains no barrier) and installed where the
// sample is installed; SAME of the sensor state is decided on the estimate, so the way back, the plant step, the rows and the events stay the lines they
// are.  n.meas_hist[t][b] is then the estimate's record, o.sample_hist[t][b] the raw sample, n.sensor_rec the sample against the truth and o.observer_rec
// the estimate against the truth.  The row is validated as a sensor row is (bmpc_observer_check; observer_info, both states untouched).  The observer does
// not see a disturbance, a spliced re-plan or a post that exhausted the plan: the innovation pulls it back, the state is not reset.  Row, state and
// record live in global memory behind opaque indices, the members of o are read through the kernel-argument segment (BMPCR_OBSERVER_FROM): nothing of
// the observer is carried in a register across the solve.
// The text of the stream and tick loops exists once, bmpc_rollout_body.inl; the kernels without a sensor expand it with BMPCR_SE 0 and hold no sensor line,
// those without an observer with BMPCR_OB 0 and hold no observer line.
// Written in the entry words of bmpc_gpu_common.h (BMPCK_*): g++ compiles the same text for the CPU tests (tests/emu/bmpc_emu_rollout.cpp:
// one source and one entry for every variant without a sensor, tests/emu/bmpc_emu_rollout_sensor.cpp for the sensor's, tests/emu/bmpc_emu_rollout_observer.cpp for the observer's, each built
// once per BMPC_NW).  The fifteen units (bmpc_rollout_observer.hip, bmpc_team_rollout_observer.hip, bmpc_rollout.hip,
// bmpc_rollout_events.hip, bmpc_rollout_audit.hip, bmpc_rollout_log.hip, bmpc_rollout_legs.hip, bmpc_rollout_tune.hip, bmpc_rollout_plant.hip, bmpc_rollout_sensor.hip,
// bmpc_team_rollout.hip, bmpc_team_rollout_legs.hip, bmpc_team_rollout_tune.hip, bmpc_team_rollout_plant.hip, bmpc_team_rollout_sensor.hip) and those builds launch through bmpc_rollout_run
// bmpc_rollout_sensor_run and bmpc_rollout_observer_run at the end of this file, the one place that picks <ZLDS, RESTO>.
#pragma once

#include "bmpc_stream_events.inl"
#include "bmpc_stream_plant.inl"
#include "bmpc_stream_sensor.inl"
#include "bmpc_stream_observer.inl"
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
// (SE) the members of the sensor kernels' fourth argument n, for the same reason read where they are consumed through the kernel-argument segment: it
// lies behind r at its natural alignment.  No sensor line names `n`.  In the TEAM kernels the pointer, and with BMPCR_SENSOR_IDX the stream and tick indices
// of the sensor lines, are made opaque in VECTOR registers: the members are then fetched by vector loads and every address the sensor lines form is vector
// arithmetic, between two solves, where vector registers are idle -- as scalars they were thirteen more scalar spills in the team kernels, whose spill
// registers then moved about at the join behind the tick loop (whole-wave copies, but the signature the build's ISA lint refuses).  The decisions taken from
// them are made scalar again (BMPCK_UNIFORM).  The one-wave kernels keep the scalar form of the plant lines: there it is the vector form that moves a spill
// register to a join inside the solve.  Both forms compute the same addresses; which one a unit takes is a matter of this toolchain's register allocation.
#ifndef BMPC_EMU
#define BMPCR_NARGS_AT ((BMPCR_RARGS_AT + sizeof(RArgs) + alignof(NArgs) - 1) / alignof(NArgs) * alignof(NArgs))
#if BMPC_NW > 1
#define BMPCR_SENSOR_IDX(i_) BMPCR_OPAQUE("+v"(i_))
#else
#define BMPCR_SENSOR_IDX(i_) BMPCR_OPAQUE("+s"(i_))
#endif
#define BMPCR_SENSOR_ARGS(na_) \
    const NArgs *na_; \
    { const char *k_ = (const char *)__builtin_amdgcn_kernarg_segment_ptr(); BMPCR_SENSOR_IDX(k_); na_ = (const NArgs *)(k_ + BMPCR_NARGS_AT); }
#else
#define BMPCR_SENSOR_ARGS(na_) const NArgs *na_ = &n
#define BMPCR_SENSOR_IDX(i_)
#endif
// (OB) the members of the observer kernels' fifth argument o, read the same way: it lies behind n at its natural alignment, and no observer line names
// `o`.  Every observer line sits in a block that has the sensor's pointer na_ (BMPCR_SENSOR_ARGS), and takes its own from it: one opaque pointer per block,
// in the sensor lines' form -- scalar on one wave, vector on teams, for the reasons written there.
#ifndef BMPC_EMU
#define BMPCR_OARGS_AT ((BMPCR_NARGS_AT + sizeof(NArgs) + alignof(OArgs) - 1) / alignof(OArgs) * alignof(OArgs))
#define BMPCR_OBSERVER_FROM(oa_, na_) const OArgs *oa_ = (const OArgs *)((const char *)(na_) + (BMPCR_OARGS_AT - BMPCR_NARGS_AT))
#else
#define BMPCR_OBSERVER_FROM(oa_, na_) const OArgs *oa_ = &o
#endif
// (the body of a tick in the kernel itself, as in bmpc_tick_kernel.inl: behind a function that takes `a` the argument loads lose their no-clobber
// property -- bmpc_args.h, BMPC_PROBLEM)
// (QT: the sixth argument counts what sits on top of the log -- 0 nothing, 1 the queue QU, 2 the queue and the table TU, 3 the queue, the table and the
// plant PL, each only ever compiled with everything below it on.  One argument for both keeps the kernels' mangled names at the length they had: tests/kernel_resources.py tells a team kernel
// from a one-wave kernel by the namespace inside the first 70 characters.)
template <bool ZLDS, bool RESTO, bool EV = false, bool AU = false, bool LG = false, int QT = 0>
BMPCK_KERNEL bmpc_stream_rollout_kernel(KArgs a, SArgs s, RArgs r) {
    constexpr bool QU = QT >= 1, TU = QT >= 2, PL = QT == 3;
#define BMPCR_SE 0
#define BMPCR_OB 0
#include "bmpc_rollout_body.inl"
#undef BMPCR_OB
#undef BMPCR_SE
}
// (SE: the same lines with the sensor's on, everything below it compiled on and the record of the sensor as a fourth argument; a kernel of its own, so
// that the one above keeps its three arguments and its instantiations the code they had)
template <bool ZLDS, bool RESTO>
BMPCK_KERNEL bmpc_stream_rollout_sensor_kernel(KArgs a, SArgs s, RArgs r, NArgs n) {
    constexpr bool EV = true, AU = true, LG = true, QU = true, TU = true, PL = true;
#define BMPCR_SE 1
#define BMPCR_OB 0
#include "bmpc_rollout_body.inl"
#undef BMPCR_OB
#undef BMPCR_SE
}
// (OB: the sensor kernel's lines with the observer's on and the record of the observer as a fifth argument; a kernel of its own, so that the two above
// keep their arguments and their instantiations the code they had)
template <bool ZLDS, bool RESTO>
BMPCK_KERNEL bmpc_stream_rollout_observer_kernel(KArgs a, SArgs s, RArgs r, NArgs n, OArgs o) {
    constexpr bool EV = true, AU = true, LG = true, QU = true, TU = true, PL = true;
#define BMPCR_SE 1
#define BMPCR_OB 1
#include "bmpc_rollout_body.inl"
#undef BMPCR_OB
#undef BMPCR_SE
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

// the same for the kernels with a sensor table (SE): one pair, or two, of instantiations per unit
template <class STREAM>
static void bmpc_rollout_sensor_run(bool zlds, bool resto, const void *kargs, const SArgs &s, const RArgs &r, const NArgs &n, int grid, STREAM st) {
    KArgs a; memcpy(&a, kargs, sizeof(a));
    if (zlds && resto) BMPCK_LAUNCH((bmpc_stream_rollout_sensor_kernel<true, true>), grid, st, a, s, r, n);
    else if (zlds) BMPCK_LAUNCH((bmpc_stream_rollout_sensor_kernel<true, false>), grid, st, a, s, r, n);
    else if constexpr (BMPC_NW == 1) {
        if (resto) BMPCK_LAUNCH((bmpc_stream_rollout_sensor_kernel<false, true>), grid, st, a, s, r, n);
        else BMPCK_LAUNCH((bmpc_stream_rollout_sensor_kernel<false, false>), grid, st, a, s, r, n);
    }
}

// the same for the kernels with an observer table (OB)
template <class STREAM>
static void bmpc_rollout_observer_run(bool zlds, bool resto, const void *kargs, const SArgs &s, const RArgs &r, const NArgs &n, const OArgs &o, int grid, STREAM st) {
    KArgs a; memcpy(&a, kargs, sizeof(a));
    if (zlds && resto) BMPCK_LAUNCH((bmpc_stream_rollout_observer_kernel<true, true>), grid, st, a, s, r, n, o);
    else if (zlds) BMPCK_LAUNCH((bmpc_stream_rollout_observer_kernel<true, false>), grid, st, a, s, r, n, o);
    else if constexpr (BMPC_NW == 1) {
        if (resto) BMPCK_LAUNCH((bmpc_stream_rollout_observer_kernel<false, true>), grid, st, a, s, r, n, o);
        else BMPCK_LAUNCH((bmpc_stream_rollout_observer_kernel<false, false>), grid, st, a, s, r, n, o);
    }
}
