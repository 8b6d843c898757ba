// bmpc_args.h -- the kernel argument records and what every kernel entry does with them: the wave of a workgroup from the argument head, and
// problem b of a batch as the wave program's Problem; at the end the argument rule of the rollout entries (host only).  Nothing of HIP in here: bmpc_gpu_common.h includes it for the kernels, and the CPU
// emulators of the kernel text (tests/emu) include it to run these very lines.  The macros name BMPC_NAMESPACE::Wave / Problem / make_gptr of the
// wave program (bmpc_wave.inl) and are expanded behind it.
#pragma once

// The horizon rule, once: horizons up to BMPC_SHORT_NMAX keep the iterate in LDS (with S <= SMAX_ZLDS) and run the first option set below,
// longer ones the second -- a cold start far from the solution wants a more central first barrier level and roomier slacks (the values of the
// barrier restart; 3-15 % fewer iterations than 0.3 / 1e-2 at N = 16..40), stalls are met by barrier restarts, so they are looked
// for earlier, the restoration phase follows a numerical breakdown only, and a solve that ends with status 2 gets a second attempt.
// bmpc_opts_for fills a WHOLE option record (OPTS = the Opts of a wave program's namespace) with the defaults of a handle of horizon N.
enum { BMPC_SHORT_NMAX = 11 };
template <class OPTS>
inline void bmpc_opts_for(int N, OPTS &o) {
    const bool lng = N > BMPC_SHORT_NMAX;
    o.tol = 1e-8; o.max_iter = 500; o.mu_init = lng ? 3.0 : 0.1; o.mu_min_fac = 0.1; o.slack_push = lng ? 0.1 : 1e-2; o.exact_hessian = 1; o.verbose = 0;
    o.mu_warm = 1e-2; o.stall_window = lng ? 20 : 40; o.bound_margin = 0.0;
    o.restoration = lng ? 2 : 1; o.resto_short = 6; o.resto_cap = 40; o.start_rollout = 1; o.hold_mu = 0; o.retry_cap = lng ? 100 : 0;
}

// The wave `W` of a workgroup from the argument head {N, S, h, o} of `a`, on the LDS array `lds` and the workspace slab `slab`; wave: its index in
// the workgroup (0 in a one-wave kernel).  A macro for the reason given at BMPC_PROBLEM.
#define BMPC_WAVE_INIT(W, a, lds, slab, wave) \
    BMPC_NAMESPACE::Wave W; W.N = (a).N; W.S = (a).S; W.h = (a).h; W.o = (a).o; W.L = (lds); \
    W.G = BMPC_NAMESPACE::make_gptr(slab); W.wv = (wave); W.deadline = 0; W.it_base = 0

// Problem `pr` = problem b of a batch kernel's arguments `a`: its slices of the inputs and of the outputs the caller passed (NULL stays NULL);
// np, nw, ng: the lengths of a problem's parameter, variable and constraint vectors (computed once, ahead of the kernel's work loop).
// A macro, expanded in the kernel body: the same lines as a function that takes `a` (by value or by reference) cost the argument loads their
// no-clobber property, and the register allocation of the whole kernel moves.
#define BMPC_STRIDES(a) const int np = 141 + 91 * (a).S, nw = (a).N * BMPC_NAMESPACE::NZ, ng = (a).N * BMPC_NAMESPACE::NG
#define BMPC_PROBLEM(pr, a, b) \
    BMPC_NAMESPACE::Problem pr; \
    pr.p = (a).p + (long long)(b) * np; pr.x0 = (a).x0 + (long long)(b) * nw; \
    pr.x = (a).x ? (a).x + (long long)(b) * nw : nullptr; pr.g = (a).g ? (a).g + (long long)(b) * ng : nullptr; \
    pr.lam_g = (a).lam_g ? (a).lam_g + (long long)(b) * ng : nullptr; pr.lam_x = (a).lam_x ? (a).lam_x + (long long)(b) * nw : nullptr; \
    pr.f = (a).f ? (a).f + (b) : nullptr; pr.kkt = (a).kkt ? (a).kkt + (b) : nullptr; \
    pr.iters = (a).iters ? (a).iters + (b) : nullptr; pr.status = (a).status ? (a).status + (b) : nullptr; \
    pr.state = (a).state ? (a).state + (long long)(b) * ((a).N * BMPC_NAMESPACE::NI + 2) : nullptr; \
    pr.resto_from = -1
// The restoration kernel's slicing (bmpc_resto.hip; its own, not BMPC_PROBLEM: x, iters and status are always there, and the shared lines with
// these overrides compile to another kernel).  fresh: an ordinary solve from x0; else the continuation of what a batch kernel left with status 4 --
// from the iterate it left in x (read before x is rewritten), counting on from its iterations.  BMPC_RESTO_X0_RETRY: the x0_retry argument of
// wave_solve_retry that goes with it (a continuation's second attempt is a fresh solve from the caller's x0).
#define BMPC_RESTO_PROBLEM(pr, a, b, fresh) \
    BMPC_NAMESPACE::Problem pr; \
    pr.p = (a).p + (long long)(b) * np; pr.x0 = ((fresh) ? (a).x0 : (a).x) + (long long)(b) * nw; \
    pr.x = (a).x + (long long)(b) * nw; pr.g = (a).g ? (a).g + (long long)(b) * ng : nullptr; \
    pr.lam_g = (a).lam_g ? (a).lam_g + (long long)(b) * ng : nullptr; pr.lam_x = (a).lam_x ? (a).lam_x + (long long)(b) * nw : nullptr; \
    pr.f = (a).f ? (a).f + (b) : nullptr; pr.kkt = (a).kkt ? (a).kkt + (b) : nullptr; \
    pr.iters = (a).iters + (b); pr.status = (a).status + (b); \
    pr.state = (a).state ? (a).state + (long long)(b) * ((a).N * BMPC_NAMESPACE::NI + 2) : nullptr; \
    pr.resto_from = (fresh) ? -1 : (a).iters[(b)]
#define BMPC_RESTO_X0_RETRY(a, b, fresh) ((fresh) ? nullptr : (a).x0 + (long long)(b) * nw)
// The fused tick's slicing (bmpc_tick_kernel.inl): p, x0 and the dual state are the ones the tick packed, x, g and status are always given, the
// multiplier outputs are not.
#define BMPC_TICK_PROBLEM(pr, a, b, p_, x0_, dual_) \
    BMPC_NAMESPACE::Problem pr; \
    pr.p = (p_); pr.x0 = (x0_); pr.x = (a).x + (long long)(b) * nw; pr.g = (a).g + (long long)(b) * ng; pr.lam_g = nullptr; pr.lam_x = nullptr; \
    pr.f = nullptr; pr.kkt = (a).kkt ? (a).kkt + (b) : nullptr; pr.iters = (a).iters ? (a).iters + (b) : nullptr; pr.status = (a).status + (b); \
    pr.state = (dual_); pr.resto_from = -1
// Stream b of a fused launch (tick, rollout): its path table, state, robot and trajectory records, packed problem and dual state (NULL stays NULL)
#define BMPC_STREAM_SLICES(a, s, b) \
    const double *path = (s).path + (long long)(b) * (s).path_stride; \
    double *ss = (s).ss + (long long)(b) * bmpcs::ss_len((a).N), *rb = (s).rb + (long long)(b) * bmpcs::RB_LEN, *traj = (s).traj + (long long)(b) * bmpcs::tr_len((a).N); \
    double *p = const_cast<double *>((a).p) + (long long)(b) * np, *x0 = const_cast<double *>((a).x0) + (long long)(b) * nw; \
    double *dual = (a).state ? (a).state + (long long)(b) * ((a).N * BMPC_NAMESPACE::NI + 2) : nullptr

// kernel arguments of a solve; OPTS = the Opts type of the wave program's namespace (same layout in every instantiation)
template <class OPTS>
struct KArgsT {
    int N, S, B; double h; OPTS o;
    const double *p, *x0; double *x, *g, *lam_g, *lam_x, *f, *kkt; int *iters, *status;
    double *state;           // optional [B][57 N + 2] dual state of a receding-horizon stream (bmpc_solve_batch_warm)
    double *latency_us;      // optional [B]: in-kernel duration of each solve (bmpc_set_latency_buffer)
    double *scratch; long long scr_stride; int *counter; unsigned long long *prof;
    long long budget_ticks;  // fused closed-loop tick only: time budget of a tick in counts of the 100 MHz wall clock, from kernel entry (0 = none)
    int *counter2, *rcount;  // restoration kernel (bmpc_resto.hip): its work queue; number of problems the batch kernel left with status 4 (NULL: phase off)
    const int *order;        // one-wave batch kernel: the work queue hands out order[0], order[1], ... instead of 0, 1, ... (NULL: natural order; bmpc_set_queue_order)
};
// kernel arguments of a service launch (bmpc_hip.hip bmpc_service_kernel): the head the wave needs, then the batch record of the job
template <class OPTS, class JOB>
struct ServiceArgsT {
    int N, S, B; double h; OPTS o; double *scratch; long long scr_stride;
    JOB job;
};
// stream arguments of a fused tick
struct SArgs {
    const double *path; int path_stride; double *ss, *rb, *traj; int flags; double rt_tol; double rt_row_cap; double lvl_c, lvl_lo, lvl_hi;
};
// what a rollout adds to the arguments of a fused tick (bmpc_rollout_kernel.inl): the ticks of every stream, the goal rule and the history
struct RArgs {
    int ticks; double goal_tol;      // goal_tol > 0: a stream stops behind the post that leaves phi_max - phi <= goal_tol
    double *hist, *traj_hist;        // [ticks][B][bmpcs::RH_LEN], [ticks][B][tr_len(N)]; either may be NULL
    int *ticks_run;                  // [B] or NULL
    // events behind a tick's post (the EV instantiations, bmpc_stream_rollout_events); NULL = off, what an initialiser of the members above leaves
    double *replan;                  // [B][replan_len]: the record of stream b is consumed behind tick replan_tick[b]
    const int *replan_tick;          // [B]; required with replan
    int *replan_info;                // [B] or NULL: -1 = not consumed, else the info of stream_update
    int update_flags;                // the flags of bmpc_stream_update: bit 0 set_goal, bit 1 splice, bit 2 poor bounds
    const double *disturb;           // [ticks][B][bmpcs::DIST_LEN]
    // audit of the state every tick starts from (the AU instantiations, bmpc_stream_rollout_audit); NULL = off
    double *tube_hist;               // [ticks][B][bmpcs::TUBE_LEN]
    double *audit;                   // [B][bmpcs::AUDIT_LEN], initialised by the kernel
    double audit_tol;                // an excess above it counts as outside a tube
    // logging records behind every tick's post and the tracking record over their stage 0 (the LG instantiations, bmpc_stream_rollout_log); NULL = off
    double *log_hist;                // [ticks][B][bmpcs::LOG_STAGE * log_stages + 4]
    int log_stages;                  // 1..N: the stages of the plan a row keeps
    double *track;                   // [B][bmpcs::TRACK_LEN], initialised by the kernel
    // a queue of re-plan records per stream in the place of the one scheduled record (the QU instantiations, bmpc_stream_rollout_legs): replan is
    // [B][legs][replan_len], replan_info [B][legs], replan_tick is not looked at; 0 / NULL = what an initialiser of the members above leaves
    int legs;                        // records per stream, >= 1 with replan
    const int *leg_tick, *leg_on;    // [B][legs]: the tick at or after which record k is due (negative: no tick condition); bit 0 at its goal, bit 1 on a lost plan
    const double *leg_tol;           // [B][legs] or NULL (goal_tol for every record): the goal tolerance of record k
    int *legs_done;                  // [B], initialised by the kernel: the head of the queue = the records consumed; required with replan
    int *leg_fired, *leg_why;        // [B][legs] or NULL: the tick behind which record k was consumed (-1: never), the conditions that held (0: never)
    // controller settings per stream (the TU instantiations, bmpc_stream_rollout_tuned): NULL = off, what an initialiser of the members above leaves
    const double *tune;              // [B][bmpctu::LEN]: row b replaces the launch's settings for every tick of stream b; a NaN slot keeps the launch's
    int *tune_info;                  // [B] or NULL: the mask of the invalid slots of row b (bit CROSS: the level rule as resolved); 0 = the stream ran
    double *tune_used;               // [B][bmpctu::LEN] or NULL: the row as resolved, pad words 0
    // an actuator model per stream between the command and the plant (the PL instantiations, bmpc_stream_rollout_plant): NULL = off, what an initialiser
    // of the members above leaves
    const double *plant;             // [B][bmpcpl::LEN]: row b stands between the first planned jerk of every tick of stream b and its plant; a NaN slot is the identity
    double *plant_state;             // [B][bmpcpl::ST_LEN], in and out: the lag's state and the previous command; required with plant
    int *plant_info;                 // [B] or NULL: the mask of the invalid slots of row b; 0 = the stream ran
    double *plant_rec;               // [B][bmpcpl::REC_LEN] or NULL, initialised by the kernel: what the plant did to the commands
};
// what a rollout with a measurement model adds (the SE kernels, bmpc_stream_rollout_sensor; bmpc_rollout_kernel.inl): a record of its own, the FOURTH
// kernel argument of those kernels -- RArgs keeps its members, and the kernels without a sensor their three arguments
struct NArgs {
    const double *sensor;            // [B][bmpcse::LEN]: row b stands between the plant of stream b and what pack, solve and post of every tick read; a NaN slot is the identity
    double *sensor_state;            // [B][bmpcse::ST_LEN], in and out: the held sample and the truth of a tick in flight; all zeros = fresh; required with sensor
    int *sensor_info;                // [B] or NULL: the mask of the invalid slots of row b; 0 = the stream ran
    double *sensor_rec;              // [B][bmpcse::REC_LEN] or NULL, initialised by the kernel: what the samples differed from the truth by
    const double *sensor_noise;      // [ticks][B][bmpcs::DIST_LEN] or NULL: unit draws, scaled by the row's NQ, NDQ, NDDQ; a non-finite word counts as 0
    double *meas_hist;               // [ticks][B][bmpcs::RB_LEN] or NULL: the robot record the pack of tick t read; NaN rows for the ticks not run
};
// what a rollout with a state observer adds (the OB kernels, bmpc_stream_rollout_observer; bmpc_rollout_kernel.inl): a record of its own, the FIFTH kernel
// argument of those kernels -- RArgs and NArgs keep their members, and the other kernels their arguments
struct OArgs {
    const double *observer;          // [B][bmpcob::LEN]: row b stands between the sample of stream b's sensor and the pack; a NaN slot is the identity
    double *observer_state;          // [B][bmpcob::ST_LEN], in and out: the last posterior and the jerks that advance it; all zeros = fresh; required with observer
    int *observer_info;              // [B] or NULL: the mask of the invalid slots of row b; 0 = the stream ran
    double *observer_rec;            // [B][bmpcob::REC_LEN] or NULL, initialised by the kernel: what the estimates differed from the truth by
    double *sample_hist;             // [ticks][B][bmpcs::DIST_LEN] or NULL: the raw sample the sensor handed the observer at tick t; NaN rows for the ticks not run
};

// ---- host and device: a row of per-stream controller settings (BMPC_TUNE_* of include/boundmpc_hip.h), what it resolves to and what is refused ----
// The slots of a row; a slot holds NaN ("the launch's value") or the value of the option, setter or argument named behind it.
namespace bmpctu {
enum { MAX_ITER = 0,      // Opts::max_iter                      (the launch's: the max_iter argument when > 0, else the handle's option)
       TOL,               // Opts::tol
       MU_INIT, MU_WARM, MU_MIN_FAC, SLACK_PUSH,      // the barrier start of Opts
       BOUND_MARGIN,      // Opts::bound_margin
       HOLD,              // Opts::hold_mu                       (bmpc_set_barrier_hold)
       LVL_C, LVL_LO, LVL_HI,      // SArgs::lvl_*               (bmpc_stream_set_level_rule)
       RT_TOL,            // SArgs::rt_tol                       (bmpc_stream_set_rt_feasibility_tol)
       RT_ROW_CAP,        // SArgs::rt_row_cap                   (bmpc_stream_set_rt_position_row_cap)
       STALL_WINDOW,      // Opts::stall_window
       SLOTS,             // the slots that are looked at; the words behind them up to LEN are pad
       LEN = 16, CROSS = 15 };      // CROSS: the bit of tune_info for the one test across slots
}
#define BMPC_TOL_MAX 1.7976931348623157e308      // the largest finite tolerance (plain comparisons: the flop-counting hosts of tests/emu read this file with their own number type)
#if defined(__HIPCC__)
#define BMPC_ARGS_HD __host__ __device__ inline
#else
#define BMPC_ARGS_HD inline
#endif
// the launch's own value of slot k: what a NaN slot resolves to
template <class OPTS>
BMPC_ARGS_HD double bmpc_tune_launch_value(int k, const OPTS &o, const SArgs &s) {
    switch (k) {
    case bmpctu::MAX_ITER: return (double)o.max_iter;
    case bmpctu::TOL: return o.tol;
    case bmpctu::MU_INIT: return o.mu_init;
    case bmpctu::MU_WARM: return o.mu_warm;
    case bmpctu::MU_MIN_FAC: return o.mu_min_fac;
    case bmpctu::SLACK_PUSH: return o.slack_push;
    case bmpctu::BOUND_MARGIN: return o.bound_margin;
    case bmpctu::HOLD: return (double)o.hold_mu;
    case bmpctu::LVL_C: return s.lvl_c;
    case bmpctu::LVL_LO: return s.lvl_lo;
    case bmpctu::LVL_HI: return s.lvl_hi;
    case bmpctu::RT_TOL: return s.rt_tol;
    case bmpctu::RT_ROW_CAP: return s.rt_row_cap;
    case bmpctu::STALL_WINDOW: return (double)o.stall_window;
    default: return 0.0;
    }
}
// THE validity rule of a slot that is not NaN, once: the test of bmpc_create or of the setter that guards the same value (plain comparisons; a cast to
// int only behind the range test that makes it defined).  NaN never gets here: it is "the launch's value".
BMPC_ARGS_HD bool bmpc_tune_slot_ok(int k, double v) {
    if (!(v >= -BMPC_TOL_MAX && v <= BMPC_TOL_MAX)) return false;      // (infinite)
    switch (k) {
    case bmpctu::MAX_ITER: return v >= 1.0 && v <= 100000.0 && (double)(int)v == v;
    case bmpctu::TOL: case bmpctu::MU_INIT: case bmpctu::MU_WARM: case bmpctu::MU_MIN_FAC: case bmpctu::SLACK_PUSH: case bmpctu::RT_TOL: return v > 0.0;
    case bmpctu::BOUND_MARGIN: return v >= 0.0 && v <= 0.5;
    case bmpctu::HOLD: return v == 0.0 || v == 1.0;
    case bmpctu::LVL_C: case bmpctu::LVL_LO: case bmpctu::LVL_HI: case bmpctu::RT_ROW_CAP: return v >= 0.0;
    case bmpctu::STALL_WINDOW: return v >= 0.0 && v <= 2147483646.0 && (double)(int)v == v && !((int)v & 1);
    default: return true;      // (pad words: never looked at)
    }
}
// Row `row` against the launch's settings {o, s}: the mask of its invalid slots, bit CROSS for the level rule AS RESOLVED (hi > 0 needs 0 < lo <= hi,
// the test of bmpc_stream_set_level_rule); 0 = the stream runs.  used (or NULL): the resolved row, a refused value as it was given, pad words 0.
template <class OPTS>
BMPC_ARGS_HD int bmpc_tune_check(const double *row, const OPTS &o, const SArgs &s, double *used) {
    int bad = 0;
    double lo = 0.0, hi = 0.0;
    for (int k = 0; k < bmpctu::LEN; k++) {
        double v = k < bmpctu::SLOTS ? row[k] : 0.0;
        if (k < bmpctu::SLOTS) {
            if (v != v) v = bmpc_tune_launch_value(k, o, s);
            else if (!bmpc_tune_slot_ok(k, v)) bad |= 1 << k;
        }
        if (k == bmpctu::LVL_LO) lo = v;
        if (k == bmpctu::LVL_HI) hi = v;
        if (used) used[k] = v;
    }
    if (hi > 0.0 && !(lo > 0.0 && lo <= hi)) bad |= 1 << bmpctu::CROSS;
    return bad;
}
// A VALID row onto the option record of a solve and onto (a copy of) the stream arguments: every slot that is not NaN replaces its value
template <class OPTS>
BMPC_ARGS_HD void bmpc_tune_opts(const double *row, OPTS &o) {
    double v;
    v = row[bmpctu::MAX_ITER]; if (v == v) o.max_iter = (int)v;
    v = row[bmpctu::TOL]; if (v == v) o.tol = v;
    v = row[bmpctu::MU_INIT]; if (v == v) o.mu_init = v;
    v = row[bmpctu::MU_WARM]; if (v == v) o.mu_warm = v;
    v = row[bmpctu::MU_MIN_FAC]; if (v == v) o.mu_min_fac = v;
    v = row[bmpctu::SLACK_PUSH]; if (v == v) o.slack_push = v;
    v = row[bmpctu::BOUND_MARGIN]; if (v == v) o.bound_margin = v;
    v = row[bmpctu::HOLD]; if (v == v) o.hold_mu = (int)v;
    v = row[bmpctu::STALL_WINDOW]; if (v == v) o.stall_window = (int)v;
}
BMPC_ARGS_HD void bmpc_tune_sargs(const double *row, SArgs &s) {
    double v;
    v = row[bmpctu::LVL_C]; if (v == v) s.lvl_c = v;
    v = row[bmpctu::LVL_LO]; if (v == v) s.lvl_lo = v;
    v = row[bmpctu::LVL_HI]; if (v == v) s.lvl_hi = v;
    v = row[bmpctu::RT_TOL]; if (v == v) s.rt_tol = v;
    v = row[bmpctu::RT_ROW_CAP]; if (v == v) s.rt_row_cap = v;
}

// ---- host and device: a row of a per-stream actuator model (BMPC_PLANT_* of include/boundmpc_hip.h), its state and its record; the rule of the step is
// stream_plant (bmpc_stream_plant.inl) ----
namespace bmpcpl {
enum { GAIN = 0,          // [7] actuator gain of joint j                                    identity 1, valid when finite
       BIAS = 7,          // [7] jerk offset, rad/s^3                                        identity 0, valid when finite
       LAG = 14,          // first-order response per tick, u_act += LAG (a - u_act)        identity 1 (none), valid when 0 < LAG <= 1
       SAT = 15,          // jerk magnitude the drive delivers                               identity +inf (none), valid when > 0 (+inf allowed)
       DELAY = 16,        // 1: the command applied is the previous tick's                   identity 0, valid when 0 or 1
       SLOTS = 17,        // the slots that are looked at; the words behind them up to LEN are pad
       LEN = 20 };
enum { ST_ACT = 0, ST_CMD = 7, ST_LEN = 16 };      // the state: the lag's state [7], the previous command [7], two pad words
enum { REC_SAMPLES = 0, REC_N_SAT, REC_MAX_DU, REC_TICK_DU, REC_JOINT_DU, REC_SUMSQ_DU, REC_LEN = 8 };      // the record; two pad words
}
// what a NaN slot resolves to: the plant that IS the model
BMPC_ARGS_HD double bmpc_plant_identity(int k) { return k < bmpcpl::BIAS ? 1.0 : k < bmpcpl::LAG ? 0.0 : k == bmpcpl::LAG ? 1.0 : k == bmpcpl::SAT ? __builtin_huge_val() : 0.0; }
// THE validity rule of a slot that is not NaN, once (plain comparisons)
BMPC_ARGS_HD bool bmpc_plant_slot_ok(int k, double v) {
    if (k < bmpcpl::LAG) return v >= -BMPC_TOL_MAX && v <= BMPC_TOL_MAX;
    if (k == bmpcpl::LAG) return v > 0.0 && v <= 1.0;
    if (k == bmpcpl::SAT) return v > 0.0;
    if (k == bmpcpl::DELAY) return v == 0.0 || v == 1.0;
    return true;      // (pad words: never looked at)
}
// Row `row`: the mask of its invalid slots, bit k = slot k; 0 = the stream runs.  used (or NULL): the row as resolved -- a NaN slot its identity value, a
// refused value as it was given, pad words 0.
BMPC_ARGS_HD int bmpc_plant_check(const double *row, double *used) {
    int bad = 0;
    for (int k = 0; k < bmpcpl::LEN; k++) {
        double v = k < bmpcpl::SLOTS ? row[k] : 0.0;
        if (k < bmpcpl::SLOTS) {
            if (v != v) v = bmpc_plant_identity(k);
            else if (!bmpc_plant_slot_ok(k, v)) bad |= 1 << k;
        }
        if (used) used[k] = v;
    }
    return bad;
}

// ---- host and device: a row of a per-stream measurement model (BMPC_SENSOR_* of include/boundmpc_hip.h), its state and its record; the rule of the two
// steps is stream_sense and stream_truth (bmpc_stream_sensor.inl) ----
namespace bmpcse {
enum { BIAS = 0,          // [7] encoder offset of joint j, rad                               identity 0, valid when finite
       RES = 7,           // quantisation step of the joint positions, rad                   identity 0 (none), valid when finite and >= 0
       NQ = 8, NDQ, NDDQ, // scale of the tick's noise row on q, dq, ddq                     identity 0, valid when finite and >= 0
       HOLD = 11,         // 1: the controller sees the previous tick's sample              identity 0, valid when 0 or 1
       SLOTS = 12,        // the slots that are looked at; the words behind them up to LEN are pad
       LEN = 16 };
// the state: the sample taken last [21], whether there is one, whether the sample handed out equals the truth, a pad word, the truth of a tick in flight
// (the words RB_Q..RB_V of the robot record [33], then RB_JERK [7])
enum { ST_HELD = 0, ST_HAS = 21, ST_SAME = 22, ST_TRUTH = 24, TRUTH_LEN = 40, ST_LEN = 64 };
// the record: samples, largest |q_m - q| with its tick and joint, largest ||p_m - p|| (position part of p_lie, metres) with its tick, sum of squares of q_m - q, a pad word
enum { REC_SAMPLES = 0, REC_MAX_DQ, REC_TICK_DQ, REC_JOINT_DQ, REC_MAX_DP, REC_TICK_DP, REC_SUMSQ_DQ, REC_LEN = 8 };
}
// what a NaN slot resolves to: the sensor that measures the plant exactly
BMPC_ARGS_HD double bmpc_sensor_identity(int k) { return 0.0; }
// THE validity rule of a slot that is not NaN, once (plain comparisons; the offsets within the bound bmpc_plant_slot_ok holds the gains to)
BMPC_ARGS_HD bool bmpc_sensor_slot_ok(int k, double v) {
    if (k < bmpcse::RES) return v >= -BMPC_TOL_MAX && v <= BMPC_TOL_MAX;
    if (k < bmpcse::HOLD) return v >= 0.0 && v <= BMPC_TOL_MAX;
    if (k == bmpcse::HOLD) return v == 0.0 || v == 1.0;
    return true;      // (pad words: never looked at)
}
// Row `row`: the mask of its invalid slots, bit k = slot k; 0 = the stream runs.  used (or NULL): the row as resolved -- a NaN slot its identity value, a
// refused value as it was given, pad words 0.
BMPC_ARGS_HD int bmpc_sensor_check(const double *row, double *used) {
    int bad = 0;
    for (int k = 0; k < bmpcse::LEN; k++) {
        double v = k < bmpcse::SLOTS ? row[k] : 0.0;
        if (k < bmpcse::SLOTS) {
            if (v != v) v = bmpc_sensor_identity(k);
            else if (!bmpc_sensor_slot_ok(k, v)) bad |= 1 << k;
        }
        if (used) used[k] = v;
    }
    return bad;
}

// ---- host and device: a row of a per-stream state observer (BMPC_OBSERVER_* of include/boundmpc_hip.h), its state and its record; the rule of the step is
// stream_observe (bmpc_stream_observer.inl) ----
namespace bmpcob {
enum { LQ = 0, LDQ, LDDQ, // correction gain on q, dq, ddq                                   identity 1 (the estimate is the sample), valid when 0 < v <= 1
       LEAD = 3,          // 1: the sample is one tick old, the estimate is advanced a step  identity 0, valid when 0 or 1
       GATE = 4,          // innovation gate on the joint positions, rad                     identity +inf (none), valid when > 0, +inf allowed
       SLOTS = 5,         // the slots that are looked at; the words behind them up to LEN are pad
       LEN = 8 };
// the state: the last posterior [21], the record's jerk at the posterior's time [7], the record's jerk read at the last call [7], whether there is a
// posterior, whether it is one tick behind the last call, three pad words
enum { ST_POST = 0, ST_JP = 21, ST_JL = 28, ST_HAS = 35, ST_LAGS = 36, ST_LEN = 40 };
// the record: estimates, gate rejections, largest |q_est - q| with its tick and joint, largest ||p_est - p|| (position part of p_lie, metres) with its tick,
// sum of squares of q_est - q
enum { REC_SAMPLES = 0, REC_N_REJ, REC_MAX_DQ, REC_TICK_DQ, REC_JOINT_DQ, REC_MAX_DP, REC_TICK_DP, REC_SUMSQ_DQ, REC_LEN = 8 };
}
// what a NaN slot resolves to: the observer that hands the sample on
BMPC_ARGS_HD double bmpc_observer_identity(int k) { return k < bmpcob::LEAD ? 1.0 : k == bmpcob::GATE ? __builtin_inf() : 0.0; }
// THE validity rule of a slot that is not NaN, once (plain comparisons)
BMPC_ARGS_HD bool bmpc_observer_slot_ok(int k, double v) {
    if (k < bmpcob::LEAD) return v > 0.0 && v <= 1.0;
    if (k == bmpcob::LEAD) return v == 0.0 || v == 1.0;
    if (k == bmpcob::GATE) return v > 0.0;      // (+inf: no gate)
    return true;      // (pad words: never looked at)
}
// Row `row`: the mask of its invalid slots, bit k = slot k; 0 = the stream runs.  used (or NULL): the row as resolved -- a NaN slot its identity value, a
// refused value as it was given, pad words 0.
BMPC_ARGS_HD int bmpc_observer_check(const double *row, double *used) {
    int bad = 0;
    for (int k = 0; k < bmpcob::LEN; k++) {
        double v = k < bmpcob::SLOTS ? row[k] : 0.0;
        if (k < bmpcob::SLOTS) {
            if (v != v) v = bmpc_observer_identity(k);
            else if (!bmpc_observer_slot_ok(k, v)) bad |= 1 << k;
        }
        if (used) used[k] = v;
    }
    return bad;
}

// ---- host only: what the rollout entries of the C ABI refuse and which kernel they run, once (bmpc_hip.hip rollout_launch; the CPU build of the
// rollout, tests/emu/bmpc_emu_rollout.cpp, asks the same function) ----
// the flags of bmpc_stream_update: bit 0 set_goal, bit 1 splice (needs the robot records), bit 2 poor bounds (with bit 1 only)
inline bool bmpc_update_flags_ok(int flags, const void *robot) { return !(flags & ~7) && !((flags & 4) && !(flags & 2)) && !((flags & 2) && !robot); }
// entry: the entry point the caller used -- 0 bmpc_stream_rollout, 1 _events, 2 _audit, 3 _log, 4 _legs, 5 _tuned, 6 _plant; r: its arguments (what an entry has no argument for is
// 0 / NULL); N: the handle's horizon; flags, robot: the tick flags and the robot records.  Returns the level of the kernel text to run -- 0 plain, 1 EV,
// 2 EV + AU, 3 EV + AU + LG, 4 all of them with the queue (QU: the one text that reads a queue, whatever else is on), 5 all of them with the table of
// per-stream settings (TU: with or without a queue or any of the other arrays; the table's rows are validated on the device, where they live), 6 all of
// them with the plant table (PL: with or without a queue, a settings table or any of the other arrays; validated on the device too) -- or
// BMPC_ROLLOUT_REFUSED (the C ABI's BMPC_ERR_ARG).  An entry without the arrays of its own feature IS the entry below it.
enum { BMPC_ROLLOUT_REFUSED = -1 };
inline int bmpc_rollout_level(int entry, const RArgs &r, int N, int flags, const void *robot) {
    if (r.ticks < 1 || !(r.goal_tol >= 0.0 && r.goal_tol <= BMPC_TOL_MAX)) return BMPC_ROLLOUT_REFUSED;      // (negative, NaN or infinite)
    if (!(flags & 1)) return BMPC_ROLLOUT_REFUSED;                    // without the plant in the loop a second tick repeats the first
    if (entry == 6) {      // the plant: whatever the sweeps entry refuses, and a table without its state; without a table that entry, and no plant argument is looked at
        const int below = bmpc_rollout_level(5, r, N, flags, robot);
        if (below == BMPC_ROLLOUT_REFUSED || !r.plant) return below;
        return r.plant_state ? 6 : BMPC_ROLLOUT_REFUSED;
    }
    if (entry == 5) {      // the table: whatever the queue entry refuses; without a table that entry, and no table argument is looked at
        const int below = bmpc_rollout_level(4, r, N, flags, robot);
        return (below == BMPC_ROLLOUT_REFUSED || !r.tune) ? below : 5;
    }
    if (entry == 0) return 0;
    if (entry == 4) {      // the queue: without records the log entry without a re-plan, and no queue argument is looked at
        if (r.replan && (!r.leg_tick || !r.leg_on || !r.legs_done || r.legs < 1)) return BMPC_ROLLOUT_REFUSED;
        if (!r.replan) entry = 3;
    } else if (r.replan && !r.replan_tick) return BMPC_ROLLOUT_REFUSED;
    if (!bmpc_update_flags_ok(r.update_flags, robot)) return BMPC_ROLLOUT_REFUSED;
    if (entry == 4) return (r.log_hist || r.track) && (r.log_stages < 1 || r.log_stages > N) ? BMPC_ROLLOUT_REFUSED
                           : (r.audit_tol >= 0.0 && r.audit_tol <= BMPC_TOL_MAX) ? 4 : BMPC_ROLLOUT_REFUSED;
    if (entry >= 3 && (r.log_hist || r.track)) {
        if (r.log_stages < 1 || r.log_stages > N) return BMPC_ROLLOUT_REFUSED;
    } else if (entry >= 3) entry = 2;
    if (entry >= 2 && !(r.audit_tol >= 0.0 && r.audit_tol <= BMPC_TOL_MAX)) return BMPC_ROLLOUT_REFUSED;
    if (entry == 2 && !r.tube_hist && !r.audit) entry = 1;
    return entry;
}
// What bmpc_stream_rollout_sensor refuses on top of what the plants' entry refuses (bmpc_rollout_level with entry 6 on its RArgs): a table without its
// state.  Without a table it IS that entry, and no member of `n` is looked at.
inline bool bmpc_rollout_sensor_ok(const NArgs &n) { return !n.sensor || n.sensor_state; }
// What bmpc_stream_rollout_observer refuses on top of what the sensors' entry refuses: an observer without a sensor table -- there is no sample to
// filter -- and an observer without its state.  Without an observer table it IS that entry, and no member of `o` is looked at.
inline bool bmpc_rollout_observer_ok(const NArgs &n, const OArgs &o) { return !o.observer || (n.sensor && o.observer_state); }
