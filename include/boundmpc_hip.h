/*
 * boundmpc_hip.h -- C ABI of the MI355X-native batched BoundMPC OCP solver (measurements and design notes: DESIGN.md).
 *
 * Drop-in boundary.  In the reference (Thieso/BoundMPC) the per-step optimisation is one CasADi `nlpsol('solver','ipopt',...)` Function object,
 * created at bound_mpc/bound_mpc/BoundMPC/casadi_ocp_formulation.py:389 and invoked only at BoundMPC/BoundMPC.py:446-453 (sol = solver(x0=, lbx=,
 * ubx=, lbg=, ubg=, p=)) and :456 (solver.stats()).  The reference defines no C ABI for it; these entry points carry what that call carries, batched:
 *   bmpc_create       <-> setup_optimization_problem(N, 7, nr_segs, dt, ...) (casadi_ocp_formulation.py:9-11) + the Ipopt option dict (BoundMPC.py:120-148)
 *   bmpc_get_bounds   <-> the lbu, ubu, lbg, ubg lists returned there (casadi_ocp_formulation.py:384-391)
 *   bmpc_solve_batch  <-> solver(x0=, ..., p=) -> {'x','f','g','lam_x','lam_g'} (BoundMPC.py:446-453) and solver.stats() (:456-457), one record per problem
 *   bmpc_destroy      <-> garbage collection of the Function object
 * All arithmetic is fp64.  Layouts (row-major, one problem per row):
 *   p      [B][n_p]   n_p = 141 + 91 S, parameter vector in the order of casadi_ocp_formulation.py:361-376
 *   x0, x  [B][44 N]  stage variables z_k = [u(7) u_phi | q dq ddq | p(6) | v(6) | phi dphi ddphi] (:90-153)
 *   g      [B][43 N]  constraints in the reference's order and form (:272-349); lam_g [B][43 N] (sign: L = f + lam_g . g); lam_x [B][44 N]
 *   f, kkt [B]; iters [B]; status [B]: 0 converged, 1 max_iter reached, 2 locally infeasible (restoration phase, or a stall that survived the
 *   barrier restarts of a long horizon), 3 numerical failure.  Per-problem failure is data, never an error code (BoundMPC.py:465-489).
 * lbx / ubx / lbg / ubg are structural constants of the formulation and do not cross the ABI per call (bmpc_get_bounds).
 * Ownership: the caller owns every buffer; the library owns the handle and its device workspace (allocated by the first solve or capture for
 * min(B, resident workgroups), grown on demand after a host wait for the handle's own last launch; it cannot grow while captured graphs of the
 * handle exist: capture for the largest batch first).  Errors are integer return codes.  One in-flight call per handle from the host's side.
 */
#ifndef BOUNDMPC_HIP_H
#define BOUNDMPC_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct bmpc_handle bmpc_handle;

typedef struct {
    double tol;         /* scaled KKT tolerance (Ipopt's error measure; reference 'tol': 10e-6, BoundMPC.py:121); default 1e-8 */
    int max_iter;       /* default 500 (BoundMPC.py:122) */
    double mu_init;     /* first barrier level: 0.1 for N <= 11, 3.0 for longer horizons (bmpc_default_options_for) */
    double mu_min_fac;  /* last barrier level = tol * mu_min_fac; default 0.1 */
    double slack_push;  /* smallest initial slack of an inequality row: 1e-2 for N <= 11, 0.1 for longer horizons */
    int exact_hessian;  /* 1 (default): exact Lagrangian Hessian, as the reference; 0: Gauss-Newton */
    int verbose;
    double mu_warm;     /* warm start (bmpc_solve_batch_warm): the barrier restarts at clamp(stored mu, mu_warm, mu_init); default 1e-2 */
    int stall_window;   /* stalled = the primal infeasibility has not halved over this many iterations (even; checked every half window; 0 = never);
                           default 40 for N <= 11, 20 beyond; 16 recommended for warm-started streams.  A stall starts the restoration phase
                           (N <= 11) or a barrier restart, then status 2 (longer horizons, or restoration off) */
    double bound_margin;/* joint position / velocity limits tightened by this much (rad, rad/s) inside the solver; default 0 = the reference's
                           limits (RobotModel.py:20-39); for real-time loops solved to a loose tolerance or a budget */
} bmpc_options;

enum { BMPC_OK = 0, BMPC_ERR_ARG = 1, BMPC_ERR_HIP = 2, BMPC_ERR_NOGPU = 4 };

/* sizeof(bmpc_options) of the library (the struct grew by bound_margin once; later additions are handle setters, not fields) */
int bmpc_options_size(void);
/* 16 hex digits: hash of the source text and compiler flags the library was built from (boundmpc_amd/build.py source_hash) */
const char *bmpc_build_hash(void);
int bmpc_default_options(bmpc_options *o);                 /* the N <= 11 defaults */
int bmpc_default_options_for(int N, bmpc_options *o);      /* defaults for horizon N; what bmpc_create(..., NULL, ...) uses */
const char *bmpc_error_string(int code);

/* N horizon (1..40), S path segments in the window (2..6), dt sampling time */
int bmpc_create(int N, int S, double dt, const bmpc_options *opts, bmpc_handle **out);
int bmpc_destroy(bmpc_handle *h);

/* Restoration phase -- what stands where Ipopt's filter line search falls back to its restoration phase (BoundMPC.py:135; Waechter & Biegler 2006,
 * 3.3).  A main phase that is jammed (`short_steps` consecutive steps shorter than 10 % with the primal infeasibility open; default 6), stalled or
 * numerically broken (dual residual beyond 1e12) switches to  min rho sum e  s.t. dynamics, h(x) - e <= 0, e >= 0  (rho = 1000, objective weights
 * zero) on the same Riccati recursion, and returns to the main phase from the first strictly feasible iterate, or ends the solve with status 2: converged
 * to a point of non-zero violation, `cap` iterations (default 40) without a feasible point, or the fourth call within one solve.
 * enabled: 0 never; 1 full (jam, stall, breakdown; long horizons: behind their three barrier restarts, never on a jam); 2 after a numerical
 * breakdown only.  Default 1 for N <= 11, 2 beyond.  A negative argument keeps the current value; nothing is changed when any argument is
 * invalid.  Read at launch / capture time; every launch shape (batch, fused tick, three-kernel tick) runs the handle's mode; time-budgeted
 * real-time ticks run without the phase. */
int bmpc_set_restoration(bmpc_handle *h, int enabled, int short_steps, int cap);
int bmpc_get_restoration(const bmpc_handle *h, int *enabled, int *short_steps, int *cap);

/* Rollout of a cold start that is not a trajectory.  A STATELESS solve (bmpc_solve_batch / bmpc_solve_batch_host: no dual state buffer,
 * max_iter > 0) whose x0 violates an integrator-chain row of g (q, dq, ddq, phi, dphi, ddphi) by more than 0.5 starts from the rollout of x0's
 * own jerks from the measured state, lifted variables projected.  The reference's own starts (its cold start BoundMPC.py:316-321, a shifted
 * plan :322-375) stay below the threshold; solves that carry a dual state (bmpc_solve_batch_warm, stream ticks) are never touched.
 * enabled: 1 (default) / 0 (x0 as given: what a caller that drives a receding-horizon loop through the stateless entry points wants).
 * Read at launch / capture time. */
int bmpc_set_start_rollout(bmpc_handle *h, int enabled);
int bmpc_get_start_rollout(const bmpc_handle *h);      /* 0 / 1; -1: no handle */

int bmpc_num_vars(const bmpc_handle *h);    /* 44 N */
int bmpc_num_cons(const bmpc_handle *h);    /* 43 N */
int bmpc_num_params(const bmpc_handle *h);  /* 141 + 91 S */

/* HOST pointers, lengths 44 N, 44 N, 43 N, 43 N */
int bmpc_get_bounds(const bmpc_handle *h, double *lbx, double *ubx, double *lbg, double *ubg);

/* DEVICE pointers; g, lam_g, lam_x, f, iters, status, kkt may be NULL.  hip_stream: hipStream_t to launch on (NULL = default stream).
 * Asynchronous w.r.t. the host.
 * x and x0: with the second attempt off (bmpc_set_second_attempt cap 0, the default for N <= 11) x may be x0 itself -- a problem's x0 is read in
 * full before its x is written, so an in-place solve gives the out-of-place results bit for bit.  With cap > 0 the second attempt reads x0 AGAIN
 * after the first attempt has written x: the ranges [x, x + 44 N B) and [x0, x0 + 44 N B) must not overlap, and the call returns BMPC_ERR_ARG
 * (nothing launched) when they do.  The same holds for bmpc_graph_create without a state.  bmpc_solve_batch_host stages its own copies. */
int bmpc_solve_batch(bmpc_handle *h, int B, const double *p, const double *x0, double *x, double *g, double *lam_g, double *lam_x,
                     double *f, int *iters, int *status, double *kkt, void *hip_stream);

/* Warm-started solve for receding-horizon streams: the reference's x0 (the shifted previous solution, BoundMPC.py:322-375) plus the solver's dual
 * state carried across ticks (the reference's lam_g0 / lam_x0 hand-over is commented out, :451-452).
 *   state [B][bmpc_state_len(h)] DEVICE doubles, read and updated in place: [nu (N x 57 internal inequality rows) | mu | iterations].
 *   mu <= 0 (a zeroed row): cold start, identical to bmpc_solve_batch.  Otherwise the barrier restarts at clamp(stored mu, mu_warm, mu_init),
 *   every slack at max(-h_i(x0), min(mu / nu_i, slack_push)).  The caller shifts `state` with x0 when the horizon advances (bmpc_stream_pack does).
 * max_iter > 0 overrides options.max_iter for this call (real-time iteration: status 1 is then the normal outcome); 0 keeps the option. */
int bmpc_state_len(const bmpc_handle *h);   /* 57 N + 2 */
int bmpc_solve_batch_warm(bmpc_handle *h, int B, const double *p, const double *x0, double *state, int max_iter, double *x, double *g,
                          double *lam_g, double *lam_x, double *f, int *iters, int *status, double *kkt, void *hip_stream);

/* Primal-dual warm start from multipliers in CasADi's convention (what a solve returns as lam_g / lam_x; the reference's lam_g0 / lam_x0,
 * BoundMPC.py:451-452): the dual state of bmpc_solve_batch_warm, computed on the GPU.  Each problem is evaluated at x0 as a solve begins (no start
 * rollout); then per node k, with pos(v) = max(v, 0) and the internal rows of the state:
 *   upper / lower row of jerk j (8), q_j and dq_j (7 each)   pos(lam_x[z]) / pos(-lam_x[z]) of that variable z
 *   phi >= 0                                                  pos(-lam_x[phi])
 *   phi <= phi_max, dphi <= dphi_max                          pos(lam_g[36]), pos(lam_g[37])
 *   tube row m (m < 5): the pair c - wd <= 0, -c - wd <= 0    pos(lam (wd + c)), pos(lam (wd - c)) with lam = pos(lam_g[38 + m])
 * c and wd >= 0 are the centre value and the half width of the squared tube row c^2 - wd^2 <= 0 at x0; the map is the exact inverse of the
 * solver's own output map wherever |c| <= wd.  IGNORED: the equality multipliers lam_g[0:36] (the solver recomputes them at every iterate) and
 * lam_x of unbounded variables.  A non-finite entry counts as 0; a converted multiplier is capped at 1e12.
 * State slot mu = mu0 when mu0 > 0, else options.mu_warm (the warm solve then starts at clamp(mu, mu_warm, mu_init)); a problem whose converted
 * multipliers are all 0 gets mu = 0: the cold start of the warm path.  Slot iterations = 0.
 * A solve with a state gets neither the start rollout (bmpc_set_start_rollout) nor the second attempt (bmpc_set_second_attempt).
 * DEVICE pointers; lam_g0 [B][43 N] and lam_x0 [B][44 N] may be NULL (= zeros); state [B][bmpc_state_len(h)] is written.  Uses the handle's
 * workspace: ordered against its other launches like bmpc_solve_batch. */
int bmpc_state_from_multipliers(bmpc_handle *h, int B, const double *p, const double *x0, const double *lam_g0, const double *lam_x0,
                                double mu0, double *state, void *hip_stream);

/* KKT certificate of ANY primal-dual point: the solver's error measure for a point (x, lam_g, lam_x) in CasADi's convention that the solver need
 * not have produced -- Ipopt's answer, an SLSQP run, a shifted plan, a candidate warm start, the rows a graph replay just returned.  `kkt` of a
 * solve is measured on the solve's own slacks at its last barrier level; a point carries no slacks, so here the slack of an internal inequality
 * row h_i <= 0 is max(-h_i, 0).  Per problem: the evaluation at x (the point is taken AS GIVEN: neither the start rollout nor the second attempt
 * applies, nothing is projected); lam_g0[36:43] / lam_x0 mapped onto the 57 N internal multipliers nu by the map of bmpc_state_from_multipliers
 * (pos(), tube pair lam (wd +- c), cap 1e12, a non-finite entry counts as 0); the adjoint sweep of a solver iteration, which RECOMPUTES the
 * equality multipliers LAM [N][36] that zero the state part of the Lagrangian gradient and leaves its jerk part RJ [N][8].  The equality
 * multipliers the caller passes are compared with them (slot 5), never trusted.  Record cert[b][BMPC_KKT_LEN] (doubles):
 *   BMPC_KKT_E             max(dual / sd, max(prim_eq, prim_ineq), compl / scl), sd = max(100, (sum |LAM| + sum nu) / (93 N)) / 100,
 *                          scl = max(100, sum nu / (57 N)) / 100: the scaled error a solve compares with options.tol
 *   BMPC_KKT_DUAL          max |RJ|: stationarity in the jerks, the states eliminated by the adjoint
 *   BMPC_KKT_PRIM_EQ       max |g[k][0:36]|
 *   BMPC_KKT_PRIM_INEQ     max_i max(h_i, 0) over the 57 N internal rows (the handle's rows: options.bound_margin included)
 *   BMPC_KKT_COMPL         max_i nu_i max(-h_i, 0)
 *   BMPC_KKT_LAM_EQ_GAP    max |lam_g0[k][0:36] - LAM|; 0 when lam_g0 is NULL
 *   BMPC_KKT_LAM_INEQ_GAP  largest |given - re-exported| over lam_g0[k][36:43] and lam_x0, "re-exported" = nu sent back through the output map of a
 *                          solve: 0 up to rounding exactly when the signs are right, unbounded variables carry no lam_x and the point is inside
 *                          its tubes; 0 when both are NULL
 *   BMPC_KKT_F             the objective at x
 * OUTSIDE a tube (|c| > wd for a tube row c^2 - wd^2 <= 0) the pair c - wd <= 0, -c - wd <= 0 gets lam (wd + |c|) on the violated row and 0 on the
 * other: the certificate is that of these split internal rows, and slot 6 shows the multiplier they stand for, lam (wd + |c|) / (2 wd).
 * NON-FINITE: a non-finite entry of lam_g0 / lam_x0 makes its gap slot (5 or 6) +inf and otherwise counts as 0; a non-finite x or p gives a
 * non-finite record -- slots 0..4 are NaN as soon as one of f, g, h, LAM, RJ is not finite -- never a fault.
 * Optional outputs (each may be NULL; they must not overlap the inputs): g [B][43 N]; lam_g [B][43 N], the CONSISTENT multipliers (rows 0:36
 * recomputed, rows 36:43 re-exported); rj [B][8 N].
 * DEVICE pointers; lam_g0 [B][43 N] and lam_x0 [B][44 N] may be NULL.  Uses the handle's workspace: ordered against its other launches like
 * bmpc_solve_batch.  BMPC_ERR_ARG on NULL p / x / cert or B < 1.  bmpc_kkt_batch_host: the same with HOST pointers -- staged copies on a stream
 * of the handle, one synchronisation. */
enum { BMPC_KKT_E = 0, BMPC_KKT_DUAL = 1, BMPC_KKT_PRIM_EQ = 2, BMPC_KKT_PRIM_INEQ = 3, BMPC_KKT_COMPL = 4, BMPC_KKT_LAM_EQ_GAP = 5,
       BMPC_KKT_LAM_INEQ_GAP = 6, BMPC_KKT_F = 7, BMPC_KKT_LEN = 8 };
int bmpc_kkt_len(void);      /* BMPC_KKT_LEN */
int bmpc_kkt_batch(bmpc_handle *h, int B, const double *p, const double *x, const double *lam_g0, const double *lam_x0, double *cert,
                   double *g, double *lam_g, double *rj, void *hip_stream);
int bmpc_kkt_batch_host(bmpc_handle *h, int B, const double *p, const double *x, const double *lam_g0, const double *lam_x0, double *cert,
                        double *g, double *lam_g, double *rj);

/* Parametric sensitivity of the solution: how (x, multipliers) move when the parameter vector moves along dp -- the tangent an nlpsol Function
 * offers with respect to p, for advanced-step corrections between ticks, linear feedback around a plan, derivatives of a closed loop.  Per problem
 * take a primal-dual point (x, lam_g, lam_x) in CasADi's convention (a solve's outputs, Ipopt's answer, ...), p, a direction dp [n_p] and a
 * barrier level mu > 0.  Internal quantities: nu [57 N], lam_g[36:43] / lam_x mapped by the map of bmpc_state_from_multipliers (pos(), tube pair
 * lam (wd +- c), cap 1e12, non-finite -> 0), exactly as bmpc_kkt_batch does; LAM [36 N], the equality multipliers RECOMPUTED by the adjoint sweep
 * (lam_g[0:36] is never trusted); the slack of internal row i, s_i = max(-h_i(x, p), mu / max(nu_i, mu)) -- a point carries no slacks; this is
 * -h_i on a converged interior-point answer and stays positive on an active or slightly violated row --; Sigma_i = nu_i / s_i.
 * The tangent (dx, dLAM, dnu) solves the linearised perturbed barrier KKT system at that point, d/dt along p + t dp, with the Hessian choice of
 * the handle (options.exact_hessian):
 *     H dx + Jg^T dLAM + Jh^T dnu = - d/dt grad_x L(x, LAM, nu; p + t dp)
 *     Jg dx                       = - d/dt g_eq(x; p + t dp)                       (36 N equalities)
 *     dnu_i                       =   Sigma_i (Jh dx + d/dt h(x; p + t dp))_i      (57 N internal rows, slack eliminated)
 * At a converged solution with mu its last barrier level (options.tol * options.mu_min_fac) this is the derivative of the solver's own solution
 * map.  One Riccati factorisation at (x, nu, p) with the inertia rule of a solver iteration, one forward sweep.  The d/dt terms are central
 * differences of the kernel's own residual evaluation at p +- eps dp with x, nu, s held fixed, eps = 1e-6 max(1, |p|_inf) / |dp|_inf: they carry
 * the rounding of a difference (measured 1e-10 .. 6e-7 of max |dx|: DESIGN.md 4g).  dp = 0 takes the step 0 and gives dx = 0 exactly; the step is
 * capped at 1e300.  NO TANGENT exists along the segment switches: the entries phi_switch of p (offset 53 + 9 S, S + 1 of them) select the path
 * segment by comparison, a piecewise-constant condition without a derivative (as in CasADi); a dp with non-zero entries there is differenced
 * across a jump or not at all, and the result is meaningless.  Leave those entries of dp at zero.
 * Record rec[b][BMPC_SENS_LEN] (doubles):
 *   BMPC_SENS_STATUS  0: factorised with delta = 0.  1: regularised -- the tangent is that of H + delta I.  3: no factorisation, or a non-finite
 *                     entry of x, p or dp (or a non-finite right-hand side): dx (and dlam_eq, dnu) are NaN then; never a fault
 *   BMPC_SENS_DELTA   the delta of status 1, else 0
 *   BMPC_SENS_RHS     max |right-hand side|: the largest of |d/dt h|, |d/dt g_eq| and the jerk part of |d/dt grad_x L| with the states eliminated
 *   BMPC_SENS_DX      max |dx|
 * Buffers: dp [B][n_p]; dx [B][44 N] (required); dlam_eq [B][36 N], dnu [B][57 N] (internal rows, the order of the dual state) and rec may be
 * NULL.  dlam_eq costs a second pair of evaluations: the adjoint's multipliers differenced along the whole tangent (x, nu, p); it satisfies the
 * stationarity rows with the exact Hessian and delta = 0.  mu <= 0: options.tol * options.mu_min_fac.  lam_g [B][43 N] / lam_x [B][44 N] may be
 * NULL (= zeros).  DEVICE pointers; outputs must not overlap inputs.  Uses the handle's workspace: ordered against its other launches like
 * bmpc_solve_batch.  BMPC_ERR_ARG on NULL p / x / dp / dx or B < 1.  bmpc_sens_batch_host: the same with HOST pointers -- staged copies on a
 * stream of the handle, one synchronisation. */
enum { BMPC_SENS_STATUS = 0, BMPC_SENS_DELTA = 1, BMPC_SENS_RHS = 2, BMPC_SENS_DX = 3, BMPC_SENS_LEN = 4 };
int bmpc_sens_len(void);      /* BMPC_SENS_LEN */
int bmpc_sens_batch(bmpc_handle *h, int B, const double *p, const double *x, const double *lam_g, const double *lam_x, const double *dp, double mu,
                    double *dx, double *dlam_eq, double *dnu, double *rec, void *hip_stream);
int bmpc_sens_batch_host(bmpc_handle *h, int B, const double *p, const double *x, const double *lam_g, const double *lam_x, const double *dp,
                         double mu, double *dx, double *dlam_eq, double *dnu, double *rec);

/* The same step captured once into a hipGraph and replayed per tick: buffers are fixed at capture time, the caller refreshes their contents.
 * Launches of one handle (direct or replayed) share its workspace: the library orders them against each other with an event whatever streams the
 * caller uses (exception: a launch on a stream the CALLER is capturing neither waits for nor records that event).  A graph keeps the workspace and
 * the latency buffer registered at capture time and holds a reference on the handle: bmpc_destroy of a handle with live graphs closes it (the
 * graphs then refuse to launch), the last bmpc_graph_destroy frees it.  bmpc_graph_launch(g, NULL) replays on a non-blocking stream of the handle,
 * ordered by events against the legacy null stream (tests/cabi/graph_nullstream.cpp has the ROCm 7.2 fault this avoids). */
typedef struct bmpc_graph bmpc_graph;
int bmpc_graph_create(bmpc_handle *h, int B, const double *p, const double *x0, double *state, int max_iter, double *x, double *g,
                      double *lam_g, double *lam_x, double *f, int *iters, int *status, double *kkt, bmpc_graph **out);
int bmpc_graph_launch(bmpc_graph *g, void *hip_stream);
int bmpc_graph_destroy(bmpc_graph *g);

/* ---- Receding-horizon streams: the per-tick host arithmetic of BoundMPC.step() as device kernels (one wave per stream) ----
 * bmpc_stream_pack <-> step() pre-solve, BoundMPC.py:310-443 (ReferencePath window ReferencePath.py:178-238, warm start :316-333,372-375,
 *     compute_initial_rot_errors util_functions.py:11-31, projection vectors :267-304, tube quartics :219-265): (path table, stream state,
 *     robot record) -> p, x0; also shifts the solver's dual state with the plan (dual_state may be NULL).
 * bmpc_stream_post <-> step() post-solve, BoundMPC.py:460-506 (feasibility rule, fallback to the previous plan) and compute_return_data :513-611.
 *     flags bit 0 (simulate): also advance the robot record like the node's kinematic simulation (util_functions.py:152-161, bound_mpc_node.py:292-372).
 *     flags bit 1 (real-time iteration, not in the reference): the acceptance rule of BoundMPC.py:460-465 decides with the threshold of
 *     bmpc_stream_set_rt_feasibility_tol and with the violation of lbx <= x <= ubx added; a rejected iterate is not applied (the previous plan is
 *     replayed, :468-489) and the next warm start continues from it (bmpc_stream_pack_rt with xlast = the solver's x; bmpc_stream_tick does
 *     so on every launch shape; plain bmpc_stream_pack restarts from the accepted plan as the reference does; status 3 is never continued from).
 * DEVICE doubles, one row per stream, row lengths from bmpc_stream_lengths:
 *   path   [B][path_entries][path_entry]  static via-point table (layout: csrc/bmpc_stream.inl; builder: boundmpc_amd.stream.path_table)
 *   sstate [B][state]   [header 32: phi-state, rotation reference, sector, error count, weights | previous solution 44 N | Cartesian pos, vel,
 *                        acc, jerk of the previous plan 4 x 3 x N | updated flag | real-time continuation word (written by bmpc_stream_post, read by
 *                        bmpc_stream_pack_rt) | dphi_max | pad].  dphi_max is the bound of the hard row dphi <= dphi_max: weights[4] as the stream was
 *                        CREATED with (BoundMPC.py:77-79; builder: boundmpc_amd.stream.initial_state).  A re-plan replaces the weights and leaves this
 *                        word, as the reference's update() does (:194).  A row that holds 0 there packs the current weights[4].
 *                        Contract of the path table: every entry's error-plane bases are orthonormal to the entry's own direction (bp1, bp2) and rotation
 *                        axis (br1, br2).  bmpc_stream_pack reads the zyx angles of the frame [br2, d, br1] through a normalised quaternion; for a frame
 *                        that is not orthogonal (a basis vector replicated onto a segment with another axis, nb < n of a re-plan record) the reference's
 *                        host code takes the nearest rotation instead, and the packed ipar, io1, io2, v1..v3 differ from it by O(1).
 *   robot  [B][robot]   q dq ddq p_lie v x_phi_d jerk = the arguments of step() (read; written when simulate)
 *   traj   [B][traj]    q dq ddq dddq (7 x N) | p v a (6 x N) | phi dphi ddphi dddphi (N) | n_valid using_previous success g_viol
 * Re-planning (BoundMPC.update, BoundMPC.py:163-217): bmpc_stream_update (below; one launch over the batch) or the host (one stream at a time,
 * boundmpc_amd.stream.apply_update) writes the new path table and the state scalars and raises the `updated` flag; bmpc_stream_pack then takes
 * the re-projection branch of step() (:335-369). */
int bmpc_stream_lengths(const bmpc_handle *h, int *path_entry, int *state, int *robot, int *traj);
int bmpc_stream_pack(bmpc_handle *h, int B, const double *path, int path_entries, double *sstate, const double *robot, double *p, double *x0,
                     double *dual_state, void *hip_stream);
/* bmpc_stream_pack with the real-time continuation: xlast (DEVICE [B][44 N] or NULL) = the iterate the solver produced last tick */
int bmpc_stream_pack_rt(bmpc_handle *h, int B, const double *path, int path_entries, double *sstate, const double *robot, double *p, double *x0,
                        double *dual_state, const double *xlast, void *hip_stream);
int bmpc_stream_post(bmpc_handle *h, int B, const double *path, int path_entries, double *sstate, double *robot, const double *x, const double *g,
                     const int *status, double *traj, int flags, void *hip_stream);
/* Threshold on the summed violation (beyond 1e-6 per row) below which bmpc_stream_post applies an iteration-capped iterate in real-time mode.
 * Default 1e-4 = the reference's rule (BoundMPC.py:462-465).  Read when a post is launched or captured. */
int bmpc_stream_set_rt_feasibility_tol(bmpc_handle *h, double tol);
/* Real-time mode (flags bit 1): a position tube row (rows 39, 40 of any stage of g: l^2 - w^2, m^2) above `cap_m2` vetoes the iterate whatever the
 * summed violation (an excess of d metres at half width w is a row of 2 w d + d^2: 1e-5 keeps every stage of an accepted plan -- also the tail a
 * stream replays after failed ticks, BoundMPC.py:468-489 -- within 0.5 mm of a 10 mm tube).  0 (default) = off: the reference's summed rule alone. */
int bmpc_stream_set_rt_position_row_cap(bmpc_handle *h, double cap_m2);
/* Real-time iteration on a HELD barrier level (what bench.py reports for BASELINE configs[4]).  bmpc_set_barrier_hold(h, 1): a solve keeps the level it
 * starts on -- clamp(level stored in the dual state, options.mu_warm, options.mu_init); a cold state starts on mu_init -- instead of walking the barrier
 * down; `tol` then never fires, the iteration cap or time budget ends every solve.  bmpc_stream_set_level_rule(h, c, lo, hi): bmpc_stream_pack (and the
 * fused ticks) write the level of a stream's next solve into its warm dual state: clamp(c (phi_max - phi), lo, hi) -- robust level `hi` far from the
 * end of the path, lower near it, where the barrier of phi <= phi_max would otherwise stall the stream short of its goal (the reference runs Ipopt's
 * adaptive barrier strategy, BoundMPC.py:130-136).  hi = 0 (default): off.  Use lo = options.mu_warm, hi = options.mu_init.  Read at launch / capture time. */
int bmpc_set_barrier_hold(bmpc_handle *h, int enabled);
int bmpc_stream_set_level_rule(bmpc_handle *h, double c, double lo, double hi);
/* Time budget of a FUSED tick in microseconds from kernel entry; 0 (default) = none.  No further iteration starts once it is used up (status 1):
 * the tick is bounded by budget + one iteration + the post-processing; results of such ticks depend on the clock.  Read at launch / capture time. */
int bmpc_stream_set_time_budget(bmpc_handle *h, double microseconds);
/* One whole tick {pack, warm-started solve with max_iter (0 = options), post} of B streams.  For B within the resident workgroups of the device
 * (bmpc_launch_info; teams: bmpc_team_info) it is ONE kernel launch, whatever N and S; otherwise the three kernels are enqueued.  In the fused
 * launch a stream that has lost its plan (error count >= N: step() returns five Nones there, BoundMPC.py:498-506) is skipped (status 3, 0
 * iterations): re-plan it (bmpc_stream_update / StreamBatch.update_device, or StreamBatch.update from the host) or restart it. */
int bmpc_stream_tick(bmpc_handle *h, int B, const double *path, int path_entries, double *sstate, double *robot, double *p, double *x0,
                     double *dual_state, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                     void *hip_stream);
/* the same tick captured into a hipGraph (one kernel node when it fuses); launch with bmpc_graph_launch */
int bmpc_stream_graph_create(bmpc_handle *h, int B, const double *path, int path_entries, double *sstate, double *robot, double *p, double *x0,
                             double *dual_state, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj,
                             int flags, bmpc_graph **out);
/* Rollout: `ticks` whole ticks of every stream in ONE launch, for closed loops run in bulk (Monte-Carlo runs, tuning, robustness batteries) where
 * the throughput of whole loops counts, not the latency of a tick.  A loop of bmpc_stream_tick launches joins the grid once per tick, so it costs
 * the sum over the ticks of the slowest stream's solve; here every stream runs at its own pace and the launch lasts as long as the slowest
 * stream's sum.  The tick arrays and their argument test are those of bmpc_stream_tick.  Waves per stream: bmpc_set_rollout_waves (below;
 * bmpc_set_team_waves does not apply) -- one wave per stream by default, or a team of BMPC_TEAM_NW cooperating waves.  Workgroup w serves streams
 * w, w + grid, w + 2 grid, ... (grid = min(B, bmpc_launch_info's grid), on teams min(B, resident teams)), so any B is served.
 * Per stream, tick after tick:
 *   lost plan  error count >= N at the start of a tick: what a fused tick writes for a skipped stream (status 3, iters 0, kkt 0) is written
 *              once, everything else keeps its last value, the stream stops;
 *   goal       goal_tol > 0: the stream stops behind the post that leaves phi_max - phi <= goal_tol (the rule of the node's loop); 0 = never.
 * With goal_tol = 0 every tick array (sstate, robot, p, x0, dual_state, x, g, iters, status, kkt, traj) holds afterwards what `ticks` successive
 * bmpc_stream_tick launches on one wave per stream (bmpc_set_team_waves(h, 1)) leave, bit for bit -- on teams what the fused ticks of the teams
 * (bmpc_set_team_waves(h, BMPC_TEAM_NW)) leave; the same holds for the loops of the entries with events, audit and log below.
 *   hist [ticks][B][BMPC_ROLL_LEN] (may be NULL): row [t][b] describes stream b BEHIND tick t: the robot record, phi, the error count, the
 *     solve's iters / status / kkt (NaN where that array is NULL) and the four trailer words of the tick's trajectory record;
 *   traj_hist [ticks][B][traj] (may be NULL): the whole trajectory record of that tick;
 *   ticks_run [B] (may be NULL): the ticks the stream ran.  Rows of ticks a stream did not run -- from its stop on, all of them if it was lost on
 *     entry -- are NaN in both arrays.
 * The barrier hold, the level rule, the real-time feasibility tolerance, the position-row cap and the restoration mode are read from the handle
 * at launch time, as for a tick; the second attempt is off.  A registered latency buffer receives the SUM of the stream's solve durations;
 * bmpc_set_timing brackets the launch like a tick.  The launch uses the handle's workspace and is ordered against the handle's other launches.
 * A direct launch: not to be enqueued inside a stream capture (BMPC_ERR_ARG).  All pointers are DEVICE pointers; asynchronous on hip_stream.
 * First tick: a loop whose tick 0 is solved out and whose later ticks are capped is bmpc_stream_tick (first cap) followed by a rollout of
 * ticks - 1.  BMPC_ERR_ARG, nothing launched: ticks < 1, a missing tick array, flags bit 0 (simulate) clear -- without the plant in the loop a
 * second tick repeats the first --, a negative or non-finite goal_tol, a time budget set on the handle (bmpc_stream_set_time_budget: a rollout
 * is not real time, and budgeted results depend on the clock). */
enum { BMPC_ROLL_ROBOT = 0 /* 43: the robot record behind the tick's post */, BMPC_ROLL_PHI = 43, BMPC_ROLL_ERRCNT = 44, BMPC_ROLL_ITERS = 45,
       BMPC_ROLL_STATUS = 46, BMPC_ROLL_KKT = 47, BMPC_ROLL_NVALID = 48, BMPC_ROLL_USINGPREV = 49, BMPC_ROLL_SUCCESS = 50, BMPC_ROLL_GVIOL = 51,
       BMPC_ROLL_LEN = 52 };
int bmpc_stream_rollout_len(void);
int bmpc_stream_rollout(bmpc_handle *h, int B, int ticks, const double *path, int path_entries, double *sstate, double *robot, double *p, double *x0,
                        double *dual_state, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                        double goal_tol, double *hist /* [ticks][B][52] or NULL */, double *traj_hist /* [ticks][B][traj] or NULL */,
                        int *ticks_run /* [B] or NULL */, void *hip_stream);
/* Waves per stream of the seven rollout entries (bmpc_stream_rollout, _events, _audit, _log, _legs, _tuned, _plant), read at launch time:
 *   1 (default)   one wave per stream, on the resident waves of the device;
 *   BMPC_TEAM_NW  a team of cooperating waves per stream whatever B is, striding over the resident teams (256 on an MI355X: a team owns a CU);
 *                 BMPC_ERR_ARG on a handle without team kernels (N > 10 or S > 4), as bmpc_set_team_waves;
 *   0             automatic: teams when the handle has them and B <= the resident teams, else one wave.
 * Anything else: BMPC_ERR_ARG, the setting stays.  Teams pay where one wave per stream leaves SIMDs idle (B up to the resident teams); their
 * results agree with the one-wave rollout's as the team ticks agree with the one-wave ticks.  bmpc_get_rollout_waves: the setting; -1: no handle. */
int bmpc_set_rollout_waves(bmpc_handle *h, int waves);
int bmpc_get_rollout_waves(const bmpc_handle *h);
/* The logging records of step() (ref_data / err_data, BoundMPC.py:614-752) of the plan a tick left behind, one row per stream:
 *   log [B][bmpc_stream_log_len] = [N][88] | n_valid | error_count | 2 pad,  a stage being
 *     ref (55): p 6, dp 6, ddp 6, dp_normed 3, r_par_bound 1, bound_lower 4, bound_upper 4, e_p_off 2, e_r_off 2, bp1, bp2, br1, br2, v1, v2, v3 (3 each)
 *     err (33): e_p, de_p, e_p_par, e_p_orth, de_p_par, de_p_orth, e_r, de_r, e_r_par, e_r_orth1, e_r_orth2 (3 each)
 *   in the key order of the reference's dictionaries.  ref p[3:] and e_r are the values of the reference's second pass (:712-752): the rotation
 *   reference integrated along the plan, and the orientation error log(R(p) R(ref)^T) against it.
 * Stages at or beyond n_valid are NaN.  A stream without a plan (error count >= N; the fused tick skips it) gets n_valid = 0 and an all-NaN
 * body.  Non-finite inputs give non-finite records.
 * Call it after bmpc_stream_post, after bmpc_stream_tick or after a graph replay of the tick, and BEFORE the next pack (which overwrites p and may
 * move the window of the path).  p and traj are the arrays of that tick, sstate the state behind its post.  After a real-time tick (flags bit 1) it
 * logs the plan traj holds: the applied or the replayed one.  All pointers are DEVICE pointers; asynchronous on hip_stream; no workspace of the
 * handle is used, so the call may also be enqueued inside a capture of the caller's stream.  BMPC_ERR_ARG on a missing array. */
int bmpc_stream_log_len(const bmpc_handle *h);      /* 88 N + 4 */
int bmpc_stream_log(bmpc_handle *h, int B, const double *path, int path_entries, const double *sstate, const double *p, const double *traj,
                    double *log, void *hip_stream);
/* Re-planning of closed-loop streams on the device: ReferencePath.__init__ (ReferencePath.py:10-163) and the state part of BoundMPC.update()
 * (BoundMPC.py:163-217) for every stream whose record carries a raised flag, one launch over the batch (host mirror, one stream at a time:
 * boundmpc_amd.stream.apply_update).  One re-plan record per stream:
 *   replan [B][bmpc_stream_replan_len] = header (32) | n_max via entries (32 each),  n_max = path_entries - S + 1
 *     header:    flag | n (via points) | nb (basis entries: the first nb bp1 / br1 are read) | p0 3 | v 3 | a 3 | jerk 3 (the linear parts of the
 *                measured Cartesian state, as update() uses them) | weights 15 | 2 pad
 *     via entry: p 3 | R 9 (rotation matrix, row-major) | p_lower 2 | p_upper 2 | r_lower 2 | r_upper 2 | bp1 3 | br1 3 | s | e_p_min | e_r_min |
 *                e_p_max | e_r_max | 1 pad
 *   (builder: boundmpc_amd.stream.replan_record).  Written for a re-planned stream: its whole block of the path table (n + S - 1 slots as
 *   ReferencePath pads its lists, the rows behind them copy the last slot), and of its state row the window start (0), the path-parameter state
 *   projected onto the new first segment, the rotation reference, phi_max, the weights, the entry count and the `updated` flag; an error count
 *   >= N goes back to N - 1, so the next tick solves a stream that had lost its plan.  The previous solution, its Cartesian arrays and dphi_max stay.
 *   flags bit 0 (set_goal) with robot != NULL: also robot[x_phi_d] = (phi_max, 0, 0), what the node does right after update()
 *   (bound_mpc_node.py:164).
 *   flags bit 1 (splice; needs robot != NULL): the words the node takes from the plant (bound_mpc_node.py:121-137,158-162) are written into every
 *   raised, valid record from the stream's robot record before it is consumed:
 *     via[0].p = p_lie[0:3] + 0.5 h v[0:3],  via[0].R = rotation matrix of the rotation vector p_lie[3:6],
 *     header p0 = p_lie[0:3], v = v[0:3], a = J ddq + dJ dq, jerk = J u + 2 dJ ddq + ddJ dq (linear rows; q, dq, ddq and u = jerk of the record).
 *   The robot record carries no Cartesian acceleration or jerk.  The node keeps both from its plant step (util_functions.py:152-161): its a is this a,
 *   its j_cart evaluates ddJ at the state before the step and uses J ddq where the kinematics say J u; the device uses the consistent derivative
 *   of a.  The difference reaches one state word, dddphi.  The spliced words stay in the record after the launch (only the flag word is cleared),
 *   so the caller can read back what was spliced.  A record whose flag is 0 and an invalid record are not spliced.
 *   flags bit 2 (poor bounds; with bit 1 only): the node's scenario 0 (:126-129): if v[2] < 0 and p_lie[1] * via[1].p[1] < 0, via[0].p[2] -= 0.05.
 *   Any other bit, bit 2 without bit 1, bit 1 without robot: BMPC_ERR_ARG.  Without bit 1 the caller splices (boundmpc_amd.stream.splice_record).
 * Flag protocol: flag == 0 leaves the stream alone, bit for bit.  A raised flag is CLEARED by the launch that consumed it, so a captured graph
 * that holds this launch re-plans only when someone raises a flag in the record buffer again.  n < 2, n > n_max, nb < 1, nb > n or a non-finite
 * n / nb: invalid record -- stream untouched, flag cleared, info[b] = 1; otherwise info[b] = 0 (info may be NULL).  Non-finite numbers elsewhere,
 * or a basis vector parallel to its direction, give non-finite table or state entries, as the host mirror does.
 * Ordering: the call belongs BETWEEN a tick's post (or log) and the next pack.  All pointers are DEVICE pointers; asynchronous on hip_stream; no
 * workspace of the handle is used, so the call may also be enqueued inside a capture of the caller's stream.  BMPC_ERR_ARG on a missing
 * replan / path / sstate, on B < 1 or on path_entries < S + 1. */
int bmpc_stream_replan_len(const bmpc_handle *h, int path_entries);      /* 32 + 32 (path_entries - S + 1); <= 0 on bad arguments */
int bmpc_stream_update(bmpc_handle *h, int B, double *replan, double *path, int path_entries, double *sstate, double *robot /* may be NULL */,
                       int *info /* may be NULL */, int flags, void *hip_stream);
/* Plant disturbance of closed-loop streams, one launch over the batch: d [B][BMPC_DIST_LEN] = delta q 7 | delta dq 7 | delta ddq 7 is added to q, dq
 * and ddq of the robot records, then p_lie and v of a record are recomputed from its disturbed joint state (the kinematics of the post, with the
 * record's jerk).  An all-zero row leaves its record untouched, bit for bit; a non-finite entry counts as 0.  The call belongs BETWEEN a tick's post
 * (or log, or update) and the next pack.  DEVICE pointers; asynchronous on hip_stream; no workspace of the handle is used, so the call may be
 * enqueued inside a capture of the caller's stream.  BMPC_ERR_ARG on a missing array or B < 1. */
enum { BMPC_DIST_LEN = 21 };
int bmpc_stream_disturb_len(void);
int bmpc_stream_disturb(bmpc_handle *h, int B, double *robot, const double *d /* [B][21] */, void *hip_stream);
/* Rollout with EVENTS: bmpc_stream_rollout (its arguments, tests and contract) with what a Monte-Carlo run needs between the ticks without a return
 * to the host -- both events sit "behind tick t of stream b" and need only the stream's own records:
 *   disturb [ticks][B][BMPC_DIST_LEN] or NULL: row [t][b] disturbs the plant of stream b behind tick t, as bmpc_stream_disturb does;
 *   replan [B][bmpc_stream_replan_len] or NULL, replan_tick [B] (required with replan): the record of stream b is consumed behind tick
 *     replan_tick[b] as bmpc_stream_update(update_flags) consumes it -- with bit 1 the state behind that tick is spliced in on the device, where
 *     alone it is known.  One re-plan per stream and launch here; a queue of them per stream, each fired by a tick, by the goal of its leg or by a
 *     lost plan, is bmpc_stream_rollout_legs (below): several legs are one rollout.  The path table is written then (the const of `path` is the
 *     plain rollout's).
 * Per stream and tick: pack, solve, post, the hist and traj_hist rows (as in the rollout: hist[t][b] shows the UNDISTURBED plant behind tick t),
 * the disturbance, the re-plan, the goal test, the next tick's lost-plan test.  So a re-plan behind the tick that reaches the old goal gives the
 * stream a new phi_max and it goes on (a second leg), and a re-plan behind the post that exhausted the plan (error count back to N - 1) rescues the
 * stream.  Stops win over events: a stream that stops before its replan_tick -- lost on entry or at the start of an earlier tick, or at its goal --
 * never consumes its record: the flag stays raised and replan_info[b] = -1; the same for replan_tick[b] < 0 or >= ticks.  Otherwise replan_info[b]
 * (may be NULL) is what bmpc_stream_update writes: 0 consumed (or a record whose flag was 0), 1 invalid record (stream untouched, flag cleared).
 * With goal_tol = 0 every tick array, the path table, the record buffer, hist, traj_hist and ticks_run hold afterwards what this loop leaves, bit
 * for bit, events applied to the streams that still run:
 *   for t in 0..ticks-1: bmpc_stream_tick on one wave per stream; bmpc_stream_disturb(rows of tick t);
 *                        bmpc_stream_update(update_flags) with exactly the flags of the streams whose replan_tick == t raised
 * BMPC_ERR_ARG, nothing launched: what the rollout refuses, replan without replan_tick, update_flags as bmpc_stream_update refuses them
 * (update_flags without replan are checked and otherwise ignored). */
int bmpc_stream_rollout_events(bmpc_handle *h, int B, int ticks, const double *path, int path_entries, double *sstate, double *robot, double *p, double *x0,
                               double *dual_state, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                               double goal_tol, double *hist, double *traj_hist, int *ticks_run, double *replan /* or NULL */,
                               const int *replan_tick /* [B]; required with replan */, int *replan_info /* [B] or NULL */, int update_flags,
                               const double *disturb /* [ticks][B][21] or NULL */, void *hip_stream);
/* The error bound, measured on the device: how far is the MEASURED state of a tick outside its tubes and its joint limits?  One row per stream from
 * the parameter vector p a pack (or a tick) left behind -- the five tube rows of the OCP (rows 38..42 of a stage) evaluated at NODE 0, the state
 * the plant is in: segment selected by phi0 against phi_switch, the tube quartics at phi0 - phi_switch[segment], the position error
 * p0 - (pref + dpref x) along bp1 / bp2 (which never select the last window segment), the orientation rows from the packed initial errors of the
 * segment (host mirror and specification: boundmpc_amd.stream.tube_excess_of_state), and q0, dq0 against the reference's joint limits (those of the
 * inequality rows, without bound_margin):
 *   tube [B][BMPC_TUBE_LEN] = l 5 | w 5 | ex_pos | ex_rot | ex_q | ex_dq | segment | phi0
 *     l, w    the rows in the linear form, |l| <= |w| inside (the OCP's rows are l^2 - w^2), in row order: orientation tangential, position bp1,
 *             position bp2, orientation br1, orientation br2
 *     ex_pos  max over the two position rows of |l| - |w|, metres; <= 0: inside.  ex_rot: the same over the three orientation rows, radians
 *     ex_q    max over the joints of |q0_j| - qlim_j;  ex_dq: max of |dq0_j| - dqlim_j
 * Non-finite inputs give non-finite slots (a maximum with a NaN among its terms is NaN), never a fault: the segment is clamped to 0..S-1 before it
 * addresses anything.  sstate may be NULL; where it is given, a stream without a plan (error count not in 0..N-1: the fused tick skips it, its p is
 * stale) gets an all-NaN row.  The call belongs BEHIND a pack or a tick and BEFORE the next pack; behind a tick it measures the state that tick
 * started from.  One launch over the batch, one wave per stream.  DEVICE pointers; asynchronous on hip_stream; no workspace of the handle is used, so
 * the call may be enqueued inside a capture of the caller's stream.  BMPC_ERR_ARG on a missing p or tube or on B < 1. */
enum { BMPC_TUBE_L = 0 /* 5 */, BMPC_TUBE_W = 5 /* 5 */, BMPC_TUBE_EX_POS = 10, BMPC_TUBE_EX_ROT = 11, BMPC_TUBE_EX_Q = 12, BMPC_TUBE_EX_DQ = 13,
       BMPC_TUBE_SEG = 14, BMPC_TUBE_PHI = 15, BMPC_TUBE_LEN = 16 };
int bmpc_stream_tube_len(void);
int bmpc_stream_tube(bmpc_handle *h, int B, const double *p, const double *sstate /* may be NULL */, double *tube /* [B][16] */, void *hip_stream);
/* Rollout with the AUDIT: bmpc_stream_rollout_events (its arguments in their order, its tests and contract; NULL event pointers switch the events off)
 * that also answers what a Monte-Carlo run asks -- did the plant leave its tube, when, and by how much?  Behind the pack of tick t the row of
 * bmpc_stream_tube is taken from the stream's p:
 *   tube_hist [ticks][B][BMPC_TUBE_LEN] or NULL: row [t][b] is the state tick t of stream b STARTS from -- the plant behind tick t - 1 with that
 *     tick's disturbance and re-plan applied, which is what a host loop measures on the p of every tick.  Rows of ticks the stream did not run are NaN,
 *     as in hist.  The state behind the LAST tick a stream runs is seen by the first pack of the next launch, not by this one.
 *   audit [B][BMPC_AUDIT_LEN] or NULL, initialised by the kernel: SAMPLES ticks audited; MAX_POS, TICK_POS the largest position excess and its (first)
 *     tick, MAX_ROT, TICK_ROT likewise; MAX_Q, MAX_DQ the largest joint figures; N_POS, N_ROT samples whose excess is > audit_tol; N_JOINT samples with
 *     ex_q or ex_dq > 1e-9; FIRST_OUT the first tick with a position or an orientation excess > audit_tol, -1 for none; one pad word.  A non-finite
 *     excess makes its maximum NaN for good and counts as outside.  A stream lost on entry has SAMPLES 0, maxima -inf, ticks and FIRST_OUT -1.
 * The audit changes nothing else: every other array holds what bmpc_stream_rollout_events leaves, bit for bit.  With tube_hist and audit both NULL
 * the call IS bmpc_stream_rollout_events.  BMPC_ERR_ARG, nothing launched: a negative or non-finite audit_tol, and what that entry refuses. */
enum { BMPC_AUDIT_SAMPLES = 0, BMPC_AUDIT_MAX_POS = 1, BMPC_AUDIT_TICK_POS = 2, BMPC_AUDIT_MAX_ROT = 3, BMPC_AUDIT_TICK_ROT = 4, BMPC_AUDIT_MAX_Q = 5,
       BMPC_AUDIT_MAX_DQ = 6, BMPC_AUDIT_N_POS = 7, BMPC_AUDIT_N_ROT = 8, BMPC_AUDIT_N_JOINT = 9, BMPC_AUDIT_FIRST_OUT = 10, BMPC_AUDIT_LEN = 12 };
int bmpc_stream_rollout_audit(bmpc_handle *h, int B, int ticks, const double *path, int path_entries, double *sstate, double *robot, double *p, double *x0,
                              double *dual_state, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                              double goal_tol, double *hist, double *traj_hist, int *ticks_run, double *replan /* or NULL */,
                              const int *replan_tick /* [B]; required with replan */, int *replan_info /* [B] or NULL */, int update_flags,
                              const double *disturb /* [ticks][B][21] or NULL */, double *tube_hist /* [ticks][B][16] or NULL */,
                              double *audit /* [B][12] or NULL */, double audit_tol, void *hip_stream);
/* Rollout with the LOG: bmpc_stream_rollout_audit (every argument up to audit_tol in its order, its tests and contract; NULL event and audit pointers
 * switch those off) that also answers what the reference's plots are about -- how well did the loop track the path, tick by tick, in the path frame?
 * Behind the post of tick t, AHEAD of that tick's disturbance and re-plan, the record of bmpc_stream_log is taken from the stream's path table, state
 * row, p and traj -- the window between a tick's post and the next pack, which inside a rollout exists on the device only:
 *   log_hist [ticks][B][88 log_stages + 4] or NULL: row [t][b] = [log_stages][88] | n_valid | error_count | 2 pad, the first log_stages (1..N) stages of
 *     the row bmpc_stream_log writes when called right behind bmpc_stream_tick (stage layout there), with the n_valid of the WHOLE plan, not clipped
 *     to log_stages.  Stages at or beyond n_valid are NaN; a tick whose post exhausted the plan gives n_valid = 0 and a NaN body.  The row of a
 *     re-plan tick is taken before the table is rewritten.  Rows of ticks the stream did not run are NaN, trailer included, as in hist.
 *   track [B][BMPC_TRACK_LEN] or NULL, initialised by the kernel, over STAGE 0 of every row -- the state the plant is in behind the tick (the robot
 *     record of hist[t][b], ahead of the tick's disturbance); a tick is a sample when the stream ran it and its row has n_valid >= 1: SAMPLES their
 *     number; MAX_EP_ORTH the largest ||e_p_orth|| (metres), TICK_EP_ORTH its first tick, SUMSQ_EP_ORTH the sum of its squares in tick order (rms =
 *     sqrt(sumsq / samples)); the same three for e_p_par and for e_r (radians; the value of the log's second pass); REPLAYED the samples whose
 *     trajectory record says using_previous; one pad word.  A norm is sqrt((x x + y y) + z z).  A non-finite norm makes its maximum NaN for good.  A
 *     stream lost on entry has SAMPLES 0, maxima -inf, ticks -1, sums 0.
 * The log changes nothing else: every other array holds what bmpc_stream_rollout_audit leaves, bit for bit.  With log_hist and track both NULL the call
 * IS bmpc_stream_rollout_audit (log_stages is not looked at).  With goal_tol = 0 log_hist holds what this loop leaves, cut to log_stages:
 *   for t in 0..ticks-1: bmpc_stream_tick on one wave per stream; bmpc_stream_log; bmpc_stream_disturb(rows of tick t); bmpc_stream_update of the
 *                        records due
 * BMPC_ERR_ARG, nothing launched: log_stages outside 1..N while log_hist or track is given, and what that entry refuses. */
enum { BMPC_TRACK_SAMPLES = 0, BMPC_TRACK_MAX_EP_ORTH = 1, BMPC_TRACK_TICK_EP_ORTH = 2, BMPC_TRACK_SUMSQ_EP_ORTH = 3, BMPC_TRACK_MAX_EP_PAR = 4,
       BMPC_TRACK_TICK_EP_PAR = 5, BMPC_TRACK_SUMSQ_EP_PAR = 6, BMPC_TRACK_MAX_ER = 7, BMPC_TRACK_TICK_ER = 8, BMPC_TRACK_SUMSQ_ER = 9,
       BMPC_TRACK_REPLAYED = 10, BMPC_TRACK_LEN = 12 };
int bmpc_stream_track_len(void);
int bmpc_stream_rollout_log_len(const bmpc_handle *h, int log_stages);      /* 88 log_stages + 4; <= 0 on bad arguments (log_stages outside 1..N) */
int bmpc_stream_rollout_log(bmpc_handle *h, int B, int ticks, const double *path, int path_entries, double *sstate, double *robot, double *p, double *x0,
                            double *dual_state, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                            double goal_tol, double *hist, double *traj_hist, int *ticks_run, double *replan /* or NULL */,
                            const int *replan_tick /* [B]; required with replan */, int *replan_info /* [B] or NULL */, int update_flags,
                            const double *disturb /* [ticks][B][21] or NULL */, double *tube_hist /* [ticks][B][16] or NULL */,
                            double *audit /* [B][12] or NULL */, double audit_tol, double *log_hist /* [ticks][B][88 log_stages + 4] or NULL */,
                            int log_stages, double *track /* [B][12] or NULL */, void *hip_stream);
/* Rollout with a MISSION: bmpc_stream_rollout_log (its arguments in their order up to and including track, their meaning, tests and contract; NULL
 * event, audit and log pointers switch those off) with a QUEUE of re-plan records per stream in the place of the one scheduled record -- task
 * sequences ("follow leg A; once there, take leg B; once there, leg C") and recovery policies ("if the plan is lost, re-plan from where the plant
 * is") in ONE launch.  Both triggers are facts of the stream's own state, known on the device only, and every stream meets them on another tick; a
 * chain of rollouts with goal_tol, each followed by bmpc_stream_update, waits for the slowest stream of the batch once per leg.  replan_tick is gone,
 * replan and replan_info grow an axis:
 *   legs       >= 1: records per stream
 *   replan     [B][legs][bmpc_stream_replan_len] or NULL: record k of stream b, in the layout of bmpc_stream_update with its flag protocol
 *   leg_tick   [B][legs]: a tick number >= 0, or negative for "no tick condition"
 *   leg_on     [B][legs]: bit 0 BMPC_LEG_AT_GOAL, bit 1 BMPC_LEG_ON_LOST
 *   leg_tol    [B][legs] or NULL: the goal tolerance of record k; NULL means goal_tol for every record
 *   legs_done  [B], required with replan, initialised by the kernel: the number of records the stream consumed
 *   leg_fired  [B][legs] or NULL: the tick behind which record k was consumed; -1 if never
 *   leg_why    [B][legs] or NULL: the conditions that held when it fired -- BMPC_LEG_WHY_GOAL | _LOST | _TICK; 0 if never
 *   replan_info [B][legs] or NULL: what bmpc_stream_update writes for that record; -1 if never consumed
 * Only the HEAD of the queue can fire: record k = legs_done[b] while k < legs.  It is due behind tick t when any of its enabled conditions holds:
 *   leg_tick >= 0 and t >= leg_tick (AT OR AFTER its tick: a record queued behind a late one still fires);
 *   bit 0 and phi_max - phi <= leg_tol (the state row behind the tick's post: the goal of the leg the stream is on);
 *   bit 1 and error count >= N (the post of this tick exhausted the plan).
 * A record with no tick condition and neither bit, or with any higher bit set, ENDS the queue: it and everything behind it are never consumed (the
 * trigger words live on the device and are not validated on the host).  At most one record is consumed per stream and tick.
 * The due record is consumed where the single re-plan of bmpc_stream_rollout_events sits: behind the tick's history and log rows and its disturbance,
 * ahead of the goal test and of the next tick's lost-plan test -- with update_flags bit 1 spliced from the robot record of that moment, then updated.
 * A due record whose flag is 0 or which is invalid is consumed as bmpc_stream_update consumes it (info 0 or 1, stream untouched) and the head still
 * advances.  So a goal-triggered record gives the stream a new phi_max before the goal test sees the old one -- with goal_tol > 0 a stream stops only
 * at the goal of its LAST leg --, and an on-lost record rescues the stream before the lost-plan stop.  Stops still win over records that are not yet
 * due: their flags stay raised.  The audit and the tracking record keep accumulating over the whole mission; per-leg spans follow from leg_fired.
 * With goal_tol = 0 every array the contract of bmpc_stream_rollout_log names, the record buffer and the path tables hold what this loop leaves, bit
 * for bit:
 *   for t in 0..ticks-1: bmpc_stream_tick on one wave per stream; bmpc_stream_log; bmpc_stream_disturb(rows of tick t);
 *                        bmpc_stream_update(update_flags) with exactly the flags of the streams whose head record is due raised
 * legs = 1, leg_on = 0, leg_tick = replan_tick in 0..ticks-1 IS bmpc_stream_rollout_log, bit for bit.  With replan == NULL the call is
 * bmpc_stream_rollout_log without a re-plan, and the queue arguments are not looked at.  Waves per stream: bmpc_set_rollout_waves, as for the others.
 * BMPC_ERR_ARG, nothing launched: what bmpc_stream_rollout_log refuses, replan without leg_tick, leg_on or legs_done, legs < 1 with replan. */
enum { BMPC_LEG_AT_GOAL = 1, BMPC_LEG_ON_LOST = 2, BMPC_LEG_WHY_GOAL = 1, BMPC_LEG_WHY_LOST = 2, BMPC_LEG_WHY_TICK = 4 };
int bmpc_stream_rollout_legs(bmpc_handle *h, int B, int ticks, const double *path, int path_entries, double *sstate, double *robot, double *p, double *x0,
                             double *dual_state, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                             double goal_tol, double *hist, double *traj_hist, int *ticks_run, double *replan /* [B][legs][len] or NULL */,
                             int *replan_info /* [B][legs] or NULL */, int update_flags, const double *disturb /* [ticks][B][21] or NULL */,
                             double *tube_hist /* [ticks][B][16] or NULL */, double *audit /* [B][12] or NULL */, double audit_tol,
                             double *log_hist /* [ticks][B][88 log_stages + 4] or NULL */, int log_stages, double *track /* [B][12] or NULL */,
                             int legs, const int *leg_tick /* [B][legs] */, const int *leg_on /* [B][legs] */, const double *leg_tol /* [B][legs] or NULL */,
                             int *legs_done /* [B] */, int *leg_fired /* [B][legs] or NULL */, int *leg_why /* [B][legs] or NULL */, void *hip_stream);
/* Rollout for SWEEPS: bmpc_stream_rollout_legs (its arguments in their order up to and including leg_why, their meaning, tests and contract; NULL
 * event, audit, log and queue pointers switch those off) with a TABLE of controller settings per stream in the place of the one set the handle carries
 * for a whole launch -- a grid over (level rule, cap, margin, acceptance), or a robustness battery with its own joint-limit margin per stream, is ONE
 * launch of as many streams, not as many handles with as many workspaces:
 *   tune       [B][BMPC_TUNE_LEN] or NULL, DEVICE: row b, slots BMPC_TUNE_*; the two words behind BMPC_TUNE_STALL_WINDOW are pad and never looked at
 *   tune_info  [B] or NULL: 0 = row b was valid and the stream ran; else the bit mask of its invalid slots (bit k = slot k, bit 15 = the level rule
 *              as resolved, below)
 *   tune_used  [B][BMPC_TUNE_LEN] or NULL: the row as resolved, pad words 0; for an invalid row the row as resolved too, the refused values as given
 * A slot that holds NaN takes the handle's value AS THE LAUNCH READS IT (for BMPC_TUNE_MAX_ITER the max_iter argument when it is > 0, else
 * options.max_iter).  Any other value replaces it for every tick of stream b and for nothing else:
 *   MAX_ITER, TOL, MU_INIT, MU_WARM, MU_MIN_FAC, SLACK_PUSH, BOUND_MARGIN, STALL_WINDOW   the options of bmpc_create of the same names, in every solve
 *   HOLD                                bmpc_set_barrier_hold, in every solve
 *   LVL_C, LVL_LO, LVL_HI               bmpc_stream_set_level_rule, in every pack
 *   RT_TOL, RT_ROW_CAP                  bmpc_stream_set_rt_feasibility_tol, bmpc_stream_set_rt_position_row_cap, in every post
 * The restoration mode, its short-step count and cap, the Hessian choice, the tick flags and the waves per stream stay the handle's.
 * A slot that is not NaN is valid when it passes the test that guards the same value in bmpc_create or in its setter: finite; MAX_ITER an integer in
 * 1..100000; TOL, MU_INIT, MU_WARM, MU_MIN_FAC, SLACK_PUSH, RT_TOL > 0; BOUND_MARGIN in [0, 0.5]; HOLD 0 or 1; LVL_C, LVL_LO, LVL_HI, RT_ROW_CAP >= 0;
 * STALL_WINDOW an even integer >= 0.  One test runs across slots, on the row as resolved: LVL_HI > 0 needs 0 < LVL_LO <= LVL_HI.
 * The table lives on the device, so it is validated there, as the trigger words of a mission are.  A row with an invalid slot DOES NOT RUN -- a sweep
 * never runs silently on a default: ticks_run[b] = 0, the rows of stream b in every history array are NaN, its audit and tracking records are those of
 * a stream lost on entry, legs_done[b] = 0 and its records keep their flags, and its tick arrays -- status, iters and kkt included -- keep every bit.
 * Every other stream is served as if the row were not there.
 * With tune == NULL the call IS bmpc_stream_rollout_legs, and tune_info and tune_used are not looked at.  With a table of NaN it leaves what that
 * entry leaves, bit for bit.  Otherwise every array of stream b holds what the same call without a table leaves for the one-stream batch {b} on a
 * handle whose options and setters carry tune_used[b], bit for bit, on one wave per stream or on teams (bmpc_set_rollout_waves, as for the others): a
 * stream's result does not depend on the batch it is in nor on the workgroup that serves it.
 * bmpc_stream_tune_defaults writes the row an all-NaN row resolves to on this handle with this max_iter argument (HOST, BMPC_TUNE_LEN doubles).
 * BMPC_ERR_ARG, nothing launched: what bmpc_stream_rollout_legs refuses; bmpc_stream_tune_defaults: no handle, max_iter < 0, no row. */
enum { BMPC_TUNE_MAX_ITER = 0, BMPC_TUNE_TOL, BMPC_TUNE_MU_INIT, BMPC_TUNE_MU_WARM, BMPC_TUNE_MU_MIN_FAC, BMPC_TUNE_SLACK_PUSH, BMPC_TUNE_BOUND_MARGIN,
       BMPC_TUNE_HOLD, BMPC_TUNE_LVL_C, BMPC_TUNE_LVL_LO, BMPC_TUNE_LVL_HI, BMPC_TUNE_RT_TOL, BMPC_TUNE_RT_ROW_CAP, BMPC_TUNE_STALL_WINDOW,
       BMPC_TUNE_LEN = 16 };      /* two pad words, never looked at */
int bmpc_stream_tune_len(void);
int bmpc_stream_tune_defaults(const bmpc_handle *h, int max_iter, double *row /* HOST [BMPC_TUNE_LEN] */);
int bmpc_stream_rollout_tuned(bmpc_handle *h, int B, int ticks, const double *path, int path_entries, double *sstate, double *robot, double *p, double *x0,
                              double *dual_state, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                              double goal_tol, double *hist, double *traj_hist, int *ticks_run, double *replan /* [B][legs][len] or NULL */,
                              int *replan_info /* [B][legs] or NULL */, int update_flags, const double *disturb /* [ticks][B][21] or NULL */,
                              double *tube_hist /* [ticks][B][16] or NULL */, double *audit /* [B][12] or NULL */, double audit_tol,
                              double *log_hist /* [ticks][B][88 log_stages + 4] or NULL */, int log_stages, double *track /* [B][12] or NULL */,
                              int legs, const int *leg_tick /* [B][legs] */, const int *leg_on /* [B][legs] */, const double *leg_tol /* [B][legs] or NULL */,
                              int *legs_done /* [B] */, int *leg_fired /* [B][legs] or NULL */, int *leg_why /* [B][legs] or NULL */,
                              const double *tune /* [B][BMPC_TUNE_LEN] or NULL */, int *tune_info /* [B] or NULL */,
                              double *tune_used /* [B][BMPC_TUNE_LEN] or NULL */, void *hip_stream);
/* Rollout with a PLANT MODEL: bmpc_stream_rollout_tuned (its arguments in their order up to and including tune_used, their meaning, tests and contract;
 * NULL event, audit, log, queue and settings pointers switch those off) with a TABLE of actuator models per stream.  In every other rollout the plant IS
 * the model: the post moves the robot record with the model's own integrator chain and the planned jerk, and the only deviation is the additive disturb
 * table, which cannot depend on what the controller commands.  Here a drive stands between the first planned jerk c of every tick and the plant:
 *   plant       [B][BMPC_PLANT_LEN] or NULL, DEVICE: row b, slots BMPC_PLANT_*; the three words behind BMPC_PLANT_DELAY are pad and never looked at
 *                 GAIN[7]   actuator gain of joint j                                   identity 1       valid when finite
 *                 BIAS[7]   jerk offset, rad/s^3                                       identity 0       valid when finite
 *                 LAG       first-order response per tick, u_act += LAG (a - u_act)    identity 1       valid when 0 < LAG <= 1
 *                 SAT       jerk magnitude the drive delivers                          identity +inf    valid when > 0 (+inf allowed)
 *                 DELAY     1: the command applied is the previous tick's              identity 0       valid when 0 or 1
 *               a NaN slot takes its identity value
 *   plant_state [B][BMPC_PLANT_STATE_LEN], required with plant, IN AND OUT so that rollouts chain: ACT[7] the lag's state, CMD[7] the previous command,
 *               two pad words; a stream at rest starts from ACT = CMD = the jerk of its robot record
 *   plant_info  [B] or NULL: 0 = row b was valid and the stream ran; else the bit mask of its invalid slots (bit k = slot k)
 *   plant_rec   [B][BMPC_PLANT_REC_LEN] or NULL, initialised by the call: SAMPLES the plant steps taken, N_SAT the ticks on which some joint clipped,
 *               MAX_DU the largest |u - c| with TICK_DU and JOINT_DU its first tick and joint, SUMSQ_DU the sum of (u - c)^2 in tick order, joints
 *               0..6 inside a tick, two pad words; a stream without a step: SAMPLES 0, MAX_DU -inf, TICK_DU and JOINT_DU -1, sums 0; a non-finite |u - c|
 *               makes MAX_DU NaN for good
 * The step, behind every post that stepped the plant (a tick whose post exhausted the plan takes none), per joint j with c_j the first planned jerk:
 *   c' = DELAY ? CMD_j : c_j;  CMD_j = c_j;  a = GAIN_j c' + BIAS_j;  f = LAG == 1 ? a : ACT_j + LAG (a - ACT_j);  ACT_j = f;
 *   u = f > SAT ? SAT : f < -SAT ? -SAT : f  (a NaN passes);  D = u - c_j;
 *   q_j += h^3/24 D;  dq_j += h^2/6 D;  ddq_j += h/2 D;  the record's jerk_j = u
 * -- the coefficients of the new jerk in the model's chain, which is linear: exactly the plant ramped from the old true jerk to u instead of to c.  Where
 * any D != 0, p_lie and v of the robot record are recomputed from the new joint state, as bmpc_stream_disturb does; where every D == 0 the record
 * keeps every bit.  Non-finite words give non-finite records.
 * The step sits AHEAD of the history, trajectory and log rows of its tick and of the tick's disturbance and re-plan: hist[t][b] shows the TRUE plant
 * behind tick t, a disturbance acts on the true plant, a spliced re-plan takes the true state, the next pack and the audit row of tick t + 1 measure it.
 * THE LOG ROWS AND THE TRACKING RECORD KEEP DESCRIBING THE PLAN, NOT THE PLANT -- stage 0 of a trajectory record comes from the plan --: the measurement
 * of the plant is the audit (tube_hist, audit).
 * The table lives on the device, so it is validated there.  A row with an invalid slot DOES NOT RUN and gets the treatment of an invalid tune row:
 * ticks_run[b] = 0, NaN history rows, the records of a stream lost on entry, untouched tick arrays and plant_state, its mask in plant_info[b]; every
 * other stream is served as if the row were not there.
 * With plant == NULL the call IS bmpc_stream_rollout_tuned, and no plant argument is looked at.  With a table of NaN or of identity values every array
 * that entry names holds what it leaves, bit for bit, and plant_state holds the commands.  With goal_tol = 0 every array, plant_state and plant_rec hold
 * what this loop leaves, bit for bit:
 *   for t in 0..ticks-1: bmpc_stream_tick on one wave per stream; bmpc_stream_plant(tick t); bmpc_stream_log; bmpc_stream_disturb(rows of tick t);
 *                        bmpc_stream_update of the head records due
 * bmpc_stream_plant is that step on its own, one launch over the batch, for per-tick loops: between a tick (or post) and bmpc_stream_log.  It skips a
 * stream whose sstate error count is >= N; for an invalid row it writes the mask and touches nothing; plant_rec (or NULL) is ACCUMULATED, not
 * initialised.  It uses no workspace of the handle and may sit inside a capture of the caller's stream, like bmpc_stream_disturb.
 * BMPC_ERR_ARG, nothing launched: what bmpc_stream_rollout_tuned refuses, and plant without plant_state; bmpc_stream_plant: no handle, B < 1, no robot,
 * sstate, plant or plant_state. */
enum { BMPC_PLANT_GAIN = 0, BMPC_PLANT_BIAS = 7, BMPC_PLANT_LAG = 14, BMPC_PLANT_SAT = 15, BMPC_PLANT_DELAY = 16, BMPC_PLANT_LEN = 20 };      /* three pad words */
enum { BMPC_PLANT_STATE_ACT = 0, BMPC_PLANT_STATE_CMD = 7, BMPC_PLANT_STATE_LEN = 16 };                                                   /* two pad words */
enum { BMPC_PLANT_REC_SAMPLES = 0, BMPC_PLANT_REC_N_SAT, BMPC_PLANT_REC_MAX_DU, BMPC_PLANT_REC_TICK_DU, BMPC_PLANT_REC_JOINT_DU, BMPC_PLANT_REC_SUMSQ_DU,
       BMPC_PLANT_REC_LEN = 8 };                                                                                                            /* two pad words */
int bmpc_stream_plant_len(void);
int bmpc_stream_plant_state_len(void);
int bmpc_stream_plant_rec_len(void);
int bmpc_stream_rollout_plant(bmpc_handle *h, int B, int ticks, const double *path, int path_entries, double *sstate, double *robot, double *p, double *x0,
                              double *dual_state, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                              double goal_tol, double *hist, double *traj_hist, int *ticks_run, double *replan /* [B][legs][len] or NULL */,
                              int *replan_info /* [B][legs] or NULL */, int update_flags, const double *disturb /* [ticks][B][21] or NULL */,
                              double *tube_hist /* [ticks][B][16] or NULL */, double *audit /* [B][12] or NULL */, double audit_tol,
                              double *log_hist /* [ticks][B][88 log_stages + 4] or NULL */, int log_stages, double *track /* [B][12] or NULL */,
                              int legs, const int *leg_tick /* [B][legs] */, const int *leg_on /* [B][legs] */, const double *leg_tol /* [B][legs] or NULL */,
                              int *legs_done /* [B] */, int *leg_fired /* [B][legs] or NULL */, int *leg_why /* [B][legs] or NULL */,
                              const double *tune /* [B][BMPC_TUNE_LEN] or NULL */, int *tune_info /* [B] or NULL */,
                              double *tune_used /* [B][BMPC_TUNE_LEN] or NULL */, const double *plant /* [B][BMPC_PLANT_LEN] or NULL */,
                              double *plant_state /* [B][BMPC_PLANT_STATE_LEN] */, int *plant_info /* [B] or NULL */,
                              double *plant_rec /* [B][BMPC_PLANT_REC_LEN] or NULL */, void *hip_stream);
int bmpc_stream_plant(bmpc_handle *h, int B, double *robot, const double *sstate, const double *plant /* [B][BMPC_PLANT_LEN] */,
                      double *plant_state /* [B][BMPC_PLANT_STATE_LEN] */, int *plant_info /* [B] or NULL */,
                      double *plant_rec /* [B][BMPC_PLANT_REC_LEN] or NULL, accumulated, not initialised */, int tick, void *hip_stream);
/* Rollout with a SENSOR MODEL: bmpc_stream_rollout_plant (its arguments in their order up to and including plant_rec, their meaning, tests and contract;
 * NULL event, audit, log, queue, settings and plant pointers switch those off) with a TABLE of measurement models per stream.  In every other rollout the
 * pack of a tick reads the robot record, and the record IS the plant: the controller measures the true state exactly.  The disturb table cannot stand in
 * for a sensor: it moves the plant, and the next pack measures the moved plant exactly.  Here a sensor stands between the plant and what the pack, the
 * solve and the post of a tick read:
 *   sensor       [B][BMPC_SENSOR_LEN] or NULL, DEVICE: row b, slots BMPC_SENSOR_*; the four words behind BMPC_SENSOR_HOLD are pad and never looked at
 *                  BIAS[7]          encoder offset of joint j, rad                          identity 0       valid when finite
 *                  RES              quantisation step of the joint positions, rad           identity 0       valid when finite and >= 0 (0: none)
 *                  NQ, NDQ, NDDQ    scale of the tick's noise row on q, dq, ddq             identity 0       valid when finite and >= 0
 *                  HOLD             1: the controller sees the previous tick's sample       identity 0       valid when 0 or 1
 *                a NaN slot takes its identity value
 *   sensor_state [B][BMPC_SENSOR_STATE_LEN], required with sensor, IN AND OUT so that rollouts chain; all zeros = fresh: HELD[21] the sample taken last
 *                (q, dq, ddq), HAS 1 once there is one, SAME 1 where the sample handed out last equalled the truth, a pad word, TRUTH[40] the words q..v
 *                [33] and jerk [7] of the robot record while a tick is in flight
 *   sensor_info  [B] or NULL: 0 = row b was valid and the stream ran; else the bit mask of its invalid slots (bit k = slot k)
 *   sensor_rec   [B][BMPC_SENSOR_REC_LEN] or NULL, initialised by the call: SAMPLES the samples taken, MAX_DQ the largest |q_m - q| with TICK_DQ and
 *                JOINT_DQ its first tick and joint, MAX_DP the largest ||p_m - p|| (metres, position part of p_lie) with TICK_DP its first tick, SUMSQ_DQ
 *                the sum of (q_m - q)^2 in tick order, joints 0..6 inside a tick, a pad word; q_m, p_m: what the controller was handed (under HOLD the
 *                sample of the tick before); a stream without a sample: SAMPLES 0, MAX_* -inf, TICK_* and JOINT_DQ -1, sum 0; a non-finite
 *                difference makes its MAX NaN for good
 *   sensor_noise [ticks][B][21] or NULL (zeros), DEVICE: unit draws made by the caller, delta q 7 | delta dq 7 | delta ddq 7 of tick t of stream b; a
 *                non-finite word counts as 0, as in bmpc_stream_disturb
 *   meas_hist    [ticks][B][robot record] or NULL: the robot record the pack of tick t read; NaN rows for the ticks a stream did not run
 * The sample of tick t, behind the lost-plan test and ahead of the pack, per joint j with n the tick's noise row:
 *   m_q = (q_j + BIAS_j) + NQ n_j;  RES > 0: m_q = RES rint(m_q / RES) (half to even);  m_dq = dq_j + NDQ n_{7+j};  m_ddq = ddq_j + NDDQ n_{14+j};
 *   out = (HOLD == 1 and HAS) ? HELD : m;  HELD = m;  HAS = 1;  SAME = every word of out compares equal to the truth's
 * Where SAME == 0 the robot record's q, dq, ddq become out and its p_lie and v are recomputed from them as bmpc_stream_disturb does (jerk and x_phi_d are
 * kept); where SAME == 1 the record keeps every bit.  The way back, behind the post and ahead of the plant step: SAME == 1: nothing, the post has
 * stepped the truth itself.  Else, where the post stepped the record (error count < N behind it): the TRUE q, dq, ddq take the model's chain step from
 * the true jerk to the first planned jerk c the post has stored, p_lie and v follow, the jerk is c -- the post's step on the true plant.  Else (the post
 * exhausted the plan and did not step) the words q..v are the truth's again.
 * WHAT EACH OUTPUT THEN DESCRIBES.  hist, robot behind the call, what disturb acts on, what the plant step corrects, what a spliced re-plan takes and what
 * the next launch starts from: the TRUTH.  p, the tube rows and the audit (taken from the pack's p), traj, the log rows and the tracking record: the
 * MEASUREMENT and the plan made from it -- what the controller's own monitor would report.  meas_hist is the measurement itself, and MAX_DP of the record
 * bounds what the audit's position excess can miss.  An audit of the truth's orientation rows would need the pack's orientation decomposition at the true
 * pose, and a splice from the measurement instead of the truth is not offered either.
 * An invalid row gets the treatment of an invalid plant row: no tick, NaN history rows, its mask in sensor_info[b], sensor_state untouched.
 * With sensor == NULL the call IS bmpc_stream_rollout_plant, and no sensor argument is looked at.  With a table of NaN or of identity values every array
 * that entry names holds what it leaves, bit for bit.  With goal_tol = 0 every array, sensor_state and sensor_rec hold what this loop leaves, bit for bit:
 *   for t in 0..ticks-1: bmpc_stream_sense(tick t, noise rows of tick t); bmpc_stream_tick on one wave per stream; bmpc_stream_unsense;
 *                        bmpc_stream_plant(tick t); bmpc_stream_log; bmpc_stream_disturb(rows of tick t); bmpc_stream_update of the head records due
 * bmpc_stream_sense and bmpc_stream_unsense are the two steps on their own, one launch over the batch each, for per-tick loops: around a tick (or pack ..
 * post).  The sample: for an invalid row it writes the mask and touches nothing; a stream whose sstate error count is >= N (the tick will skip it) takes no
 * sample, and SAME = 1 is written so that the way back leaves it alone; sensor_noise is ONE row per stream [B][21]; meas (or NULL) [B][robot record] is
 * the record the pack will read; sensor_rec (or NULL) is ACCUMULATED, not initialised.  Neither uses workspace of the handle; both may sit inside a
 * capture of the caller's stream, like bmpc_stream_plant.
 * BMPC_ERR_ARG, nothing launched: what bmpc_stream_rollout_plant refuses, and sensor without sensor_state; the two steps: no handle, B < 1, no robot,
 * sstate, sensor or sensor_state. */
enum { BMPC_SENSOR_BIAS = 0, BMPC_SENSOR_RES = 7, BMPC_SENSOR_NQ = 8, BMPC_SENSOR_NDQ = 9, BMPC_SENSOR_NDDQ = 10, BMPC_SENSOR_HOLD = 11, BMPC_SENSOR_LEN = 16 };      /* four pad words */
enum { BMPC_SENSOR_STATE_HELD = 0, BMPC_SENSOR_STATE_HAS = 21, BMPC_SENSOR_STATE_SAME = 22, BMPC_SENSOR_STATE_TRUTH = 24, BMPC_SENSOR_STATE_LEN = 64 };              /* one pad word */
enum { BMPC_SENSOR_REC_SAMPLES = 0, BMPC_SENSOR_REC_MAX_DQ, BMPC_SENSOR_REC_TICK_DQ, BMPC_SENSOR_REC_JOINT_DQ, BMPC_SENSOR_REC_MAX_DP, BMPC_SENSOR_REC_TICK_DP,
       BMPC_SENSOR_REC_SUMSQ_DQ, BMPC_SENSOR_REC_LEN = 8 };                                                                                                        /* one pad word */
int bmpc_stream_sensor_len(void);
int bmpc_stream_sensor_state_len(void);
int bmpc_stream_sensor_rec_len(void);
int bmpc_stream_rollout_sensor(bmpc_handle *h, int B, int ticks, const double *path, int path_entries, double *sstate, double *robot, double *p, double *x0,
                               double *dual_state, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                               double goal_tol, double *hist, double *traj_hist, int *ticks_run, double *replan /* [B][legs][len] or NULL */,
                               int *replan_info /* [B][legs] or NULL */, int update_flags, const double *disturb /* [ticks][B][21] or NULL */,
                               double *tube_hist /* [ticks][B][16] or NULL */, double *audit /* [B][12] or NULL */, double audit_tol,
                               double *log_hist /* [ticks][B][88 log_stages + 4] or NULL */, int log_stages, double *track /* [B][12] or NULL */,
                               int legs, const int *leg_tick /* [B][legs] */, const int *leg_on /* [B][legs] */, const double *leg_tol /* [B][legs] or NULL */,
                               int *legs_done /* [B] */, int *leg_fired /* [B][legs] or NULL */, int *leg_why /* [B][legs] or NULL */,
                               const double *tune /* [B][BMPC_TUNE_LEN] or NULL */, int *tune_info /* [B] or NULL */,
                               double *tune_used /* [B][BMPC_TUNE_LEN] or NULL */, const double *plant /* [B][BMPC_PLANT_LEN] or NULL */,
                               double *plant_state /* [B][BMPC_PLANT_STATE_LEN] */, int *plant_info /* [B] or NULL */,
                               double *plant_rec /* [B][BMPC_PLANT_REC_LEN] or NULL */, const double *sensor /* [B][BMPC_SENSOR_LEN] or NULL */,
                               double *sensor_state /* [B][BMPC_SENSOR_STATE_LEN] */, int *sensor_info /* [B] or NULL */,
                               double *sensor_rec /* [B][BMPC_SENSOR_REC_LEN] or NULL */, const double *sensor_noise /* [ticks][B][21] or NULL */,
                               double *meas_hist /* [ticks][B][robot record] or NULL */, void *hip_stream);
int bmpc_stream_sense(bmpc_handle *h, int B, double *robot, const double *sstate, const double *sensor /* [B][BMPC_SENSOR_LEN] */,
                      double *sensor_state /* [B][BMPC_SENSOR_STATE_LEN] */, int *sensor_info /* [B] or NULL */,
                      double *sensor_rec /* [B][BMPC_SENSOR_REC_LEN] or NULL, accumulated, not initialised */, const double *sensor_noise /* [B][21] or NULL */,
                      double *meas /* [B][robot record] or NULL */, int tick, void *hip_stream);
int bmpc_stream_unsense(bmpc_handle *h, int B, double *robot, const double *sstate, const double *sensor /* [B][BMPC_SENSOR_LEN] */,
                        const double *sensor_state /* [B][BMPC_SENSOR_STATE_LEN] */, void *hip_stream);
/* Rollout with a STATE OBSERVER: bmpc_stream_rollout_sensor (its arguments in their order up to and including meas_hist, their meaning, tests and contract)
 * with a TABLE of state estimators per stream.  The sensor hands its sample straight to the pack: offsets, quantisation and noise on q, dq and ddq, and under
 * BMPC_SENSOR_HOLD a sample that is one tick old.  Here an observer stands between the sample and what the pack, the solve and the post of a tick read: a
 * predictor-corrector on the model's own jerk-integrator chain.
 *   observer       [B][BMPC_OBSERVER_LEN] or NULL, DEVICE: row b, slots BMPC_OBSERVER_*; the three words behind BMPC_OBSERVER_GATE are pad and never looked at
 *                    LQ, LDQ, LDDQ    correction gain on q, dq, ddq                                          identity 1       valid when 0 < v <= 1
 *                    LEAD             1: the sample is one tick old (the sensor's HOLD): the corrected       identity 0       valid when 0 or 1
 *                                     estimate is advanced one chain step before it is handed out
 *                    GATE             innovation gate, rad: a sample with any |m_q,j - prior_q,j| not        identity +inf    valid when > 0 (+inf: none)
 *                                     <= GATE is rejected and the posterior is the prior (NaN is rejected)
 *                  a NaN slot takes its identity value
 *   observer_state [B][BMPC_OBSERVER_STATE_LEN], required with observer, IN AND OUT so that rollouts chain; all zeros = fresh: POST[21] the last posterior
 *                  (q, dq, ddq), JP[7] the record's jerk at the posterior's time, JL[7] the record's jerk read at the last call, HAS 1 once there is a
 *                  posterior, LAGS 1 where POST is one tick behind the last call, three pad words
 *   observer_info  [B] or NULL: 0 = row b was valid and the stream ran; else the bit mask of its invalid slots (bit k = slot k)
 *   observer_rec   [B][BMPC_OBSERVER_REC_LEN] or NULL, initialised by the call: SAMPLES the estimates made, N_REJ the samples the gate rejected, MAX_DQ the
 *                  largest |q_est - q| with TICK_DQ and JOINT_DQ its first tick and joint, MAX_DP the largest ||p_est - p|| (metres, position part of p_lie)
 *                  with TICK_DP its first tick, SUMSQ_DQ the sum of (q_est - q)^2 in tick order, joints 0..6 inside a tick; the conventions of sensor_rec
 *   sample_hist    [ticks][B][21] or NULL: the raw sample m (q | dq | ddq) the sensor handed the observer at tick t; NaN rows for the ticks not run
 * The estimate of tick t, right behind the sample and ahead of the pack, with m the sample (behind the sensor's HOLD), J the jerk the robot record carries at
 * this tick (the sensor keeps it; behind a plant step it is the jerk the drive delivered) and step(x, up, u) the model's chain step per joint from the jerk
 * up to the jerk u with the handle's h:
 *   fresh (HAS == 0)   post = out = m;  POST = m, JP = JL = J, HAS = 1, LAGS = 0; no gate is applied
 *   LEAD == 0          prior = step(POST, JP, J);  post = prior + L (m - prior) per word with the gain of its derivative, the word m itself where L == 1;
 *                      a rejected sample: post = prior;  out = post;  POST = post, JP = JL = J, LAGS = 0
 *   LEAD == 1          prior = LAGS ? step(POST, JP, JL) : POST (the sample's own time);  post as above;  out = step(post, LAGS ? JL : JP, J);
 *                      POST = post, where LAGS was 1 JP = the old JL, then JL = J, LAGS = 1
 * out replaces the sample where bmpc_stream_rollout_sensor installs the sample: SAME of the sensor state is decided on out against the truth over all 21
 * words; where it is 0 the record's q, dq, ddq become out and p_lie and v are recomputed from them, where it is 1 the record keeps every bit.  The way back
 * to the truth, the plant step, the rows and the events are that entry's.  meas_hist keeps its meaning, the record the pack of tick t read: it is now the
 * ESTIMATE's record.  sensor_rec keeps its meaning, the sample against the truth; observer_rec is the estimate against the truth.
 * KNOWN BLIND SPOT.  The observer is not told of a disturbance, a spliced re-plan or a post that exhausted the plan (the plant did not step): its prediction
 * is then off by what happened and the innovation pulls it back over the next samples, as a real filter's would.  The state is not reset.
 * An invalid row gets the treatment of an invalid sensor row: no tick, NaN history rows, its mask in observer_info[b], sensor_state and observer_state
 * untouched.  With observer == NULL the call IS bmpc_stream_rollout_sensor, and no observer argument is looked at.  With a table of NaN or of identity
 * values every array that entry names holds what it leaves, bit for bit.  With goal_tol = 0 every array, the states and the records hold what this loop
 * leaves, bit for bit:
 *   for t in 0..ticks-1: bmpc_stream_observe(tick t, noise rows of tick t); bmpc_stream_tick on one wave per stream; bmpc_stream_unsense;
 *                        bmpc_stream_plant(tick t); bmpc_stream_log; bmpc_stream_disturb(rows of tick t); bmpc_stream_update of the head records due
 * bmpc_stream_observe is the sample and the estimate on their own, one launch over the batch, for per-tick loops in the place of bmpc_stream_sense (its
 * arguments with their meaning, then the observer's): for an invalid sensor or observer row it writes the masks and touches nothing; a stream whose sstate
 * error count is >= N takes no sample and makes no estimate, SAME = 1 is written; observer_rec (or NULL) is ACCUMULATED, not initialised; sample (or NULL)
 * [B][21] is the raw sample.  It uses no workspace of the handle and may sit inside a capture of the caller's stream.
 * BMPC_ERR_ARG, nothing launched: what bmpc_stream_rollout_sensor refuses, observer without sensor, and observer without observer_state; the step: what
 * bmpc_stream_sense refuses, and no observer or observer_state. */
enum { BMPC_OBSERVER_LQ = 0, BMPC_OBSERVER_LDQ = 1, BMPC_OBSERVER_LDDQ = 2, BMPC_OBSERVER_LEAD = 3, BMPC_OBSERVER_GATE = 4, BMPC_OBSERVER_LEN = 8 };      /* three pad words */
enum { BMPC_OBSERVER_STATE_POST = 0, BMPC_OBSERVER_STATE_JP = 21, BMPC_OBSERVER_STATE_JL = 28, BMPC_OBSERVER_STATE_HAS = 35, BMPC_OBSERVER_STATE_LAGS = 36,
       BMPC_OBSERVER_STATE_LEN = 40 };                                                                                                                     /* three pad words */
enum { BMPC_OBSERVER_REC_SAMPLES = 0, BMPC_OBSERVER_REC_N_REJ, BMPC_OBSERVER_REC_MAX_DQ, BMPC_OBSERVER_REC_TICK_DQ, BMPC_OBSERVER_REC_JOINT_DQ, BMPC_OBSERVER_REC_MAX_DP,
       BMPC_OBSERVER_REC_TICK_DP, BMPC_OBSERVER_REC_SUMSQ_DQ, BMPC_OBSERVER_REC_LEN = 8 };
int bmpc_stream_observer_len(void);
int bmpc_stream_observer_state_len(void);
int bmpc_stream_observer_rec_len(void);
int bmpc_stream_rollout_observer(bmpc_handle *h, int B, int ticks, const double *path, int path_entries, double *sstate, double *robot, double *p, double *x0,
                                 double *dual_state, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                                 double goal_tol, double *hist, double *traj_hist, int *ticks_run, double *replan /* [B][legs][len] or NULL */,
                                 int *replan_info /* [B][legs] or NULL */, int update_flags, const double *disturb /* [ticks][B][21] or NULL */,
                                 double *tube_hist /* [ticks][B][16] or NULL */, double *audit /* [B][12] or NULL */, double audit_tol,
                                 double *log_hist /* [ticks][B][88 log_stages + 4] or NULL */, int log_stages, double *track /* [B][12] or NULL */,
                                 int legs, const int *leg_tick /* [B][legs] */, const int *leg_on /* [B][legs] */, const double *leg_tol /* [B][legs] or NULL */,
                                 int *legs_done /* [B] */, int *leg_fired /* [B][legs] or NULL */, int *leg_why /* [B][legs] or NULL */,
                                 const double *tune /* [B][BMPC_TUNE_LEN] or NULL */, int *tune_info /* [B] or NULL */,
                                 double *tune_used /* [B][BMPC_TUNE_LEN] or NULL */, const double *plant /* [B][BMPC_PLANT_LEN] or NULL */,
                                 double *plant_state /* [B][BMPC_PLANT_STATE_LEN] */, int *plant_info /* [B] or NULL */,
                                 double *plant_rec /* [B][BMPC_PLANT_REC_LEN] or NULL */, const double *sensor /* [B][BMPC_SENSOR_LEN] or NULL */,
                                 double *sensor_state /* [B][BMPC_SENSOR_STATE_LEN] */, int *sensor_info /* [B] or NULL */,
                                 double *sensor_rec /* [B][BMPC_SENSOR_REC_LEN] or NULL */, const double *sensor_noise /* [ticks][B][21] or NULL */,
                                 double *meas_hist /* [ticks][B][robot record] or NULL */, const double *observer /* [B][BMPC_OBSERVER_LEN] or NULL */,
                                 double *observer_state /* [B][BMPC_OBSERVER_STATE_LEN] */, int *observer_info /* [B] or NULL */,
                                 double *observer_rec /* [B][BMPC_OBSERVER_REC_LEN] or NULL */, double *sample_hist /* [ticks][B][21] or NULL */, void *hip_stream);
int bmpc_stream_observe(bmpc_handle *h, int B, double *robot, const double *sstate, const double *sensor /* [B][BMPC_SENSOR_LEN] */,
                        double *sensor_state /* [B][BMPC_SENSOR_STATE_LEN] */, int *sensor_info /* [B] or NULL */,
                        double *sensor_rec /* [B][BMPC_SENSOR_REC_LEN] or NULL, accumulated, not initialised */, const double *sensor_noise /* [B][21] or NULL */,
                        double *meas /* [B][robot record] or NULL */, int tick, const double *observer /* [B][BMPC_OBSERVER_LEN] */,
                        double *observer_state /* [B][BMPC_OBSERVER_STATE_LEN] */, int *observer_info /* [B] or NULL */,
                        double *observer_rec /* [B][BMPC_OBSERVER_REC_LEN] or NULL, accumulated, not initialised */, double *sample /* [B][21] or NULL */,
                        void *hip_stream);

/* HOST pointers; one staged copy each way on a stream of the handle, then a stream synchronisation (the single-problem solver(...) call) */
int bmpc_solve_batch_host(bmpc_handle *h, int B, const double *p, const double *x0, double *x, double *g, double *lam_g, double *lam_x,
                          double *f, int *iters, int *status, double *kkt);
/* HOST pointers: the same with multipliers (lam_g0 [B][43 N], lam_x0 [B][44 N]; either may be NULL = zeros): staged copies, the conversion of
 * bmpc_state_from_multipliers (mu0 = 0), the warm solve on that state, one synchronisation -- the single solver(...) call with lam_g0 / lam_x0. */
int bmpc_solve_batch_host_dual(bmpc_handle *h, int B, const double *p, const double *x0, const double *lam_g0, const double *lam_x0,
                               double *x, double *g, double *lam_g, double *lam_x, double *f, int *iters, int *status, double *kkt);

/* Timing of the solver kernel with HIP events on the launch stream: the {start, stop} pairs of the last `keep` launches are kept (0 = off).
 * bmpc_kernel_ms(h, back, &ms): duration of the launch `back` launches ago (0 = the last; synchronises on its stop event). */
int bmpc_set_timing(bmpc_handle *h, int keep);
int bmpc_kernel_ms(bmpc_handle *h, int back, float *ms);
int bmpc_last_kernel_ms(bmpc_handle *h, float *ms);
/* Per-solve latency: while a DEVICE buffer [>= B] is registered, every solve stores its own in-kernel duration in microseconds; NULL = off. */
int bmpc_set_latency_buffer(bmpc_handle *h, double *latency_us);

/* Teams and pairs: for short horizons (S <= 4) the library also holds kernels that put several COOPERATING WAVES on one problem (the item-parallel
 * passes of an iteration run over all their lanes, the recursions on one wave, recursion-independent work beside them on another).  Teams: 4
 * waves, N <= 10; a team owns a CU (most of its workspace lives in the CU's LDS): 256 resident on an MI355X.  Pairs: 2 waves on the one-wave
 * budget (40 KB of LDS, workspace in the global slab), N <= 11: 512 resident.  They serve the batches that leave SIMDs idle anyway: closed-loop
 * streams (BASELINE configs[4]: 256), the single solver(...) call of the drop-in (BoundMPC.py:446-453), batches up to 512.
 * bmpc_set_team_waves(h, 0) (default): teams when the batch fits into the resident teams, else pairs when it fits into the resident pairs,
 * else one wave per problem; (h, 1): always one wave; (h, 2): pairs whatever the batch; (h, 4): teams whatever the batch (an error where the
 * instantiation does not exist).  Results agree with the one-wave kernels up to the order of a few sums (same iterates unless a filter
 * decision sits on a rounding error).  bmpc_team_info: waves per problem a batch of B would get, resident teams / pairs of that kind, LDS
 * bytes of its workgroup.  The fused closed-loop ticks run on teams or on one wave per stream; a rollout (bmpc_stream_rollout) has a setting
 * of its own, bmpc_set_rollout_waves, whatever is set here. */
int bmpc_set_team_waves(bmpc_handle *h, int waves);
int bmpc_team_info(const bmpc_handle *h, int B, int *waves, int *resident_teams, int *lds_bytes);

/* Work-queue order of a batch that takes several rounds of the resident waves (stateless solves, one wave per problem, B > bmpc_launch_info's grid):
 * mode 1 = longest-expected-first -- an evaluation pass ranks the problems by decreasing objective at x0 and the queue hands them out in that
 * order (a launch lasts until its last wave is done); mode 0 = natural order.  Default 1 for N > 11, 0 for shorter horizons.  Batches beyond 65 536
 * problems keep their natural order.  Results do not depend on the order. */
int bmpc_set_queue_order(bmpc_handle *h, int mode);
int bmpc_get_queue_order(const bmpc_handle *h);      /* 0 / 1; -1: no handle */

/* Second attempt: a stateless solve (no dual state buffer) that ends with status 2 is run once more from x0 on the barrier start of the short horizons
 * (mu_init 0.1, slacks pushed to 1e-2) for at most `cap` iterations; `iters` is the sum of both attempts, a second attempt that runs into its cap keeps
 * status 2.  cap = 0: off.  Default 100 for N > 11, 0 for shorter horizons.  (What Ipopt users do by hand with another mu_init; the reference has no
 * counterpart: BoundMPC.py:465-489 reports the failure.)  The rule holds on every launch shape -- one wave per problem, pairs and teams
 * (bmpc_set_team_waves) -- and with every restoration mode: status and iters do not depend on the batch size.  With cap > 0 the output x of a
 * stateless device solve must not overlap its x0 (bmpc_solve_batch). */
int bmpc_set_second_attempt(bmpc_handle *h, int cap);
int bmpc_get_second_attempt(const bmpc_handle *h);      /* cap; -1: no handle */

/* launch geometry actually used: resident workgroups (one wave each), LDS bytes per workgroup, scratch bytes per workgroup */
int bmpc_launch_info(const bmpc_handle *h, int *grid, int *lds_bytes, long long *scratch_bytes);

#ifdef __cplusplus
}
#endif
#endif
