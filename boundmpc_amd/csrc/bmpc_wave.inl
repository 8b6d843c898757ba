// bmpc_wave.inl -- the BoundMPC OCP solver as a "wave program": ONE problem per 64-lane
// wavefront (CDNA4 wave64), lanes cooperating through LDS, N-scaling arrays in a per-wave
// global scratch slab (L2 / Infinity-Cache resident).
//
// The same text is compiled
//   * by hipcc for gfx950 inside bmpc_hip.hip (the product), where a "phase"
//     (LANES_BEGIN ... LANES_END) is the body executed by the 64 lanes followed by a
//     wavefront-scope fence (the workgroup IS one wave: its LDS and memory instructions execute
//     in program order, so no s_barrier / waitcnt drain is needed between phases), and
//   * by g++ inside tests/emu/bmpc_emu.cpp (TEST-ONLY lane emulator, never shipped or loaded
//     by the product), where a phase is a loop over the 64 lanes in a configurable order --
//     running forward and reverse lane orders exposes any intra-phase cross-lane dependence.
//
// What is solved (reference: /root/reference/bound_mpc/bound_mpc/BoundMPC/
// casadi_ocp_formulation.py:9-391 with bound_mpc_functions.py:13-310, mpc_utils_casadi.py:6-165,
// jerk_trajectory_casadi.py:78-175, RobotModel/RobotModel.py:62-100,1055-1107,1270-1303):
// the N-stage, 44-variable/43-constraint-per-stage NLP the reference hands to
// CasADi->Ipopt->MUMPS at BoundMPC.py:446-453.  Algorithm: primal-dual interior point with
// the exact Lagrangian Hessian; the block-tridiagonal Newton system is factorised stage by
// stage (Riccati recursion on a 35-dim reduced node state, lifted pos/v variables and the
// trapezoidal omega coupling eliminated node-locally), filter line search (Waechter-Biegler).
//
// Lane maps: evaluation = one lane per kinematic evaluation point (2N points); adjoint /
// forward sweeps = one lane per state component; Riccati = one lane per PAIR of integrator chains
// (8 x 8 pairs = 64 lanes): the stage map is I_8 (x) CF, so every 4x4 block of the value-function
// Hessian transforms independently; inequality rows = one lane per row (57 per node).
//
// TEAMS (BMPC_NW > 1; round 4): the same program run by a workgroup of NW cooperating waves on ONE problem, for batches that leave
// SIMDs idle (B <= resident workgroups / NW: closed-loop streams, the single solver(...) call of the drop-in).  The waves share the
// LDS working set and the workspace slab and execute the same wave-uniform control flow (every scalar of the driver is computed
// redundantly by every wave from the same LDS words); what changes is who executes a phase:
//   * WIDE_BEGIN ... WIDE_END: item-parallel passes (row passes, node gradients, stage data, trial points, outputs) run over
//     64 NW lanes -- `wl` = wave * 64 + lane is the item lane, WS = 64 NW the stride -- and end with a workgroup barrier;
//   * SOLO_BEGIN(w) ... SOLO_END: a region only wave w executes (the sequential sweeps: adjoint, Riccati, forward; their phases keep the
//     wavefront-scope fences of the one-wave program), the other waves go on to the next TEAM_SYNC();
//   * reductions over a wide pass (red_*_w) read the NW x 64 per-lane partials in a fixed order in every wave.
// With BMPC_NW == 1 every one of these reduces to the one-wave text: wl = lane, WS = 64, TEAM_SYNC() = nothing, SOLO = unconditional.
//
// PAIRS (BMPC_NW == 2 with BMPC_WSG; round 6, csrc/bmpc_pair.hip): a team of TWO waves that keeps the one-wave program's budget per problem -- 40 KB
// of LDS and the workspace in the global slab (WSG) -- so that two pairs share a CU (512 problems resident; compiled for 256 registers per wave it
// would be four, but the text needs ~440: bmpc_pair.hip has the numbers).  Wave 0 runs the recursions; wave 1 owns what does not depend on them: the
// references / objective half of an evaluation beside the kinematics, and -- inside the Riccati sweep -- the staging of the node-cost inputs of the
// NEXT stage from the slab into LDS (its own register prefetch, a stage ahead), the recursion-independent half of the node-cost add, the q~ rows
// and t6.  What the helper hands over per stage (14 words per lane) goes through the part of the value-function block area that is idle between
// two Schur updates (L_PREP: single-buffered, hence a second LDS-only barrier per stage, placed where the helper is already waiting).
#pragma once

#ifndef BMPC_NW
#define BMPC_NW 1
#endif
#ifndef BMPC_NAMESPACE
#define BMPC_NAMESPACE bmpc
#endif
#ifndef TEAM_SYNC
#if BMPC_NW > 1
#error "a team build (BMPC_NW > 1) must define TEAM_SYNC(), WIDE_BEGIN / WIDE_END and SOLO_BEGIN / SOLO_END"
#endif
#define TEAM_SYNC()
#define TEAM_SYNC_LDS()
#define WIDE_BEGIN LANES_BEGIN const int wl = lane; (void)wl;
#define WIDE_END LANES_END
#define SOLO_BEGIN(w) {
#define SOLO_END }
#define TEAM_IS(w) true
#endif
#ifndef BMPC_LANE_ID
#define BMPC_LANE_ID threadIdx.x
#endif
#ifndef LIDXW
#define LIDXW LIDX      // index of a lane's register set inside a wide phase (the emulator of a team: the item lane)
#endif

#ifndef LIDXH
#ifdef BMPC_EMU
#define LIDXH (64 + lane)   // register set of a lane of the HELPER wave (wave 1 of a pair): the emulator keeps one set per lane of the team
#else
#define LIDXH LIDX
#endif
#endif
#ifndef BMPC_PROF
#define BMPC_PROF(W, id)
#endif
// four independent partial sums: breaks the dependent fp64 FMA chain of a long dot product (use inside fully unrolled loops)
#define BMPC_ACC4(acc, idx, val) { if (((idx) & 3) == 0) acc##0 += (val); else if (((idx) & 3) == 1) acc##1 += (val); else if (((idx) & 3) == 2) acc##2 += (val); else acc##3 += (val); }
#define BMPC_ACC4_DECL(acc) double acc##0 = 0, acc##1 = 0, acc##2 = 0, acc##3 = 0
#define BMPC_ACC4_SUM(acc) ((acc##0 + acc##1) + (acc##2 + acc##3))
#ifndef BMPC_SCHED_FENCE
#define BMPC_SCHED_FENCE()   // GPU build: stops the scheduler from hoisting LDS loads across this point (bounds live ranges)
#endif

namespace BMPC_NAMESPACE {

// ----------------------------------------------------------------------------------------
// dimensions and index maps
// ----------------------------------------------------------------------------------------
constexpr int NZ = 44, NG = 43, NE = 36, NS = 35, NU = 8, NI = 57, SMAX = 6, SMAX_ZLDS = 4, NPMAX = 141 + 91 * SMAX, NMAX = 40;
constexpr int NW = BMPC_NW, WS = 64 * NW;      // waves per problem (team size), lanes of a wide pass
constexpr int cdiv_(int a, int b) { return (a + b - 1) / b; }
#define GN_MU_GATE 0.0       // Gauss-Newton fallback of the inertia correction while mu >= GN_MU_GATE.  Until round 4 it was 0.05 (first barrier level only): on the tight
                             // 30-stage batch the problems of the tail spend 40-150 iterations at LOW barrier levels with an indefinite exact Hessian, regularised by
                             // delta ~ 0.1 in every iteration (steps cut to a few per cent by the tube rows); with the positive semidefinite Gauss-Newton matrix there
                             // as well: mean 35.3 -> 32.7 iterations, failed sweeps 6.2 -> 4.1 per problem, p99 108 -> 78, 99.71 -> 99.80 % converged (oracle, 2048 problems)
#define GN_PROBE 3           // while the fallback keeps being needed, every GN_PROBE-th iteration tries the exact Hessian again
#define DELTA_FIRST 1e-3     // inertia correction constants of oracle/bmpc_oracle.c
#define DELTA_UP_FIRST 10.0
#define DELTA_KEEP_MIN 1e-5
#define STALL_FACTOR 0.5     // stall test: primal infeasibility must halve per stall_window iterations
#define STALL_RESTARTS 3     // barrier restarts from a stalled iterate before status 2 (long horizons only; oracle/bmpc_oracle.c solve_one)
#define STALL_RESTARTS_RETRY 2   // ... when a second attempt stands behind the solve (Opts::retry_cap) and it has not been through a restoration phase: the third restart
                             // rescues less than the second attempt does and costs a stall window more (configs[3]: 163 -> 155 ms at 99.95 -> 99.93 %)
#define STALL_RESTART_MU 3.0
#define STALL_RESTART_PUSH 1e-1
// restoration phase (oracle/bmpc_oracle.c solve_one has the description and the numbers)
#define RESTO_RHO 1e3          // l1 penalty of the elastic variables (Ipopt's resto_penalty_parameter: 1000)
#define RESTO_MU 1.0           // its first barrier level
#define RESTO_MU_BACK 1.0      // barrier level of the main phase when it resumes from the feasible point
#define RESTO_PUSH_BACK 1e-6   // smallest slack there
#define RESTO_SHORT_ALPHA 0.1  // a step shorter than this is "short" (jam detection)
#define RESTO_REL 1e-3         // the restoration phase counts as converged at a KKT error of RESTO_REL * rho * (largest violation)
#define RESTO_MARGIN 1e-6      // strictly feasible: max h <= -RESTO_MARGIN ...
#define RESTO_GTOL 1e-4        // ... and equality residuals below this
#define RESTO_MAX 3            // restoration phases per solve
#define RESTO_ROLLOUT_TOL 1e-2 // the phase starts from the rollout of the iterate's own jerks when an equality residual exceeds this
#define START_ROLLOUT_TOL 0.5 // a stateless solve starts from the rollout of x0's own jerks when an integrator-chain residual of x0 exceeds this (oracle/bmpc_oracle.c solve_one)
#define KAPPA_EPS 100.0   // barrier problem "solved" at KKT error <= KAPPA_EPS * mu (oracle/bmpc_oracle.c).  A deliberate departure from Ipopt, whose
                          // barrier_tol_factor defaults to 10: measured on the bench batches it takes 2 of 14 iterations off the mean and 36 -> 20 off the slowest problem
                          // (DESIGN.md 2, round 2); the price is an occasional premature barrier reduction (a problem that then crawls for some iterations)
enum { ZJ = 0, ZJPHI = 7, ZQ = 8, ZDQ = 15, ZDDQ = 22, ZPOS = 29, ZIW = 32, ZV = 35, ZW = 38, ZPHI = 41, ZDPHI = 42, ZDDPHI = 43 };
enum { GQ = 0, GDQ = 7, GDDQ = 14, GPOS = 21, GIW = 24, GV = 27, GW = 30, GPHI = 33, GDPHI = 34, GDDPHI = 35 };
enum { SQ = 0, SDQ = 7, SDDQ = 14, SJ = 21, SPHI = 28, SDPHI = 29, SDDPHI = 30, SJPHI = 31, SIOTA = 32 };
enum { IJU = 0, IJL = 8, IQU = 16, IQL = 23, IDQU = 30, IDQL = 37, IPHI0 = 44, IPHIMAX = 45, IDPHIMAX = 46, ITUBE = 47 };
// kinematics record (stride KREC): aT[3][7], wT[3][7], D[6][7], pos[3], v[6], dq[7]
enum { KA = 0, KW = 21, KD = 42, KPOS = 84, KV = 87, KDQ = 93, KREC = 104 };
// node-reference record (stride RREC)
enum { RSEG = 0, RX = 1, RDP = 2, RDH = 8, REP = 11, RER = 14, RERPAR = 17, RL2 = 20, RRR = 23, RV2RR = 26, RSIG = 27, RSIG1 = 28,
       RSIG2 = 29, RC = 30, RWD = 35, RW1 = 40, RW2 = 45, RC2 = 50, RGC = 55 /* [5][4]: 3 vector comps + phi */,
       // multiplier-independent part of the (pos, iw, phi) cost Hessian, evaluated once per iterate with the record (wide over the
       // nodes) instead of once per Riccati stage: Hpp 3x3, Hrr 3x3, Hp,phi 3, Hr,phi 3, H phi,phi, |dp_d|^2
       RHPPG = 80, RHRRG = 89, RHPFG = 98, RHRFG = 101, RHFFG = 104, RDPDP = 105, RREC = 108 };
// parameter offsets (casadi_ocp_formulation.py:361-376) as functions of S
struct POff {
    int q0, dq0, ddq0, phi0, p0, v0, iwref0, dtau, ipar, io1, io2, xphid, jerk, jerkphi, sw, jacr, jacl, pref, dpref, dpn, bp1, bp2,
        br1, br2, a[5], w, phimax, dphimax, v1, v2, v3, qd, size;
};
BMPC_HD inline POff make_poff(int S) {
    POff o; int c = 0;
    o.q0 = c; c += 7; o.dq0 = c; c += 7; o.ddq0 = c; c += 7; o.phi0 = c; c += 3; o.p0 = c; c += 6; o.v0 = c; c += 6;
    o.iwref0 = c; c += 3; o.dtau = c; c += 3; o.ipar = c; c += 3 * S; o.io1 = c; c += 3 * S; o.io2 = c; c += 3 * S;
    o.xphid = c; c += 3; o.jerk = c; c += 7; o.jerkphi = c; c += 1; o.sw = c; c += S + 1; o.jacr = c; c += 9; o.jacl = c; c += 9;
    o.pref = c; c += 6 * S; o.dpref = c; c += 6 * S; o.dpn = c; c += 3 * S; o.bp1 = c; c += 3 * S; o.bp2 = c; c += 3 * S;
    o.br1 = c; c += 3 * S; o.br2 = c; c += 3 * S;
    for (int i = 0; i < 5; i++) { o.a[i] = c; c += 9 * (S + 1); }
    o.w = c; c += 15; o.phimax = c; c += 1; o.dphimax = c; c += 1; o.v1 = c; c += 3 * S; o.v2 = c; c += 3 * S; o.v3 = c; c += 3 * S;
    o.qd = c; c += 7; o.size = c;
    return o;
}
// LDS-relative offsets (index into L, from L_PAR = 0) of the parameter arrays; see the note at the LDS layout
BMPC_HD inline int poff_split(int S) { return S <= SMAX_ZLDS ? (1 << 30) : make_poff(S).a[3]; }
BMPC_HD inline int lds_index_of_p(int S, int id, int lzl) { const int sp = poff_split(S); return id < sp ? id : id - sp + lzl; }
BMPC_HD inline POff make_poff_lds(int S, int lzl) {
    POff o = make_poff(S);
    if (S > SMAX_ZLDS) {
        const int sh = lzl - o.a[3];
        o.a[3] += sh; o.a[4] += sh; o.w += sh; o.phimax += sh; o.dphimax += sh; o.v1 += sh; o.v2 += sh; o.v3 += sh; o.qd += sh;
    }
    return o;
}

// LDS layout (doubles)
// The parameter vector occupies [L_PAR, L_PAR + 512): 141 + 91 S <= 505 doubles up to S = 4.  Handles with 5 or 6 path segments run the
// instantiation that keeps the iterate in the workspace (wave_solve<false>), whose iterate area L_ZL (484 doubles) is free: the tail of p
// from a[3] on (27 S + 42 <= 204 doubles) lives there, and the offsets of make_poff_lds point at it.  lds_index maps an index of p.
enum { L_PAR = 0, L_PM = 512, L_SR = L_PM + 35 * 36, L_RED = L_SR + 8 * 44, L_PV = L_RED + 6 * 64, L_PR = L_PV + 36, L_QT = L_PR + 36,
       L_RD = L_QT + 36, L_DS = L_RD + 36, L_DSN = L_DS + 36, L_DU = L_DSN + 36, L_MV = L_DU + 8, L_AE = L_MV + 44, L_K0 = L_AE + 42,
       L_K1 = L_K0 + KREC, L_KV = L_K1 + KREC, L_XT = L_KV + KREC, L_NC = L_XT + 15 * 14, L_WY = L_NC + 160, L_WV = L_WY + 196, L_TOT = L_WV + 196,
       L_MU = L_TOT + 44, L_FLAG = L_MU + 16, L_FILT = L_FLAG + 8, L_PROF = L_FILT + 64, L_KV1 = L_PROF + 32, L_ST = L_KV1 + KREC, L_ZL = L_ST + 460, L_SIZE1 = L_ZL + 484 };
enum { L_KKP = L_WY };
// per-lane partials of the wide passes: 6 slots x WS (L_REDW) and 5 x WS (L_KKPW; the fifth, max h, is written in the restoration phase only).  One wave: the one-wave areas themselves.  Teams: own
// areas behind the one-wave layout (a team owns a whole CU: 1 workgroup of NW waves at 512 registers each), plus the hand-over words of
// the solo regions (forward sweep's gradient products, the Riccati sweep's verdict, the work-queue index)
enum { L_PP = L_PM };   // [4 fields][64 pairs] partial products of P rdyn (blk_add_lane -> S0), in the area the value-function blocks used to occupy
enum { L_DUMMY = L_FLAG + 1 };   // write-only slot: target of the stores of lanes that have nothing to store (keeps phases branch-free)
// row descriptors of the 57 internal inequality rows (box rows: +-Z[src] - lim), built once per problem: [sgn 57 | lim 57 | src 57]
// integrator-chain coefficients CF[fr][fc] (4 x 5) as a table: chain_cf() with a lane-dependent argument compiles into a nest of
// branches, a table look-up is one LDS read
enum { L_CFT = L_QT };
// Z index of every reduced-state row (35): q, dq, ddq, jerk (7 each), phi, dphi, ddphi, jerk_phi, iota -> iw
enum { L_ZMAP = L_TOT };
// the 15x14 area of the retired cross block XT now holds: t6 (6), the row table (3 x 57), the adjoint partials (2 x 8)
enum { L_T6 = L_XT, L_ROWT = L_XT + 8, L_RJP = L_XT + 8 + 3 * 57 + 1 /* 2 x 8: jerk residual partials of the adjoint sweep (ping-pong) */ };
static_assert(8 + 3 * 57 + 1 + 16 <= 15 * 14, "adjoint partials must fit into the retired XT area");
static_assert(8 + 3 * 57 <= 15 * 14, "row table must fit into the retired XT area");   // inequality part of the KKT error (4 x 64 slots), parked in the node-cost work area between sweeps (WY 196 + WV 196)   // L_ZL: iterate Z (N <= 11)
// Block (chain-pair) Riccati storage, overlaid on the L_PM..L_RED region (column scheme retired):
//   PB  [16 planes (f*4+g)][64 pairs (i*8+l)]  value-function Hessian blocks P[(f,i)][(g,l)]
//   PCI [3][4][8]  P[(f,i)][iota_a] ;  PII [3][3] ;  GS [8][36] jerk rows of M (col 35 = m_j) ; R8 [8][8] ; KS [8][36] gains (col 35 = kff)
//   MCI [3][5][8]  C^T P_c,iota, then M_c,iota in place ;  PE [3][14] = P_ii E ;  KHP [2][72] prefix vectors of the kinematic curvature
enum { L_PB = L_PM, L_PCI = L_PB + 1024, L_PII = L_PCI + 96, L_GS = L_PII + 12, L_R8 = L_GS + 288, L_KS = L_R8 + 64, L_MCI = L_KS + 288,
       L_PE = L_MCI + 120, L_BLK_END = L_PE + 42, L_KHP = L_WV /* 152 of the 196 */ };
static_assert(10 * 57 <= (int)L_PV - (int)L_PB, "multiplier staging of the adjoint (ten nodes per pass) must fit into the block area");
static_assert((int)L_BLK_END <= (int)L_PV, "block Riccati storage must fit into the retired PM/SR/RED region");
// staging area inside L_ST: per-stage inputs of the sequential sweeps, loaded from the scratch slab in ONE burst per stage
enum { ST_REF = 0, ST_Z = 108, ST_SG = 152, ST_NU = 212, ST_G = 272, ST_LAM0 = 308, ST_LAM1 = 344, ST_GH = 380, ST_RLVM = 424, ST_RLV0 = 436, ST_RLVP = 448,
       /* forward sweep view */ ST_KT = 0, ST_KF = 280, ST_RDY = 288, ST_AES = 324, ST_RLVF = 366, ST_GHF = 378 /* 64: gradient entry of the lane's dZ component */ };
// node-cost work area inside L_NC
enum { NC_HPP = 0, NC_HRR = 9, NC_HPF = 18, NC_HRF = 21, NC_SC = 24 /* hff,hdd,hddd,cv */, NC_A1 = 28 /* Hpp*Jp 3x7 */, NC_A2 = 49 /* Hrr*Ehat 3x14 */,
       NC_GL = 91 /* 44 */, NC_RL = 135 /* 9 */, NC_GY = 144 /* 14 */ };

// row of the NCS workspace array (one per stage): [0, 91) mirrors the LDS node-cost area L_NC (small blocks 28 | A1 21 | A2 42),
// then the curvature multipliers (12 -> L_MU + 4), dp_d of the stage's node (6 -> ST_REF + RDP), the 12 non-trivial entries of
// gl - g^ (rows pos 3, v 6, phi, dphi, ddphi of Z) and a zero word (what the other rows of gl add to g^)
// Per-joint vectors of the kinematic curvature of a stage (round 4): with them an entry of sum lambda . d2F/dq_i dq_l is three dot products
// (kh_qq) instead of five double cross products.  Row layout [vector 0..6][coordinate 0..2][joint 0..6] like the kinematics record:
//   X = mu_p x a + (mu_v x W) x a - (mu_v x a) x W,  n = mu_v x a,  o = mu_w x a   (roles of the FIRST index i)
//   Y = a x V + W x w,  g = a x Wgt                                                  (roles of the SECOND index l)
//   g' = a' x Wgt', o' = mu_w' x a'                                                  (velocity point of the next node: only its angular rows)
// (a, w: axes and J_v columns of the record; W = Wlt, V = Vge, Wgt: the prefix vectors kin_point leaves in KHPG)
enum { KHV_X = 0, KHV_N = 21, KHV_O = 42, KHV_Y = 63, KHV_G = 84, KHV_G1 = 105, KHV_O1 = 126, KHV_LEN = 147, KHV_STRIDE = 152 };
enum { NCS_MU = 91, NCS_RDP = 103, NCS_ADDV = 109, NCS_ZERO = 121, NCS_DUMMY = 122, NCS_STRIDE = 128 };

// Teams also keep most of the WORKSPACE in LDS (L_WSL; a team has the LDS of a whole CU, 160 KB, to itself): the row arrays of the
// inequality rows, residuals, multipliers, gradients, defects, the kinematics and reference records and the node-cost rows -- everything
// the wide passes exchange between phases.  With one wave per CU the 148 KB slabs of an XCD's problems do not fit its L2 (4 MB) and every
// dependent round trip to them costs ~1.7 k cycles (Infinity Cache); measured (profiles/r04_a_*): the wide passes of a team were bound by
// exactly those trips, not by issue.  Only the Riccati gains, the curvature prefix vectors (both consumed through the sweeps' register
// prefetch) and, for long horizons, the iterate stay in the global slab.
constexpr int WSL_PER_STAGE = 10 * NI + 3 * NE + NZ + 8 + NU + 36 + 42 + 12 + 2 * KREC + RREC + NCS_STRIDE;      // make_scr's LDS-resident arrays, doubles per stage
#if BMPC_NW > 1 && defined(BMPC_WSG)
constexpr int TEAM_NMAX = 11;      // pairs: the horizons whose iterate lives in LDS (wave_solve<true>); L_DSA (36 per stage) sits in the first 512 words of the block area
#else
constexpr int TEAM_NMAX = 10;      // longest horizon a team's LDS holds (the reference's experiments and BASELINE configs[1], [2], [4] run N = 10)
#endif
#if BMPC_NW > 1 && defined(BMPC_WSG)
// Pairs: the one-wave layout plus eight words.  The helper wave's staging of a stage (inputs of blk_prep_lane / node_q_row_p / stage_t6) uses the
// areas the sweep's wave of a team leaves idle during the Riccati sweep: L_NC[0..91) (small blocks, A1, A2), ST_SG, ST_G, L_KHP (= L_WV), L_WY and
// the two velocity-record buffers L_KV / L_KV1 (cut up below).  Hand-over to the sweep's wave: L_PREP (block area behind the partial products L_PP,
// idle between the D gather of one Schur phase and the MFMA of the next) and L_QRB (double-buffered by stage parity: the sweep's wave reads the
// q~ rows of stage k while the helper writes those of stage k - 1).  L_DSA (forward sweep -> wide dZ pass) sits where the trial iterate will be written.
#ifdef BMPC_EMU
enum { WRED_STRIDE = WS, L_REDW = L_SIZE1, L_KKPW = L_REDW + 6 * WRED_STRIDE, L_TFLAG = L_KKPW + 5 * WRED_STRIDE };      // the emulator's per-lane slots do not fit the one-wave areas
#else
enum { WRED_STRIDE = 64, L_REDW = L_RED, L_KKPW = L_KKP, L_TFLAG = L_SIZE1 };      // GPU: word `wave` of each 64-word slot of the one-wave areas
#endif
enum { PREP_N = 14, L_PREP = L_PB + 256 /* add: 10 planes x 64 | c3inc: 3 x 32 | piinc: 6 */, PREP_C3 = 640, PREP_PII = 736, PREP_LEN = 742,
       L_DSA = L_PB, L_WY2 = L_WY, L_HKHP = L_KHP,
       L_HKV = L_KV /* 24: axes (KA part) of the velocity record of the next node */, L_QRB = L_KV + 24 /* 2 x 40 */,
       L_HGL = L_KV1 /* 44: gl of the helper's stage */, L_HRD = L_KV1 + 44 /* 36: its defect vector */, L_HDP = L_KV1 + 80 /* 6: its dp_d */,
       L_SIZE = L_TFLAG + 8 };
static_assert(256 + PREP_LEN <= 1024 && 36 * TEAM_NMAX <= 512, "hand-over areas must fit the block area");
static_assert(24 + 80 <= KREC && 86 <= KREC, "the helper's small staging must fit the two idle record buffers");
#ifndef BMPC_EMU
static_assert(L_SIZE * 8 <= 40 * 1024, "a pair's working set must fit a quarter of the LDS of a CU (four pairs per CU)");
#endif
#elif BMPC_NW > 1
#ifdef BMPC_EMU
enum { WRED_STRIDE = WS };      // the emulator runs the lanes of a wide pass one after the other: per-lane slots, reduced in the GPU's order afterwards
#else
enum { WRED_STRIDE = NW };      // GPU: a wave reduces its 64 partials in registers (butterfly) and stores ONE word per wave and slot
#endif
// L_PREP: what the helper wave of the Riccati sweep hands to the sweep's wave per stage (blk_prep_lane's results: 10 block entries, 3 iota
// increments, 1 P_ii increment per lane, plane-major), double-buffered by stage parity; L_WY2: second curvature table (the helper writes
// stage k-1's while S0 of stage k reads its own); L_HKHP: the helper's staging of the curvature prefix vectors (the one array it needs
// that lives in the global slab)
enum { PREP_N = 14 };
// L_DSA: the forward sweep's reduced states of all stages (36 per stage), from which a wide pass forms the dZ rows behind the sweep
enum { L_REDW = L_SIZE1, L_KKPW = L_REDW + 6 * WRED_STRIDE, L_DSA = L_KKPW + 5 * WRED_STRIDE, L_TFLAG = L_DSA + 36 * TEAM_NMAX, L_PREP = L_TFLAG + 8,
       L_WY2 = L_PREP + 2 * PREP_N * 64, L_HKHP = L_WY2 + 196, L_QRB = L_KV1 /* 2 x 40: q~ rows + t6 per stage parity */, L_HGL = L_KV /* 44: the helper's gl */, L_WSL = L_HKHP + KHV_STRIDE, L_SIZE = L_WSL + WSL_PER_STAGE * TEAM_NMAX + 16 };
#ifndef BMPC_EMU
static_assert(L_SIZE * 8 <= 160 * 1024, "a team's working set must fit the 160 KB of LDS of a CU");
#endif
#else
enum { WRED_STRIDE = 64, L_REDW = L_RED, L_KKPW = L_KKP, L_SIZE = L_SIZE1 };
#endif

struct Opts {
    double tol; int max_iter; double mu_init; double mu_min_fac; double slack_push; int exact_hessian; int verbose; double mu_warm; int stall_window;
    double bound_margin;      // joint position / velocity limits tightened by this much inside the solver (real-time modes: a plan solved to a loose
                              // tolerance then still respects the true limits); 0 = the reference's limits
    int restoration;          // 1: a jammed, stalled or numerically broken main phase hands over to the restoration phase (round 5; oracle/bmpc_oracle.c solve_one;
                              // long horizons: behind the barrier restarts); 2: only a numerical breakdown does; 0: never (status 2 / 3)
    int resto_short;          // consecutive steps shorter than RESTO_SHORT_ALPHA that count as a jam (6; 0 = the stall test alone)
    int resto_cap;            // iterations one restoration phase may take before the solve ends as status 2 (40)
    int start_rollout;        // 1: a stateless solve (no dual state buffer) whose x0 is far off its own dynamics (START_ROLLOUT_TOL) starts from the rollout of x0's jerks; 0: from x0 as given
    int hold_mu;              // 1: the barrier level a solve starts on (clamp(stored level, mu_warm, mu_init)) is HELD: no barrier update (real-time iteration on a
                              // per-stream level that the caller / stream_pack sets in the dual state, bmpc_set_barrier_hold; round 6); 0: the monotone update
    int retry_cap;            // > 0: a stateless solve that ends with status 2 gets a SECOND ATTEMPT from x0 of at most this many iterations on the barrier start of
                              // the short horizons (wave_solve_retry below; bmpc_set_second_attempt; default 100 for N > 11, else 0)
};

// global scratch layout (doubles) for horizon N
struct Scr {
    int Z, ZT, T, TT, NUm, LAM, G, GT, HIN, HT, DZ, DT, DNU, GH, GVP, RJ, KIN, REF, KT, KF, RDY, AES, RLV, SG, TI, SR, NU2, NCS, KHPG, KHV, E, ET, DE, size, lsize;
};
BMPC_HD inline Scr make_scr(int N) {
#if BMPC_NW > 1 && !defined(BMPC_WSG)
    // teams: two index spaces -- `l` counts the LDS-resident arrays (offsets from L_WSL, accessor WL), `c` what stays in the global slab (accessor G)
    Scr s; int c = 0, l = 0;
    s.Z = c; c += N * NZ; s.ZT = c; c += N * NZ; s.DZ = c; c += N * NZ; s.KT = c; c += N * NS * NU; s.KF = c; c += N * NU; s.KHPG = c; c += 2 * N * 72; s.KHV = c; c += N * KHV_STRIDE;
    s.DNU = c; c += N * NI;      // (multiplier directions: written by row pass B, read once by the update pass -- what did not fit)
    s.E = c; c += N * NI; s.ET = c; c += N * NI; s.DE = c; c += N * NI;      // elastic variables of the restoration phase (rare: global slab, accessor G)
    s.T = l; l += N * NI; s.TT = l; l += N * NI; s.NUm = l; l += N * NI; s.LAM = l; l += N * NE; s.G = l; l += N * NE; s.GT = l; l += N * NE;
    s.HIN = l; l += N * NI; s.HT = l; l += N * NI; s.DT = l; l += N * NI; s.GH = l; l += N * NZ; s.GVP = l; l += N * 8;
    s.RJ = l; l += N * NU; s.KIN = l; l += 2 * N * KREC; s.REF = l; l += N * RREC; s.RDY = l; l += N * 36; s.AES = l; l += N * 42; s.RLV = l; l += N * 12;
    s.SG = l; l += N * NI; s.TI = l; l += N * NI; s.SR = l; l += N * NI; s.NU2 = l; l += N * NI; s.NCS = l; l += N * NCS_STRIDE;
    s.size = (c + 15) & ~15; s.lsize = l;
    return s;
#else
    Scr s; int c = 0;
    s.Z = c; c += N * NZ; s.ZT = c; c += N * NZ; s.T = c; c += N * NI; s.TT = c; c += N * NI; s.NUm = c; c += N * NI;
    s.LAM = c; c += N * NE; s.G = c; c += N * NE; s.GT = c; c += N * NE; s.HIN = c; c += N * NI; s.HT = c; c += N * NI;
    s.DZ = c; c += N * NZ; s.DT = c; c += N * NI; s.DNU = c; c += N * NI; s.GH = c; c += N * NZ; s.GVP = c; c += N * 8;
    s.RJ = c; c += N * NU; s.KIN = c; c += 2 * N * KREC; s.REF = c; c += N * RREC; s.KT = c; c += N * NS * NU; s.KF = c; c += N * NU;
    s.RDY = c; c += N * 36; s.AES = c; c += N * 42; s.RLV = c; c += N * 12; s.SG = c; c += N * NI; s.TI = c; c += N * NI; s.SR = c; c += N * NI; s.NU2 = c; c += N * NI;   // NU2: second multiplier buffer (the update ping-pongs)
    s.NCS = c; c += N * NCS_STRIDE;   // node-cost data of every stage (wave_stage_data_wide): see the NCS_* row layout
    s.KHPG = c; c += 2 * N * 72;      // prefix vectors of the kinematic curvature, one row per kinematics record (kin_point)
    s.KHV = c; c += N * KHV_STRIDE;   // per-joint vectors of the kinematic curvature, one row per stage (wave_stage_data_wide)
    s.E = c; c += N * NI; s.ET = c; c += N * NI; s.DE = c; c += N * NI;      // elastic variables of the restoration phase, trial values, directions (accessor G)
    s.size = (c + 15) & ~15; s.lsize = 0;
    return s;
#endif
}

struct Problem {           // per-problem global pointers
    const double *p, *x0;
    double *x, *g, *lam_g, *lam_x, *f, *kkt;
    int *iters, *status;
    double *state;         // optional dual state of a receding-horizon stream: [nu (N*57) | mu | iterations]; mu <= 0: cold start
    int resto_from;        // >= 0 (instantiations with RESTO only): x0 is the iterate at which the main phase of another kernel jammed after (low 20 bits)
                           // iterations and (bits 20..) barrier restarts -- the solve starts in the restoration phase and counts on from there; -1: an ordinary solve
};

// Workspace accessor: wave-uniform base (an SGPR pair on the GPU) plus an unsigned 32-bit BYTE offset.  Indexing a plain double * with
// an int makes every access a sign extension + a 64-bit shift-add + a 64-bit address register pair; this form is the hardware's
// "scalar base + 32-bit vector offset" addressing mode (the slab of one wave is far below 4 GB).
#if defined(__HIP_DEVICE_COMPILE__)
#define BMPC_ASSUME(c) __builtin_assume(c)
#else
#define BMPC_ASSUME(c)
#endif
struct GPtr {
    char *b; int o;      // o: byte offset, never negative
    // signed arithmetic (overflow undefined) plus the stated range lets the compiler split constant index parts off into the
    // instruction's immediate field; with unsigned wrap-around semantics every access got an address add of its own
    BMPC_D double &operator[](int i) const { const int off = o + i * (int)sizeof(double); BMPC_ASSUME(off >= 0); return *(double *)(b + (size_t)(unsigned)off); }
    BMPC_D GPtr operator+(int i) const { GPtr r; r.b = b; r.o = o + i * (int)sizeof(double); BMPC_ASSUME(r.o >= 0); return r; }
    BMPC_D double *ptr() const { return (double *)(b + o); }
};
BMPC_D inline GPtr make_gptr(double *base) { GPtr r; r.b = (char *)base; r.o = 0; return r; }
// accessor of the workspace arrays a team keeps in LDS (make_scr): the global slab itself in the one-wave program
#if BMPC_NW > 1 && !defined(BMPC_WSG)
typedef double *LPtr;
#define BMPC_WL(W) ((W).L + L_WSL)
#else
typedef GPtr LPtr;
#define BMPC_WL(W) ((W).G)
#endif
struct Wave {
    int N, S; double h; Opts o;
    double *L;             // LDS base (L_SIZE doubles)
    GPtr G;                // scratch base (workspace slab of this wave)
    long long tprev;       // diagnostic build only (BMPC_PROFILE): last phase stamp
    double ca, cb;         // wave-uniform constants 2 w_a / h^2 and 2 w_a / h (w_a = weights[5]), hoisted out of the phases: a run-time
                           // fp64 division costs ~40 instructions
    int oK0, oK1, oKV, oKV1;   // LDS offsets of the four kinematics records of the current Riccati stage (the buffers rotate, see
                           // wave_backward_blk: two of the four records of stage k are records of stage k+1)
    double *Zc, *Zt, *Dz;  // iterate, trial iterate, Newton direction [N][44]: LDS-resident for N <= 11, else in the scratch slab
    int wv;                // this wave's index in its team (0 in the one-wave program); wave-uniform
    long long deadline;    // real-time instantiation (wave_solve<., true>: the fused closed-loop tick) only: wall-clock count (BMPC_NOW) after
                           // which no further iteration is started; 0 = none
    int last_status, last_it, it_base;   // wave_solve leaves status and iteration count here (wave-uniform) and adds it_base to the count it reports (wave_solve_retry)
#ifdef BMPC_EMU
    int order[64];
    int worder[BMPC_NW];   // team emulator: order in which the waves run a wide phase
#endif
};

// ----------------------------------------------------------------------------------------
// small helpers
// ----------------------------------------------------------------------------------------
template <class PA, class PB> BMPC_D inline void cross3(const PA a, const PB b, double *c) {
    double x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
    c[0] = x; c[1] = y; c[2] = z;
}
template <class PA, class PB> BMPC_D inline double dot3(const PA a, const PB b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
#define BMPC_DEG(x) ((x) * 3.14159265358979323846 / 180.0)
BMPC_D inline double qlim(int i) { return (i == 0 || i == 2 || i == 4) ? BMPC_DEG(165.0) : (i == 6 ? BMPC_DEG(170.0) : BMPC_DEG(115.0)); }
BMPC_D inline double dqlim(int i) { return i <= 1 ? BMPC_DEG(85.0) : (i == 2 ? BMPC_DEG(100.0) : (i == 3 ? BMPC_DEG(75.0) : (i == 4 ? BMPC_DEG(130.0) : BMPC_DEG(135.0)))); }
constexpr double ULIM = 35.0;

// node k (0..N) variable access: node 0 from the parameter vector, node k>=1 = Z[k-1]
BMPC_D inline double ndv(const double *PAR, const POff &po, const double *Z, int k, int zoff, int poff) {
    return k ? Z[(k - 1) * NZ + zoff] : PAR[poff];
}

// sin and cos of a joint angle.  The library sincos() carries the full-range argument reduction (Payne-Hanek path, ~100 instructions a
// call, 7 calls per evaluation point); joint angles are bounded (|q| < 3 rad inside the limits, RobotModel.py:20-28; a trial point of the
// line search may leave them by a little), so a two-constant Cody-Waite reduction by pi/2 is exact here and the classical minimax
// kernels on [-pi/4, pi/4] (the coefficients every libm descended from fdlibm uses) finish in ~30 instructions, error < 1 ulp
// (tests/test_emu.py checks it against libm over [-50, 50]).
#ifndef BMPC_RINT
#define BMPC_RINT(x) __builtin_rint(x)
#endif
BMPC_D inline void bmpc_sincos(double x, double *sn, double *cs) {
    const double k = BMPC_RINT(x * 6.36619772367581382433e-01);
    const double r = (x - k * 1.57079632673412561417e+00) - k * 6.07710050650619224932e-11;
    const double z = r * r;
    const double ps = 8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)));
    const double s = r + (z * r) * (-1.66666666666666324348e-01 + z * ps);
    const double pc = z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 + z * (-2.75573143513906633035e-07 +
                      z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
    const double c = 1.0 - (0.5 * z - z * pc);
    const int n = (int)k;
    const double a = (n & 1) ? c : s, b = (n & 1) ? s : c;
    *sn = (n & 2) ? -a : a; *cs = ((n + 1) & 2) ? -b : b;
}

// ----------------------------------------------------------------------------------------
// kinematics of one evaluation point (sequential, one lane): iiwa14 as a geometric chain,
// joint axes (z,y,z,-y,z,y,z), link offsets along local z (RobotModel.py:9-16).
// Writes the record rec[KREC]: axes, J_v columns, D = d(J dq)/dq, pos, v = J dq, dq.
// ----------------------------------------------------------------------------------------
template <class PR, class PH> BMPC_D inline void kin_point(const double *q, const double *dq, const PR rec, const PH hp) {
    const double preZ[7] = {0.0, 0.1575 + 0.2025, 0.0, 0.2375 + 0.1825, 0.0, 0.2175 + 0.1825, 0.0};
    const double toolZ = 0.081 + (0.071 + 0.145);
    double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, o[3] = {0, 0, 0}, O[7][3], a[7][3], w[7][3];
#pragma unroll
    for (int j = 0; j < 7; j++) {
        for (int i = 0; i < 3; i++) o[i] += R[i][2] * preZ[j];
        double s, c;
        bmpc_sincos(q[j], &s, &c);
        if ((j & 1) == 0) {   // +z joints 0,2,4,6
            for (int i = 0; i < 3; i++) { a[j][i] = R[i][2]; O[j][i] = o[i]; }
            for (int i = 0; i < 3; i++) { double c0 = R[i][0], c1 = R[i][1]; R[i][0] = c * c0 + s * c1; R[i][1] = -s * c0 + c * c1; }
        } else {              // +y joints 1,5 ; -y joint 3
            const double sg = (j == 3) ? -1.0 : 1.0;
            for (int i = 0; i < 3; i++) { a[j][i] = sg * R[i][1]; O[j][i] = o[i]; }
            s *= sg;
            for (int i = 0; i < 3; i++) { double c0 = R[i][0], c2 = R[i][2]; R[i][0] = c * c0 - s * c2; R[i][2] = s * c0 + c * c2; }
        }
    }
    double pos[3], v[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 3; i++) pos[i] = o[i] + R[i][2] * toolZ;
#pragma unroll
    for (int j = 0; j < 7; j++) {
        double r[3];
        for (int i = 0; i < 3; i++) r[i] = pos[i] - O[j][i];
        cross3(a[j], r, w[j]);
        for (int i = 0; i < 3; i++) { v[i] += dq[j] * w[j][i]; v[3 + i] += dq[j] * a[j][i]; }
    }
    // D_v[:,i] = a_i x V>=_i + W<_i x w_i ;  D_w[:,i] = a_i x W>_i   (suffix sums built backwards)
    double Vge[3] = {0, 0, 0}, Wgt[3] = {0, 0, 0}, Wlt[3];
    for (int c = 0; c < 3; c++) Wlt[c] = v[3 + c];   // total angular velocity, peeled from the top
#pragma unroll
    for (int i = 6; i >= 0; i--) {
        double t1[3], t2[3];
        for (int c = 0; c < 3; c++) { Vge[c] += dq[i] * w[i][c]; Wlt[c] -= dq[i] * a[i][c]; }
        if (i == 0) for (int c = 0; c < 3; c++) Wlt[c] = 0.0;   // exact zero (matches the forward prefix sum)
        cross3(a[i], Vge, t1); cross3(Wlt, w[i], t2);
        for (int c = 0; c < 3; c++) rec[KD + c * 7 + i] = t1[c] + t2[c];
        cross3(a[i], Wgt, t1);
        for (int c = 0; c < 3; c++) rec[KD + (3 + c) * 7 + i] = t1[c];
        for (int c = 0; c < 3; c++) Wgt[c] += dq[i] * a[i][c];
    }
#pragma unroll
    for (int j = 0; j < 7; j++) {
        for (int c = 0; c < 3; c++) { rec[KA + c * 7 + j] = a[j][c]; rec[KW + c * 7 + j] = w[j][c]; }
        rec[KDQ + j] = dq[j];
    }
    for (int c = 0; c < 3; c++) rec[KPOS + c] = pos[c];
    for (int c = 0; c < 6; c++) rec[KV + c] = v[c];
    // prefix vectors of the kinematic curvature, hp = [Wlt 8x3 | Vge 7x3 | Wgt 7x3] (kh_qq): Wlt_j = sum_{m<j} dq_m a_m,
    // Vge_j = sum_{m>=j} dq_m w_m, Wgt_j = sum_{m>j} dq_m a_m -- the lane has a, w, dq in registers here; until round 2 every Riccati
    // stage rebuilt them from the record in LDS (node-cost phase 2)
    {
        double wl[3] = {0, 0, 0}, vg[3] = {0, 0, 0}, wg[3] = {0, 0, 0};
#pragma unroll
        for (int j = 0; j < 7; j++) { for (int c = 0; c < 3; c++) { hp[3 * j + c] = wl[c]; wl[c] += dq[j] * a[j][c]; } }
        for (int c = 0; c < 3; c++) hp[21 + c] = wl[c];
#pragma unroll
        for (int j = 6; j >= 0; j--) {
            for (int c = 0; c < 3; c++) { hp[45 + 3 * j + c] = wg[c]; vg[c] += dq[j] * w[j][c]; hp[24 + 3 * j + c] = vg[c]; wg[c] += dq[j] * a[j][c]; }
        }
    }
}

// one entry (ya,yb), ya<=yb, of the Hessian of  mu_p.pos + mu_v.(J_v dq) + mu_w.(J_w dq)  w.r.t. y=(q,dq);
// rec is a kinematics record (read with computed addresses: keep it in LDS)
BMPC_D inline void ldA(const double *rec, int j, double *o) { o[0] = rec[KA + j]; o[1] = rec[KA + 7 + j]; o[2] = rec[KA + 14 + j]; }
BMPC_D inline void ldW(const double *rec, int j, double *o) { o[0] = rec[KW + j]; o[1] = rec[KW + 7 + j]; o[2] = rec[KW + 14 + j]; }
BMPC_D inline double kin_hess_entry(const double *rec, const double *mu_p, const double *mu_v, const double *mu_w, int ya, int yb) {
    const double *dq = rec + KDQ;
    if (yb < 7) {                       // q_i q_l, i <= l
        const int i = ya, l = yb;
        double Wlt_i[3] = {0, 0, 0}, Wil[3] = {0, 0, 0}, Vge[3] = {0, 0, 0}, Wgt[3] = {0, 0, 0};
        for (int j = 0; j < 7; j++) {
            const double d = dq[j];
            double aj[3], wj[3]; ldA(rec, j, aj); ldW(rec, j, wj);
            const double m0 = j < i ? d : 0.0, m1 = (j >= i && j < l) ? d : 0.0, m2 = j >= l ? d : 0.0, m3 = j > l ? d : 0.0;
            for (int c = 0; c < 3; c++) { Wlt_i[c] += m0 * aj[c]; Wil[c] += m1 * aj[c]; Vge[c] += m2 * wj[c]; Wgt[c] += m3 * aj[c]; }
        }
        double ai[3], al[3], wl[3]; ldA(rec, i, ai); ldA(rec, l, al); ldW(rec, l, wl);
        double t[3], u[3], val;
        cross3(ai, wl, t); val = dot3(mu_p, t);
        cross3(Wlt_i, t, u); val += dot3(mu_v, u);
        cross3(al, Vge, t); cross3(ai, t, u); val += dot3(mu_v, u);
        cross3(Wil, wl, t); cross3(ai, t, u); val += dot3(mu_v, u);
        cross3(al, Wgt, t); cross3(ai, t, u); val += dot3(mu_w, u);
        return val;
    } else if (ya < 7) {                // q_i dq_j
        const int i = ya, j = yb - 7;
        const int lo = i <= j ? i : j, hi = i <= j ? j : i;
        double alo[3], whi[3], t[3], val;
        ldA(rec, lo, alo); ldW(rec, hi, whi);
        cross3(alo, whi, t); val = dot3(mu_v, t);
        if (i < j) { double aj[3]; ldA(rec, j, aj); cross3(alo, aj, t); val += dot3(mu_w, t); }
        return val;
    }
    return 0.0;                         // dq dq
}

// ----------------------------------------------------------------------------------------
// node quantities depending on (pos, iw, phi): segment, tubes, errors -> record rr[RREC]
// (bound_mpc_functions.py:13-20,34-40,43-149,152-202; mpc_utils_casadi.py:6-10,52,163)
// ----------------------------------------------------------------------------------------
template <class PR> BMPC_D inline void node_ref(const double *PAR, const POff &po, int S, const double *pos, const double *iw, double phi, const PR rr, int ex) {
    const double *sw = PAR + po.sw;
    int seg = S - 1;
    for (int i = S - 2; i >= 0; i--) if (phi < sw[i + 1]) seg = i;
    int segb = (seg < S - 2) ? seg : (S - 2);
    if (segb < 0) segb = 0;
    const double x = phi - sw[seg];
    rr[RSEG] = (double)seg; rr[RX] = x;
    double dp[6], d[3], rho[3], dh[3], bp1[3], bp2[3], br1[3], br2[3], v1[3], v2[3], v3[3];
    for (int c = 0; c < 6; c++) { dp[c] = PAR[po.dpref + c * S + seg]; rr[RDP + c] = dp[c]; }
    for (int c = 0; c < 3; c++) {
        d[c] = dp[c]; rho[c] = dp[3 + c];
        dh[c] = PAR[po.dpn + c * S + seg]; rr[RDH + c] = dh[c];
        bp1[c] = PAR[po.bp1 + c * S + segb]; bp2[c] = PAR[po.bp2 + c * S + segb];
        br1[c] = PAR[po.br1 + c * S + seg]; br2[c] = PAR[po.br2 + c * S + seg];
        v1[c] = PAR[po.v1 + c * S + seg]; v2[c] = PAR[po.v2 + c * S + seg]; v3[c] = PAR[po.v3 + c * S + seg];
    }
    double b[9], b1[9], b2[9];
    for (int ch = 0; ch < 9; ch++) {   // row S of the a-arrays is undefined in the reference (BoundMPC.py:235-240): row seg <= S-1 is used
        const double a4 = PAR[po.a[0] + ch * (S + 1) + seg], a3 = PAR[po.a[1] + ch * (S + 1) + seg], a2 = PAR[po.a[2] + ch * (S + 1) + seg],
                     a1 = PAR[po.a[3] + ch * (S + 1) + seg], a0 = PAR[po.a[4] + ch * (S + 1) + seg];
        b[ch] = (((a4 * x + a3) * x + a2) * x + a1) * x + a0;
        b1[ch] = ((4 * a4 * x + 3 * a3) * x + 2 * a2) * x + a1;
        b2[ch] = (12 * a4 * x + 6 * a3) * x + 2 * a2;
    }
    const double *jacl = PAR + po.jacl, *jacr = PAR + po.jacr;   // [col][row]
    double rrv[3], l1[3], l2[3], l3[3];
    for (int c = 0; c < 3; c++) {
        rrv[c] = jacr[0 * 3 + c] * rho[0] + jacr[1 * 3 + c] * rho[1] + jacr[2 * 3 + c] * rho[2];
        l1[c] = l2[c] = l3[c] = 0;
        for (int r = 0; r < 3; r++) { const double jl = jacl[c * 3 + r]; l1[c] += jl * v1[r]; l2[c] += jl * v2[r]; l3[c] += jl * v3[r]; }
        rr[RRR + c] = rrv[c]; rr[RL2 + c] = l2[c];
    }
    double ep[3], dlt[3], er[3], erpar[3];
    for (int c = 0; c < 3; c++) { ep[c] = pos[c] - (PAR[po.pref + c * S + seg] + d[c] * x); rr[REP + c] = ep[c]; }
    for (int r = 0; r < 3; r++) {
        double s = 0;
        for (int c = 0; c < 3; c++)
            s += jacl[c * 3 + r] * (iw[c] - PAR[po.p0 + 3 + c]) - jacr[c * 3 + r] * (PAR[po.pref + (3 + c) * S + seg] + rho[c] * x - PAR[po.iwref0 + c]);
        dlt[r] = s; er[r] = PAR[po.dtau + r] + s; rr[RER + r] = er[r];
    }
    const double s1 = dot3(dlt, v1), s2 = dot3(dlt, v2), s3 = dot3(dlt, v3);
    const double *ipar = PAR + po.ipar + 3 * seg, *io1 = PAR + po.io1 + 3 * seg, *io2 = PAR + po.io2 + 3 * seg;
    for (int c = 0; c < 3; c++) { erpar[c] = ipar[c] + s2 * dh[c]; rr[RERPAR + c] = erpar[c]; }
    const double aa = 100.0 * (phi - (PAR[po.phimax] - 0.02));
    const double sig = 1.0 / (1.0 + BMPC_EXP(-aa));
    rr[RSIG] = sig; rr[RSIG1] = 100.0 * sig * (1.0 - sig); rr[RSIG2] = 100.0 * (100.0 * sig * (1.0 - sig)) * (1.0 - 2.0 * sig);
    const double dhdh = dot3(dh, dh), b1b1 = dot3(br1, br1), b2b2 = dot3(br2, br2);
    const double v1rr = dot3(v1, rrv), v2rr = dot3(v2, rrv), v3rr = dot3(v3, rrv);
    rr[RV2RR] = v2rr;
    // m = 0 tangential orientation
    rr[RC + 0] = dot3(dh, ipar) + s2 * dhdh;
    for (int c = 0; c < 3; c++) rr[RGC + 0 * 4 + c] = dhdh * l2[c];
    rr[RGC + 0 * 4 + 3] = -dhdh * v2rr; rr[RC2 + 0] = 0;
    { const double wv = b[8], sg = wv >= 0 ? 1.0 : -1.0; rr[RWD + 0] = sg * wv; rr[RW1 + 0] = sg * b1[8]; rr[RW2 + 0] = sg * b2[8]; }
    for (int m = 0; m < 2; m++) {   // orthogonal position
        const double *bp = m ? bp2 : bp1;
        const double off = 0.5 * (b[m] + b[2 + m]), off1 = 0.5 * (b1[m] + b1[2 + m]), off2 = 0.5 * (b2[m] + b2[2 + m]);
        const double hw = 0.5 * (b[m] - b[2 + m]), sg = hw >= 0 ? 1.0 : -1.0;
        rr[RC + 1 + m] = dot3(ep, bp) - off;
        for (int c = 0; c < 3; c++) rr[RGC + (1 + m) * 4 + c] = bp[c];
        rr[RGC + (1 + m) * 4 + 3] = -dot3(d, bp) - off1; rr[RC2 + 1 + m] = -off2;
        rr[RWD + 1 + m] = sg * hw; rr[RW1 + 1 + m] = sg * 0.5 * (b1[m] - b1[2 + m]); rr[RW2 + 1 + m] = sg * 0.5 * (b2[m] - b2[2 + m]);
    }
    for (int m = 0; m < 2; m++) {   // orthogonal orientation
        const double *br = m ? br2 : br1, *io = m ? io2 : io1, *l = m ? l3 : l1;
        const double bb = m ? b2b2 : b1b1, sc = m ? s3 : s1, vrr = m ? v3rr : v1rr;
        const double off = 0.5 * (b[4 + m] + b[6 + m]), off1 = 0.5 * (b1[4 + m] + b1[6 + m]), off2 = 0.5 * (b2[4 + m] + b2[6 + m]);
        const double hw = 0.5 * (b[4 + m] - b[6 + m]), sg = hw >= 0 ? 1.0 : -1.0;
        rr[RC + 3 + m] = dot3(br, io) + sc * bb - off;
        for (int c = 0; c < 3; c++) rr[RGC + (3 + m) * 4 + c] = bb * l[c];
        rr[RGC + (3 + m) * 4 + 3] = -bb * vrr - off1; rr[RC2 + 3 + m] = -off2;
        rr[RWD + 3 + m] = sg * hw; rr[RW1 + 3 + m] = sg * 0.5 * (b1[4 + m] - b1[6 + m]); rr[RW2 + 3 + m] = sg * 0.5 * (b2[4 + m] - b2[6 + m]);
    }
    // ---- multiplier-independent Hessian blocks of the tracking cost over (pos, iw, phi) (objective_function with the blended
    //      errors e_obj = sig e + (1 - sig) e_par; exact second-order terms when ex) ----
    {
        const double *w = PAR + po.w;
        const double sig1 = 100.0 * sig * (1.0 - sig), sig2 = 100.0 * sig1 * (1.0 - 2.0 * sig);
        const double dde = dot3(d, ep), dd = dot3(d, d);
        double jp[3][3], jr[3][3], jpf[3], jrf[3], epo[3], ero[3], eperp[3], erd[3];
        for (int r = 0; r < 3; r++) {
            eperp[r] = ep[r] - dde * d[r]; erd[r] = er[r] - erpar[r];
            epo[r] = sig * ep[r] + (1 - sig) * dde * d[r]; ero[r] = sig * er[r] + (1 - sig) * erpar[r];
            jpf[r] = -(sig * d[r] + (1 - sig) * dd * d[r]) + sig1 * eperp[r];
            jrf[r] = -sig * rrv[r] - (1 - sig) * dh[r] * v2rr + sig1 * erd[r];
            for (int a = 0; a < 3; a++) { jp[r][a] = (r == a ? sig : 0.0) + (1 - sig) * d[r] * d[a]; jr[r][a] = sig * jacl[a * 3 + r] + (1 - sig) * dh[r] * l2[a]; }
        }
        const double depo = dot3(d, epo), dhero = dot3(dh, ero);
        double spf = 0, srf = 0, spp = 0, srr = 0, dpdp = 0;
        for (int a = 0; a < 3; a++) {
            for (int b2_ = 0; b2_ < 3; b2_++) {
                double sp = 0, sr = 0;
                for (int r = 0; r < 3; r++) { sp += jp[r][a] * jp[r][b2_]; sr += jr[r][a] * jr[r][b2_]; }
                rr[RHPPG + a * 3 + b2_] = 2 * w[0] * sp; rr[RHRRG + a * 3 + b2_] = 2 * w[1] * sr;
            }
            double sp = 0, sr = 0;
            for (int r = 0; r < 3; r++) { sp += jp[r][a] * jpf[r]; sr += jr[r][a] * jrf[r]; }
            double hp = 2 * w[0] * sp, hr = 2 * w[1] * sr;
            if (ex) {
                double jl = 0; for (int r = 0; r < 3; r++) jl += ero[r] * jacl[a * 3 + r];
                hp += 2 * w[0] * sig1 * (epo[a] - depo * d[a]); hr += 2 * w[1] * sig1 * (jl - dhero * l2[a]);
            }
            rr[RHPFG + a] = hp; rr[RHRFG + a] = hr;
            spf += jpf[a] * jpf[a]; srf += jrf[a] * jrf[a];
            spp += epo[a] * (sig2 * eperp[a] - 2 * sig1 * (d[a] - dd * d[a]));
            srr += ero[a] * (sig2 * erd[a] + 2 * sig1 * (-rrv[a] + dh[a] * v2rr));
        }
        for (int c = 0; c < 6; c++) dpdp += dp[c] * dp[c];
        double hff = 2 * w[0] * spf + 2 * w[1] * srf;
        if (ex) hff += 2 * w[0] * spp + 2 * w[1] * srr;
        rr[RHFFG] = hff; rr[RDPDP] = dpdp;
    }
}
// tube row m uses pos (m = 1,2) or iw (m = 0,3,4) as its 3-vector variable
BMPC_D inline int tube_voff(int m) { return (m == 1 || m == 2) ? ZPOS : ZIW; }

// Box rows (i < ITUBE) are +-Z[src] - lim: descriptor without memory accesses, so that a batch of rows can issue all its
// loads first.  Tube rows (i >= ITUBE) read the node's reference record instead.
BMPC_D inline void ineq_box_row(const double *PAR, const POff &po, int i, int &src, double &sgn, double &lim) {
    if (i < IJL) { src = ZJ + i; sgn = 1.0; lim = ULIM; }
    else if (i < IQU) { src = ZJ + i - IJL; sgn = -1.0; lim = ULIM; }
    else if (i < IQL) { src = ZQ + i - IQU; sgn = 1.0; lim = qlim(i - IQU); }
    else if (i < IDQU) { src = ZQ + i - IQL; sgn = -1.0; lim = qlim(i - IQL); }
    else if (i < IDQL) { src = ZDQ + i - IDQU; sgn = 1.0; lim = dqlim(i - IDQU); }
    else if (i < IPHI0) { src = ZDQ + i - IDQL; sgn = -1.0; lim = dqlim(i - IDQL); }
    else if (i == IPHI0) { src = ZPHI; sgn = -1.0; lim = 0.0; }
    else if (i == IPHIMAX) { src = ZPHI; sgn = 1.0; lim = PAR[po.phimax]; }
    else if (i == IDPHIMAX) { src = ZDPHI; sgn = 1.0; lim = PAR[po.dphimax]; }
    else { src = 0; sgn = 0.0; lim = 0.0; }
}
// value of internal inequality row i (0..56) at node variables Zn with reference record rr
BMPC_D inline double ineq_val(const double *PAR, const POff &po, const double *Zn, const double *rr, int i) {
    if (i < IJL) return Zn[ZJ + i] - ULIM;
    if (i < IQU) return -Zn[ZJ + i - IJL] - ULIM;
    if (i < IQL) return Zn[ZQ + i - IQU] - qlim(i - IQU);
    if (i < IDQU) return -Zn[ZQ + i - IQL] - qlim(i - IQL);
    if (i < IDQL) return Zn[ZDQ + i - IDQU] - dqlim(i - IDQU);
    if (i < IPHI0) return -Zn[ZDQ + i - IDQL] - dqlim(i - IDQL);
    if (i == IPHI0) return -Zn[ZPHI];
    if (i == IPHIMAX) return Zn[ZPHI] - PAR[po.phimax];
    if (i == IDPHIMAX) return Zn[ZDPHI] - PAR[po.dphimax];
    const int m = (i - ITUBE) >> 1;
    return ((i - ITUBE) & 1) ? (-rr[RC + m] - rr[RWD + m]) : (rr[RC + m] - rr[RWD + m]);
}
// grad h_i . dZ
BMPC_D inline double ineq_dir(const double *dZ, const double *rr, int i) {
    if (i < IJL) return dZ[ZJ + i];
    if (i < IQU) return -dZ[ZJ + i - IJL];
    if (i < IQL) return dZ[ZQ + i - IQU];
    if (i < IDQU) return -dZ[ZQ + i - IQL];
    if (i < IDQL) return dZ[ZDQ + i - IDQU];
    if (i < IPHI0) return -dZ[ZDQ + i - IDQL];
    if (i == IPHI0) return -dZ[ZPHI];
    if (i == IPHIMAX) return dZ[ZPHI];
    if (i == IDPHIMAX) return dZ[ZDPHI];
    const int m = (i - ITUBE) >> 1, vo = tube_voff(m);
    const double s = rr[RGC + m * 4 + 0] * dZ[vo] + rr[RGC + m * 4 + 1] * dZ[vo + 1] + rr[RGC + m * 4 + 2] * dZ[vo + 2] + rr[RGC + m * 4 + 3] * dZ[ZPHI];
    return (((i - ITUBE) & 1) ? -s : s) - rr[RW1 + m] * dZ[ZPHI];
}
BMPC_D inline bool bmpc_finite(double v) { return BMPC_FABS(v) <= 1.7976931348623157e308; }      // (false for NaN and +-inf)

// integrator-chain coefficients CF[f'][f]: row field f' (q,dq,ddq,j of the next node) vs column field f (q,dq,ddq,j,u)
BMPC_D inline double chain_cf(double h, int fr, int fc) {
    const double h2 = h * h, h3 = h2 * h;
    if (fr == 0) return fc == 0 ? 1.0 : fc == 1 ? h : fc == 2 ? h2 / 2 : fc == 3 ? h3 / 8 : h3 / 24;
    if (fr == 1) return fc == 0 ? 0.0 : fc == 1 ? 1.0 : fc == 2 ? h : fc == 3 ? h2 / 3 : h2 / 6;
    if (fr == 2) return fc <= 1 ? 0.0 : fc == 2 ? 1.0 : h / 2;
    return fc == 4 ? 1.0 : 0.0;
}
BMPC_D inline int srow(int f, int i) { return i < 7 ? f * 7 + i : 28 + f; }   // reduced-state index of (field, chain)
// column of a reduced-state row in the jerk rows GS / gains KS of a Riccati stage: chain-major (the four fields of a chain are adjacent),
// so that a chain-pair lane reads its 4 rows / 4 columns of the Schur update as contiguous words; iota rows and the gradient column keep
// their index.  gcol: from (field, chain); pcol: from the reduced-state index; prow: back.
BMPC_D inline int gcol(int f, int i) { return i * 4 + f; }
BMPC_D inline int pcol(int r) { return r < 28 ? (r % 7) * 4 + r / 7 : r; }
BMPC_D inline int prow(int c) { return c < 28 ? (c & 3) * 7 + (c >> 2) : c; }

// per-problem tables and constants that depend only on the parameter vector (already in LDS)
BMPC_D inline void wave_init_tables(Wave &W, const POff &po) {
    double *L = W.L;
    LANES_BEGIN
        if (lane < NI) {
            int src; double sgn, lim; ineq_box_row(L + L_PAR, po, lane, src, sgn, lim);
            if (lane >= IQU && lane < IPHI0) lim -= W.o.bound_margin;      // joint position and velocity rows
            L[L_ROWT + lane] = sgn; L[L_ROWT + NI + lane] = lim; L[L_ROWT + 2 * NI + lane] = (double)src;
        }
    LANES_END
    LANES_BEGIN
        if (lane < 20) L[L_CFT + lane] = chain_cf(W.h, lane / 5, lane % 5);
#if BMPC_NW == 1
        // t6 of the Riccati sweep: stage 0 reads it behind a 0/1 factor and only the stages k >= 1 write it -- at N = 1 nobody does, and what
        // LDS held before (a NaN of an earlier kernel) would pass the factor (0 x NaN)
        if (lane < 6) L[L_T6 + lane] = 0.0;
#endif
        if (lane < NS) {
            const int r = lane;
            const int z = r < 7 ? ZQ + r : (r < 14 ? ZDQ + r - 7 : (r < SJ ? ZDDQ + r - SDDQ : (r < SPHI ? ZJ + r - SJ : (r == SPHI ? ZPHI : (r == SDPHI ? ZDPHI :
                          (r == SDDPHI ? ZDDPHI : (r == SJPHI ? ZJPHI : ZIW + r - SIOTA)))))));
            // packed with the row's defect source in g (bits 8..15) and the "carries no defect" flag (bit 16): functions of a
            // lane-dependent integer compile into divergent branches, a table look-up does not
            const bool io = r >= SIOTA;
            const int gsrc = r < SJ ? r : ((r >= SPHI && r <= SDDPHI) ? GPHI + r - SPHI : (io ? GIW + r - SIOTA : 0));
            const int zero = ((r >= SJ && r < SPHI) || r == SJPHI) ? 1 : 0;          // jerk states carry no defect
            const int fr = r < 28 ? r / 7 : (r < SIOTA ? r - 28 : 0), ir = r < 28 ? r % 7 : (r < SIOTA ? 7 : 0);   // (field, chain) of a chain row: bits 17..19, 20..22
            L[L_ZMAP + r] = (double)(z + (gsrc << 8) + (zero << 16) + (fr << 17) + (ir << 20));
        }
    LANES_END
    TEAM_SYNC();      // (teams: every wave wrote the same words; nobody reads the tables or the parameter vector before all are in)
    W.ca = 2 * L[L_PAR + po.w + 5] / (W.h * W.h); W.cb = 2 * L[L_PAR + po.w + 5] / W.h;
}

// ---- how every wave program begins: where the iterate lives, and a point (p, x) taken in ----
// iterate, trial iterate and direction: in LDS (ZLDS) or in the workspace slab
template <bool ZLDS>
BMPC_D inline void wave_iterate_ptrs(Wave &W, const Scr &sc) {
    double *L = W.L; const GPtr G = W.G;
    if (ZLDS) { W.Zc = L + L_ZL; W.Zt = L + L_PB; W.Dz = L + L_PB + 512; } else { W.Zc = (G + sc.Z).ptr(); W.Zt = (G + sc.ZT).ptr(); W.Dz = (G + sc.DZ).ptr(); }
}
// "a solve begins": coalesced load of the parameter vector into LDS and of x into the iterate, then the tables.  The warm-start conversion
// (bmpc_dual.inl) and the certificate (bmpc_kkt.inl) start here and wave_solve with twin lines (see there); the sensitivities (bmpc_sens.inl)
// load p + t dp instead.
template <bool ZLDS>
BMPC_D inline void wave_load_point(Wave &W, const POff &po, const Scr &sc, const double *p, const double *x) {
    double *L = W.L; const int S = W.S, np = po.size, nw = W.N * NZ;
    wave_iterate_ptrs<ZLDS>(W, sc);
    WIDE_BEGIN
        for (int id = wl; id < np; id += WS) L[L_PAR + (ZLDS ? id : lds_index_of_p(S, id, L_ZL))] = p[id];
        for (int id = wl; id < nw; id += WS) W.Zc[id] = x[id];
    WIDE_END
    wave_init_tables(W, po);
}

// ---- the output map: the internal rows in the reference's conventions (casadi nlpsol), one entry per call ----
// Read: the iterate W.Zc, the parameter vector, G / LAM and the reference records of the last evaluation, the multipliers nu [N][57] at sc.NUm.
// Caller: wave_certify (bmpc_kkt.inl); the output pass of wave_solve keeps twin lines (see there).  The multiplier map dual_row (bmpc_dual.inl)
// is the inverse.
// entry id of [N][43]: the constraint value gv and its multiplier lv
BMPC_D inline void out_g_entry(const Wave &W, const POff &po, const Scr &sc, int id, double &gv, double &lv) {
    const double *PAR = W.L + L_PAR; const LPtr WL = BMPC_WL(W);
    const int k = id / NG, i = id - k * NG;
    const double *Zn = W.Zc + k * NZ; const LPtr rr = WL + sc.REF + k * RREC, nu = WL + sc.NUm + k * NI;
    if (i < NE) { gv = WL[sc.G + k * NE + i]; lv = WL[sc.LAM + k * NE + i]; }
    else if (i == 36) { gv = Zn[ZPHI] - PAR[po.phimax]; lv = nu[IPHIMAX]; }
    else if (i == 37) { gv = Zn[ZDPHI] - PAR[po.dphimax]; lv = nu[IDPHIMAX]; }
    else { const int m = i - 38; const double c = rr[RC + m], wd = rr[RWD + m]; gv = c * c - wd * wd; lv = wd > 0 ? (nu[ITUBE + 2 * m] + nu[ITUBE + 2 * m + 1]) / (2 * wd) : 0.0; }
}
// entry id of [N][44]: the multiplier of the variable's bounds (0 for an unbounded one)
BMPC_D inline double out_lam_x_entry(const Wave &W, const Scr &sc, int id) {
    const int k = id / NZ, z = id - k * NZ; const LPtr nu = BMPC_WL(W) + sc.NUm + k * NI; double v = 0;
    if (z < 8) v = nu[IJU + z] - nu[IJL + z]; else if (z < ZDQ) v = nu[IQU + z - ZQ] - nu[IQL + z - ZQ];
    else if (z < ZDDQ) v = nu[IDQU + z - ZDQ] - nu[IDQL + z - ZDQ]; else if (z == ZPHI) v = -nu[IPHI0];
    return v;
}

#ifndef BMPC_RU
#define BMPC_RU 9   // N=10: all 570 rows of a pass in one trip per lane (6: two trips; 10 starts to spill); +2 % (profiles/r02_n_rows_in_flight_ab.txt)
#endif
static_assert(64 * BMPC_RU >= 40 * 8, "the first batch of a row pass must cover the N * NU <= 320 jerk-gradient entries (KKT pass)");
static_assert(64 * BMPC_RU >= 10 * 57, "one batch must cover the 570 multiplier rows of a ten-node pass (wave_node_grad_wide)");
constexpr int RU = BMPC_RU;   // rows of a lane-strided pass kept in flight per lane (loads of a batch are issued before their first use)
constexpr int RUW = cdiv_(RU, NW);   // the same for the wide passes of a team: NW x 64 lanes share the rows
struct LaneRegs { double mc[16]; double pf[24]; double ghd; };   // ghd: the lane's share of (QP gradient) . dZ, accumulated by the forward sweep   // pf: software prefetch of the next stage's inputs (global -> registers -> LDS)   // a lane's 4x4 state block of M, kept in registers between the M and the Schur phases
// the register sets a wave program hands to its sweeps: the lane's own on the GPU, one per lane of the team in the emulator
#ifdef BMPC_EMU
#define BMPC_LANE_REGS(name) LaneRegs name[WS]
#else
#define BMPC_LANE_REGS(name) LaneRegs name[1]
#endif

// ----------------------------------------------------------------------------------------
// wave-uniform deterministic reductions through LDS (RED has 6 x 64 slots)
// ----------------------------------------------------------------------------------------
// fixed-order pairwise trees over the 64 slots (order identical in the emulator -> bitwise reproducible)
#ifdef BMPC_WAVE_RED
// GPU: every lane reads its own slot and the wave reduces by a butterfly of cross-lane exchanges (xor 8,16,32,1,2,4): exactly
// the tree written out below (fp addition is commutative, so every lane ends with the same bits), without 64 LDS reads per lane
BMPC_D inline double red_sum(const double *r) {
    double v = r[BMPC_LANE_ID];
    v += __shfl_xor(v, 8); v += __shfl_xor(v, 16); v += __shfl_xor(v, 32); v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
    return v;
}
BMPC_D inline double red_max(const double *r) {
    double v = r[BMPC_LANE_ID];
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = BMPC_FMAX(v, __shfl_xor(v, m));
    return v;
}
BMPC_D inline double red_min(const double *r) {
    double v = r[BMPC_LANE_ID];
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = BMPC_FMIN(v, __shfl_xor(v, m));
    return v;
}
// Wide passes of a team: a wave reduces the partials of its 64 lanes in registers (the one-wave tree) and leaves ONE word per wave and
// slot in LDS; behind the barrier every wave folds the NW words in a fixed order -- every wave of the team ends with the same bits.
BMPC_D inline double wave_sum(double v) {
    v += __shfl_xor(v, 8); v += __shfl_xor(v, 16); v += __shfl_xor(v, 32); v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
    return v;
}
BMPC_D inline double wave_max(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = BMPC_FMAX(v, __shfl_xor(v, m));
    return v;
}
BMPC_D inline double wave_min(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = BMPC_FMIN(v, __shfl_xor(v, m));
    return v;
}
BMPC_D inline double fold_sum(const double *r) { double v = r[0];
#pragma unroll
    for (int w = 1; w < NW; w++) v += r[w]; return v; }
BMPC_D inline double fold_max(const double *r) { double v = r[0];
#pragma unroll
    for (int w = 1; w < NW; w++) v = BMPC_FMAX(v, r[w]); return v; }
BMPC_D inline double fold_min(const double *r) { double v = r[0];
#pragma unroll
    for (int w = 1; w < NW; w++) v = BMPC_FMIN(v, r[w]); return v; }
#else
BMPC_D inline double red_sum(const double *r) {
    double a[8];
#pragma unroll
    for (int i = 0; i < 8; i++) a[i] = ((r[i] + r[i + 8]) + (r[i + 16] + r[i + 24])) + ((r[i + 32] + r[i + 40]) + (r[i + 48] + r[i + 56]));
    return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}
BMPC_D inline double red_max(const double *r) { double s = r[0];
#pragma unroll
    for (int i = 1; i < 64; i++) s = BMPC_FMAX(s, r[i]); return s; }
BMPC_D inline double red_min(const double *r) { double s = r[0];
#pragma unroll
    for (int i = 1; i < 64; i++) s = BMPC_FMIN(s, r[i]); return s; }
// wide-pass partials of a team (NW x 64 per-lane slots in the emulator): the one-wave tree per wave, then a left fold over the waves -- the
// order of the GPU's wave_sum / fold_sum
BMPC_D inline double red_sum_w(const double *r) { double v = red_sum(r); for (int w = 1; w < NW; w++) v += red_sum(r + 64 * w); return v; }
BMPC_D inline double red_max_w(const double *r) { double s = r[0]; for (int i = 1; i < WS; i++) s = BMPC_FMAX(s, r[i]); return s; }
BMPC_D inline double red_min_w(const double *r) { double s = r[0]; for (int i = 1; i < WS; i++) s = BMPC_FMIN(s, r[i]); return s; }
#endif
// partial of this lane into slot `slot` of a wide-pass reduction area (L_REDW / L_KKPW), and the reduced value afterwards (behind the barrier)
#if BMPC_NW == 1
#define WRED_PUT_SUM(area, slot, v) L[(area) + (slot) * 64 + wl] = (v)
#define WRED_PUT_MAX(area, slot, v) L[(area) + (slot) * 64 + wl] = (v)
#define WRED_PUT_MIN(area, slot, v) L[(area) + (slot) * 64 + wl] = (v)
#define WRED_GET_SUM(area, slot) red_sum(L + (area) + (slot) * 64)
#define WRED_GET_MAX(area, slot) red_max(L + (area) + (slot) * 64)
#define WRED_GET_MIN(area, slot) red_min(L + (area) + (slot) * 64)
#elif defined(BMPC_EMU)
#define WRED_PUT_SUM(area, slot, v) L[(area) + (slot) * WS + wl] = (v)
#define WRED_PUT_MAX(area, slot, v) L[(area) + (slot) * WS + wl] = (v)
#define WRED_PUT_MIN(area, slot, v) L[(area) + (slot) * WS + wl] = (v)
#define WRED_GET_SUM(area, slot) red_sum_w(L + (area) + (slot) * WS)
#define WRED_GET_MAX(area, slot) red_max_w(L + (area) + (slot) * WS)
#define WRED_GET_MIN(area, slot) red_min_w(L + (area) + (slot) * WS)
#else
#define WRED_PUT_SUM(area, slot, v) L[(area) + (slot) * WRED_STRIDE + W.wv] = wave_sum(v)      // (every lane stores the wave's value to the wave's word)
#define WRED_PUT_MAX(area, slot, v) L[(area) + (slot) * WRED_STRIDE + W.wv] = wave_max(v)
#define WRED_PUT_MIN(area, slot, v) L[(area) + (slot) * WRED_STRIDE + W.wv] = wave_min(v)
#define WRED_GET_SUM(area, slot) fold_sum(L + (area) + (slot) * WRED_STRIDE)
#define WRED_GET_MAX(area, slot) fold_max(L + (area) + (slot) * WRED_STRIDE)
#define WRED_GET_MIN(area, slot) fold_min(L + (area) + (slot) * WRED_STRIDE)
#endif

// ========================================================================================
//                                   the wave program
// ========================================================================================

// kinematics of point pt (pt < N: predicted point of node pt+1, with the dynamics residuals of q, dq, ddq; pt >= N: velocity point of node
// pt - N): record -> KIN, curvature prefix vectors -> KHPG
BMPC_D inline void eval_kin_lane(Wave &W, const POff &po, const Scr &sc, const double *Zs, int oG, int pt) {
    const int N = W.N; const double h = W.h, h2 = h * h, h3 = h2 * h;
    const GPtr G = W.G; const LPtr WL = BMPC_WL(W); const double *PAR = W.L + L_PAR;
    if (pt < 2 * N) {
        const int k = pt < N ? pt : pt - N;
        double q[7], dq[7];
        if (pt < N) {   // predicted point of node k+1 (jerk_trajectory_casadi.py closed form; bound_mpc_functions.py:254-260)
            const LPtr gk = WL + oG + k * NE;
            const double *Zn = Zs + k * NZ;
            for (int i = 0; i < 7; i++) {
                const double q0 = ndv(PAR, po, Zs, k, ZQ + i, po.q0 + i), d0 = ndv(PAR, po, Zs, k, ZDQ + i, po.dq0 + i),
                             dd0 = ndv(PAR, po, Zs, k, ZDDQ + i, po.ddq0 + i), j0 = ndv(PAR, po, Zs, k, ZJ + i, po.jerk + i), j1 = Zn[ZJ + i];
                q[i] = q0 + h * d0 + h2 / 2 * dd0 + h3 / 8 * j0 + h3 / 24 * j1;
                dq[i] = d0 + h * dd0 + h2 / 3 * j0 + h2 / 6 * j1;
                const double ddqn = dd0 + h / 2 * (j0 + j1);
                gk[GQ + i] = q[i] - Zn[ZQ + i]; gk[GDQ + i] = dq[i] - Zn[ZDQ + i]; gk[GDDQ + i] = ddqn - Zn[ZDDQ + i];
            }
        } else {
            for (int i = 0; i < 7; i++) { q[i] = ndv(PAR, po, Zs, k, ZQ + i, po.q0 + i); dq[i] = ndv(PAR, po, Zs, k, ZDQ + i, po.dq0 + i); }
        }
        kin_point(q, dq, WL + sc.KIN + pt * KREC, G + sc.KHPG + pt * 72);
    }
}

// Node phase of the evaluation for ONE lane = node k (index k: node k+1): `lifted`: the twelve residual rows of the lifted variables
// (pos, i-omega, v: these read the kinematics records) -- or, for projected trial points, the lifted variables themselves --; `refs`: the
// path-parameter residuals, the node's reference record and its objective term (returned).  The two parts share no data except through
// `project`, so a team runs `refs` on a second wave beside the kinematics.
BMPC_D inline double eval_node_lane(Wave &W, const POff &po, const Scr &sc, double *Zs, int oG, bool project, int k, bool lifted, bool refs) {
    const int N = W.N; const double h = W.h, h2 = h * h, h3 = h2 * h;
    const GPtr G = W.G; const LPtr WL = BMPC_WL(W); const double *PAR = W.L + L_PAR;
    double fk = 0;
    {
            double *Zn = Zs + k * NZ; const LPtr kp = WL + sc.KIN + k * KREC, kv = WL + sc.KIN + (N + k) * KREC;
            const LPtr gk = WL + oG + k * NE, rr = WL + sc.REF + k * RREC;
            if (lifted) {
            if (project) {
                double iw[3] = {PAR[po.p0 + 3], PAR[po.p0 + 4], PAR[po.p0 + 5]};
                for (int j = 0; j <= k; j++) {
                    const LPtr kpj = WL + sc.KIN + j * KREC, kvj = WL + sc.KIN + (N + j) * KREC;
                    for (int i = 0; i < 3; i++) iw[i] = iw[i] + 0.5 * h * (kvj[KV + 3 + i] + kpj[KV + 3 + i]);
                }
                for (int i = 0; i < 3; i++) { Zn[ZPOS + i] = kp[KPOS + i]; gk[GPOS + i] = 0.0; Zn[ZIW + i] = iw[i]; gk[GIW + i] = 0.0; }
                for (int i = 0; i < 6; i++) { Zn[ZV + i] = kp[KV + i]; gk[GV + i] = 0.0; }
            } else {
                // all twelve record entries first, then the stores: a store between two loads of the workspace makes the second load wait
                // for it (they may alias as far as the compiler knows), and this block was twelve dependent round trips
                double kpos[3], kvel[6], kvw[3];
#pragma unroll
                for (int i = 0; i < 3; i++) { kpos[i] = kp[KPOS + i]; kvw[i] = kv[KV + 3 + i]; }
#pragma unroll
                for (int i = 0; i < 6; i++) kvel[i] = kp[KV + i];
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    gk[GPOS + i] = kpos[i] - Zn[ZPOS + i];
                    gk[GIW + i] = ndv(PAR, po, Zs, k, ZIW + i, po.p0 + 3 + i) + 0.5 * h * (kvw[i] + kvel[3 + i]) - Zn[ZIW + i];
                }
#pragma unroll
                for (int i = 0; i < 6; i++) gk[GV + i] = kvel[i] - Zn[ZV + i];
            }
            }
            if (refs) {
            const double ph = ndv(PAR, po, Zs, k, ZPHI, po.phi0), dph = ndv(PAR, po, Zs, k, ZDPHI, po.phi0 + 1),
                         ddph = ndv(PAR, po, Zs, k, ZDDPHI, po.phi0 + 2), jp0 = ndv(PAR, po, Zs, k, ZJPHI, po.jerkphi), jp1 = Zn[ZJPHI];
            gk[GPHI] = ph + h * dph + h2 / 2 * ddph + h3 / 8 * jp0 + h3 / 24 * jp1 - Zn[ZPHI];
            gk[GDPHI] = dph + h * ddph + h2 / 3 * jp0 + h2 / 6 * jp1 - Zn[ZDPHI];
            gk[GDDPHI] = ddph + h / 2 * (jp0 + jp1) - Zn[ZDDPHI];
            node_ref(PAR, po, W.S, Zn + ZPOS, Zn + ZIW, Zn[ZPHI], rr, W.o.exact_hessian);
            // objective of node k+1 (bound_mpc_functions.py:205-246; casadi_ocp_formulation.py:227-265)
            const double *w = PAR + po.w; const LPtr d = rr + RDP;
            const double sig = rr[RSIG], dde = dot3(d, rr + REP);
            double epo[3], ero[3];
            for (int c = 0; c < 3; c++) { epo[c] = sig * rr[REP + c] + (1 - sig) * dde * d[c]; ero[c] = sig * rr[RER + c] + (1 - sig) * rr[RERPAR + c]; }
            fk = w[1] * dot3(ero, ero) + w[0] * dot3(epo, epo);
            for (int c = 0; c < 6; c++) {
                const double vp = (project && k > 0) ? WL[sc.KIN + (k - 1) * KREC + KV + c] : ndv(PAR, po, Zs, k, ZV + c, po.v0 + c);
                const double rv = Zn[ZV + c] - Zn[ZDPHI] * d[c], ra = (Zn[ZV + c] - vp) / h - Zn[ZDDPHI] * d[c];
                fk += w[2] * rv * rv + w[5] * ra * ra;
            }
            for (int i = 0; i < 7; i++) {
                const double dqd = Zn[ZQ + i] - PAR[po.qd + i];
                fk += w[10] * dqd * dqd + w[11] * Zn[ZDQ + i] * Zn[ZDQ + i] + w[12] * Zn[ZDDQ + i] * Zn[ZDDQ + i] + w[13] * Zn[ZJ + i] * Zn[ZJ + i];
            }
            const double e0 = PAR[po.xphid] - Zn[ZPHI], e1 = PAR[po.xphid + 1] - Zn[ZDPHI], e2 = PAR[po.xphid + 2] - Zn[ZDDPHI];
            fk += w[6] * e0 * e0 + w[7] * e1 * e1 + w[8] * e2 * e2 + w[9] * Zn[ZJPHI] * Zn[ZJPHI];
            }
    }
    return fk;
}

// Evaluate at Zs: kinematic records, node references, equality residuals Gd[N][36], inequality
// values Hd[N][57]; returns the objective (wave-uniform).
// project (trial points of the line search after a rejected first trial; oracle/bmpc_oracle.c eval_values): the lifted variables
// pos, i-omega, v of every node are overwritten in Zs by what their defining equalities give for the trial (q, dq), so those 12
// residual rows are exactly zero.  One lane per node: a lane writes only its own node's entries and reads its neighbours' projected
// values from the kinematics records of phase 1 (v of the previous node; the i-omega recursion as a prefix sum from node 0), never
// from Zs -- no cross-lane dependence inside the phase.
// ls (trial points of the line search): the row pass also forms the trial slacks tt = t + alpha dt (-> TT) and the two sums the filter
// needs -- theta = ||c||_1 + ||h + tt||_1 and the barrier term -mu sum log tt -- from the values it has in registers, and leaves their
// per-lane parts in L_RED + 64 / + 128: the trial used to cost two more passes over the rows (slacks before, sums after the
// evaluation), each a dependent round trip to the workspace.
struct LsRows { double alpha, mu; bool el; };      // el: restoration phase (elastic rows: trial e -> ET, theta and the barrier sum include them)
BMPC_D inline double wave_eval(Wave &W, const POff &po, const Scr &sc, double *Zs, int oG, int oH, bool project, const LsRows *ls = nullptr) {
    const int N = W.N; const double h = W.h, h2 = h * h, h3 = h2 * h;
    double *L = W.L; const GPtr G = W.G; const LPtr WL = BMPC_WL(W);
    const double *PAR = L + L_PAR;
    // one lane per kinematics point: 2 N points; the points past the first 64 (N > 32 only) take a second phase
    SOLO_BEGIN(0)
    LANES_BEGIN
        eval_kin_lane(W, po, sc, Zs, oG, lane);
    LANES_END
    if (2 * N > 64) {
        LANES_BEGIN
            eval_kin_lane(W, po, sc, Zs, oG, 64 + lane);
        LANES_END
    }
    SOLO_END
    if (NW > 1 && !project) {      // team: references and objective of the nodes on wave 1, beside the kinematics
        SOLO_BEGIN(1)
        LANES_BEGIN
            double fk = 0;
            if (lane < N) fk = eval_node_lane(W, po, sc, Zs, oG, false, lane, false, true);
            L[L_RED + lane] = fk;
        LANES_END
        SOLO_END
    }
    TEAM_SYNC();
    BMPC_PROF(W, 25);
    if (NW == 1 || project) {
        // one wave (and the projected trial points of a team, which need the kinematics first): the whole node phase in one lane per node
        SOLO_BEGIN(0)
        LANES_BEGIN
            double fk = 0;
            if (lane < N) fk = eval_node_lane(W, po, sc, Zs, oG, project, lane, true, true);
            L[L_RED + lane] = fk;
        LANES_END
        SOLO_END
        TEAM_SYNC();
    } else {
        // team: the references / objective part of the node phase does not read the kinematics records (pos, iw, v are variables of Z):
        // wave 1 ran it beside the kinematics of wave 0 (above); what is left are the twelve lifted residual rows per node
        SOLO_BEGIN(0)
        LANES_BEGIN
            if (lane < N) eval_node_lane(W, po, sc, Zs, oG, false, lane, true, false);
        LANES_END
        SOLO_END
        TEAM_SYNC();
    }
    const double f = red_sum(L + L_RED);
    BMPC_PROF(W, 26);
    WIDE_BEGIN   // inequality values, lane-strided rows (wide: over the lanes of the whole team), RUW rows in flight per lane: all loads of a batch are issued before the first use
        double th = 0, br = 0;
        // wave-uniform trip counts (rows past the end are clamped duplicates): a lane-dependent loop exit makes the compiler restore the
        // exec mask behind the loop, and that is where this toolchain has placed register copies under the stale mask (build.py lint_isa)
        const int trips_i = (N * NI + WS * RUW - 1) / (WS * RUW), trips_e = (N * NE + WS * RUW - 1) / (WS * RUW);
        double the = 0;
        if (ls) {   // 1-norm of the equality residuals (written by the node phase): read ahead of this pass's stores, which its loads would
                    // otherwise have to wait for
            for (int tr_ = 0; tr_ < trips_e; tr_++) {
                const int base = wl + tr_ * WS * RUW;
                double gv[RUW];
#pragma unroll
                for (int u = 0; u < RUW; u++) { const int id0 = base + WS * u; gv[u] = WL[oG + (id0 < N * NE ? id0 : N * NE - 1)]; }
#pragma unroll
                for (int u = 0; u < RUW; u++) the += base + WS * u < N * NE ? BMPC_FABS(gv[u]) : 0.0;
            }
        }
        for (int tr_ = 0; tr_ < trips_i; tr_++) {
            const int base = wl + tr_ * WS * RUW;
            double zv[RUW], rc[RUW], rw[RUW], sg[RUW], lm[RUW], tv[RUW], dv[RUW];
#pragma unroll
            // rows past the end are clamped to the last row: they load, compute and store exactly what its owner does (no exec-mask
            // branch anywhere in the pass)
            for (int u = 0; u < RUW; u++) {
                const int id0 = base + WS * u, id = id0 < N * NI ? id0 : N * NI - 1;
                const int k = id / NI, i = id - k * NI;
                const int m = i >= ITUBE ? (i - ITUBE) >> 1 : 0;
                sg[u] = L[L_ROWT + i]; lm[u] = L[L_ROWT + NI + i];
                zv[u] = Zs[k * NZ + (int)L[L_ROWT + 2 * NI + i]];
                const LPtr rr = WL + sc.REF + k * RREC;
                rc[u] = rr[RC + m]; rw[u] = rr[RWD + m];
                if (ls) { tv[u] = WL[sc.T + id]; dv[u] = WL[sc.DT + id]; }      // wave-uniform condition
            }
            double ev[RUW], dev[RUW], eprod = 1.0, esum = 0.0;
            if (ls && ls->el) {      // (wave-uniform; restoration phase only)
#pragma unroll
                for (int u = 0; u < RUW; u++) { const int id0 = base + WS * u, id = id0 < N * NI ? id0 : N * NI - 1; ev[u] = G[sc.E + id]; dev[u] = G[sc.DE + id]; }
            }
            double tprod = 1.0;
#pragma unroll
            for (int u = 0; u < RUW; u++) {
                const int id0 = base + WS * u, id = id0 < N * NI ? id0 : N * NI - 1;
                const int i = id % NI;
                // 0/1 factors instead of a select between the two row formulas (their operands are loads: a select becomes a branch nest)
                const double mt = i >= ITUBE ? 1.0 : 0.0, s2 = (i >= ITUBE && ((i - ITUBE) & 1)) ? -1.0 : 1.0;
                const double hv = mt * (s2 * rc[u] - rw[u]) + (1.0 - mt) * (sg[u] * zv[u] - lm[u]);
                WL[oH + id] = hv;
                if (ls) {
                    const double tt = tv[u] + ls->alpha * dv[u]; const bool ok_ = id0 < N * NI;
                    WL[sc.TT + id] = tt;
                    if (ls->el) {
                        const double et = ev[u] + ls->alpha * dev[u];
                        G[sc.ET + id] = et;
                        th += ok_ ? BMPC_FABS(hv + tt - et) : 0.0; tprod *= ok_ ? tt : 1.0; eprod *= ok_ ? et : 1.0; esum += ok_ ? et : 0.0;
                    } else {
                    th += ok_ ? BMPC_FABS(hv + tt) : 0.0; tprod *= ok_ ? tt : 1.0;
                    }
                }
            }
            if (ls) br -= ls->mu * BMPC_LOG(tprod);      // one log per batch of RU slacks: sum of logs = log of the product (t in [1e-12, 1e2])
            if (ls && ls->el) br += RESTO_RHO * esum - ls->mu * BMPC_LOG(eprod);
        }
        if (ls) { WRED_PUT_SUM(L_REDW, 1, th + the); WRED_PUT_SUM(L_REDW, 2, br); }
    WIDE_END
    return f;
}

// mu_q, mu_dq of stage kk (node kk -> kk+1) from lam_kk and the predicted-point record, into L_MU[0..15]
// (lanes 0..7; chain 7 = path parameter)
// (value form: chain ch of 0..7, 7 = path parameter; branch-free on a clamped joint index)
BMPC_D inline void stage_mu_vals(const double *lam, const double *kp, double h, int ch, double &muq, double &mudq) {
    const int i = ch < 7 ? ch : 0;
    double s = lam[GQ + i], s2 = lam[GDQ + i];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double mv = lam[GV + c], mw = lam[GW + c] + 0.5 * h * lam[GIW + c];
        s += kp[KW + c * 7 + i] * lam[GPOS + c] + kp[KD + c * 7 + i] * mv + kp[KD + (3 + c) * 7 + i] * mw;
        s2 += kp[KW + c * 7 + i] * mv + kp[KA + c * 7 + i] * mw;
    }
    const double lp = lam[GPHI], ld = lam[GDPHI];
    muq = ch < 7 ? s : lp; mudq = ch < 7 ? s2 : ld;
}
BMPC_D inline void stage_mu(Wave &W, const double *lam, const double *kp, int lane) {
    double *L = W.L;
    // branch-free: lanes >= 8 repeat chain 0 (identical values, duplicate stores); chain 7 (path parameter) selects its own pair
    const int ch = lane < 8 ? lane : 0;
    double muq, mudq; stage_mu_vals(lam, kp, W.h, ch, muq, mudq);
    L[L_MU + ch] = muq; L[L_MU + 8 + ch] = mudq;
}

// d(f + nu.h)/dZ of every node -> GH [N][44] (the reference's objective_function / error_function, casadi_ocp_formulation.py:227-265,
// bound_mpc_functions.py:152-246, differentiated; multipliers nu of the 57 internal inequality rows staged in LDS at L_PB).
// One lane per (node, component) item in four homogeneous kinds -- box rows (jerk, q, dq, ddq: weight x value + multiplier pair),
// Cartesian-velocity rows (which also carry the acceleration term of the NEXT node: no second pass over GH), pos / iw rows, and the
// three path-parameter rows -- instead of one lane per node running all 44 components in sequence on 10 of 64 lanes (rounds 1-2:
// 9.3 k cycles per call + a read-modify-write pass over GH).  The only loads from the workspace are entries of the reference records,
// issued together ahead of the arithmetic: one dependent round trip per call.
BMPC_D inline void wave_node_grad_wide(Wave &W, const POff &po, const Scr &sc, int oNU, bool use_hat, double mu) {
    const int N = W.N; const double h = W.h, hinv = 1.0 / h;
    double *L = W.L; const GPtr G = W.G; const LPtr WL = BMPC_WL(W);
    const double *PAR = L + L_PAR, *w = PAR + po.w, *Zs = W.Zc;
    const int npass = (N + 9) / 10;
    for (int pass = 0; pass < npass; pass++) {
    // the multipliers of the pass's ten nodes (570 rows: one batch) are staged through LDS with coalesced loads (the value-function block
    // area is free outside the Riccati sweep): one lane per item would otherwise issue scattered global loads of its own.  use_hat: the
    // multiplier estimate mu / t + (nu / t) r of the QP gradient instead of the stored multiplier.
    WIDE_BEGIN
        const int first = pass * 10 * NI, last = N * NI - 1;
        double a_[RUW], b_[RUW];
#pragma unroll
        for (int u = 0; u < RUW; u++) {
            const int id0 = first + wl + WS * u, id = id0 < last ? id0 : last;
            a_[u] = WL[(use_hat ? sc.TI : oNU) + id]; b_[u] = WL[sc.SR + id];
        }
#pragma unroll
        for (int u = 0; u < RUW; u++) { const int j0 = wl + WS * u, j = j0 < 10 * NI ? j0 : 10 * NI - 1; const double v = use_hat ? mu * a_[u] + b_[u] : a_[u];
                                       L[j0 < 10 * NI ? L_PB + j : L_DUMMY] = v; }
    WIDE_END
    const double *NUV = L + L_PB - pass * 10 * NI;      // row k of the staged block: NUV + k NI for the nodes 10 pass .. 10 pass + 9
    // (teams: the item kinds are dealt out to the waves -- wave 0: v and pos / iw rows; wave 1: path-parameter rows; box rows: trip u on
    // wave u mod NW -- every test below is wave-uniform, and with one wave all of them are true)
    WIDE_BEGIN
        // item maps (one integer division each per call): v / pos+iw rows 6 per node, path-parameter rows 3 per node, box rows 29 per node
        const int k6 = lane / 6, c6 = lane - 6 * k6, k3 = lane / 3, a3 = lane - 3 * k3, k29 = lane / 29, z29 = lane - 29 * k29;
        {
            const int kv0 = 10 * pass + k6, kv = kv0 < N ? kv0 : N - 1, kn = kv < N - 1 ? kv + 1 : kv;
            const int kf0 = 10 * pass + k3, kf = kf0 < N ? kf0 : N - 1;
            const bool on6 = lane < 60, on3 = lane < 30;
            // ---- loads from the workspace: reference-record entries of the items' nodes ----
            const LPtr rv_ = WL + sc.REF + kv * RREC, rn_ = WL + sc.REF + kn * RREC, rf_ = WL + sc.REF + kf * RREC;
            const double dv = rv_[RDP + c6], dn = rn_[RDP + c6];                              // v rows: dp_d[c] of the node and of the next node
            const int cc = c6 < 3 ? c6 : c6 - 3;                                              // pos / iw rows: coordinate
            double pd[3], pdh[3], pep[3], per_[3], ppar[3], pl2[3], prr[3], pgc[5];
#pragma unroll
            for (int c = 0; c < 3; c++) { pd[c] = rv_[RDP + c]; pdh[c] = rv_[RDH + c]; pep[c] = rv_[REP + c]; per_[c] = rv_[RER + c]; ppar[c] = rv_[RERPAR + c]; pl2[c] = rv_[RL2 + c]; prr[c] = rv_[RRR + c]; }
#pragma unroll
            for (int m = 0; m < 5; m++) pgc[m] = rv_[RGC + m * 4 + cc];
            const double psig = rv_[RSIG];
            double fd[6], fdh[3], fep[3], fer[3], fpar[3], frr[3], fg3[5], fw1[5];
#pragma unroll
            for (int c = 0; c < 6; c++) fd[c] = rf_[RDP + c];
#pragma unroll
            for (int c = 0; c < 3; c++) { fdh[c] = rf_[RDH + c]; fep[c] = rf_[REP + c]; fer[c] = rf_[RER + c]; fpar[c] = rf_[RERPAR + c]; frr[c] = rf_[RRR + c]; }
#pragma unroll
            for (int m = 0; m < 5; m++) { fg3[m] = rf_[RGC + m * 4 + 3]; fw1[m] = rf_[RW1 + m]; }
            const double fsig = rf_[RSIG], fsig1 = rf_[RSIG1], fv2rr = rf_[RV2RR];
            // ---- v rows: tracking of v_ref = dphi dp_d and a_ref = ddphi dp_d, plus the acceleration term of node k+1 (which holds v_k) ----
            if (NW == 1 || W.wv == 0) {
                const double *Zn = Zs + kv * NZ, *Z1 = Zs + kn * NZ;
                const double vk = Zn[ZV + c6], vp = kv ? Zs[(kv - 1) * NZ + ZV + c6] : PAR[po.v0 + c6];
                const double rv = vk - Zn[ZDPHI] * dv, ra = (vk - vp) * hinv - Zn[ZDDPHI] * dv;
                const double ra1 = (Z1[ZV + c6] - vk) * hinv - Z1[ZDDPHI] * dn;
                const double gz = 2 * w[2] * rv + 2 * w[5] * ra * hinv;
                const double gn = kv < N - 1 ? -2 * w[5] * ra1 * hinv : 0.0;
                WL[on6 ? sc.GH + kv * NZ + ZV + c6 : sc.GVP + 6] = gz + gn;      // lanes without an item write to a spare word
            }
            // ---- pos rows (c6 < 3) and iw rows (c6 >= 3): blended tracking errors + tube rows ----
            if (NW == 1 || W.wv == 0) {
                const double *nuv = NUV + kv * NI;
                const double dde = dot3(pd, pep), dd = dot3(pd, pd);
                double epo[3], ero[3];
#pragma unroll
                for (int c = 0; c < 3; c++) { epo[c] = psig * pep[c] + (1 - psig) * dde * pd[c]; ero[c] = psig * per_[c] + (1 - psig) * ppar[c]; }
                const double depo = dot3(pd, epo), dhero = dot3(pdh, ero);
                const double *jacl = PAR + po.jacl;
                double sj = 0;
#pragma unroll
                for (int r = 0; r < 3; r++) sj += psig * jacl[cc * 3 + r] * ero[r];
                const double gpos = 2 * w[0] * (psig * epo[cc] + (1 - psig) * depo * pd[cc]);
                const double giw = 2 * w[1] * (sj + (1 - psig) * dhero * pl2[cc]);
                double tp = 0, ti = 0;
#pragma unroll
                for (int m = 0; m < 5; m++) {
                    const double dnu = nuv[ITUBE + 2 * m] - nuv[ITUBE + 2 * m + 1];
                    if (m == 1 || m == 2) tp += dnu * pgc[m]; else ti += dnu * pgc[m];
                }
                const bool isp = c6 < 3;
                WL[on6 ? sc.GH + kv * NZ + (isp ? ZPOS : ZIW) + cc : sc.GVP + 6] = isp ? gpos + tp : giw + ti;
            }
            // ---- path-parameter rows phi (a3 = 0), dphi (1), ddphi (2) ----
            if (NW == 1 || W.wv == 1 % NW) {
                const double *Zn = Zs + kf * NZ, *nuv = NUV + kf * NI;
                const double dde = dot3(fd, fep), dd = dot3(fd, fd);
                double epo[3], ero[3], eperp[3], erd[3];
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    eperp[c] = fep[c] - dde * fd[c]; epo[c] = fsig * fep[c] + (1 - fsig) * dde * fd[c];
                    erd[c] = fer[c] - fpar[c]; ero[c] = fsig * fer[c] + (1 - fsig) * fpar[c];
                }
                const double depo = dot3(fd, epo), dhero = dot3(fdh, ero);
                double gphi = 2 * w[0] * (-(fsig * depo + (1 - fsig) * depo * dd) + fsig1 * dot3(eperp, epo));
                gphi += 2 * w[1] * (-fsig * dot3(frr, ero) - (1 - fsig) * fv2rr * dhero + fsig1 * dot3(erd, ero));
                gphi += -2 * w[6] * (PAR[po.xphid + 0] - Zn[ZPHI]);
                gphi += -nuv[IPHI0] + nuv[IPHIMAX];
#pragma unroll
                for (int m = 0; m < 5; m++) {
                    const double nu_u = nuv[ITUBE + 2 * m], nu_l = nuv[ITUBE + 2 * m + 1];
                    gphi += (nu_u - nu_l) * fg3[m] - (nu_u + nu_l) * fw1[m];
                }
                double gdphi = 0, gddphi = 0;
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    const double vk = Zn[ZV + c], vp = kf ? Zs[(kf - 1) * NZ + ZV + c] : PAR[po.v0 + c];
                    const double rv = vk - Zn[ZDPHI] * fd[c], ra = (vk - vp) * hinv - Zn[ZDDPHI] * fd[c];
                    gdphi += -2 * w[2] * rv * fd[c]; gddphi += -2 * w[5] * ra * fd[c];
                }
                gdphi += -2 * w[7] * (PAR[po.xphid + 1] - Zn[ZDPHI]) + nuv[IDPHIMAX];
                gddphi += -2 * w[8] * (PAR[po.xphid + 2] - Zn[ZDDPHI]);
                WL[on3 ? sc.GH + kf * NZ + ZPHI + a3 : sc.GVP + 6] = a3 == 0 ? gphi : (a3 == 1 ? gdphi : gddphi);
            }
            // ---- box rows: jerk (8), q, dq, ddq (7 each): 2 weight (value - target) + upper - lower multiplier; two nodes per trip ----
#pragma unroll
            for (int u = 0; u < 5; u++) if (NW == 1 || u % NW == W.wv) {
                const int kb0 = 10 * pass + 2 * u + k29, kb = kb0 < N ? kb0 : N - 1, z = z29;
                const bool on = lane < 58;
                const double *Zn = Zs + kb * NZ, *nuv = NUV + kb * NI;
                // kind of the component: weight index, target, multiplier rows (ddq has none: both indices point at a row pair that cancels)
                const bool isJ = z < 7, isJp = z == 7, isQ = z >= ZQ && z < ZDQ, isDQ = z >= ZDQ && z < ZDDQ;
                int wi = 12; wi = isDQ ? 11 : wi; wi = isQ ? 10 : wi; wi = isJp ? 9 : wi; wi = isJ ? 13 : wi;
                int iu = IJU, il = IJU; iu = isDQ ? IDQU + z - ZDQ : iu; il = isDQ ? IDQL + z - ZDQ : il; iu = isQ ? IQU + z - ZQ : iu; il = isQ ? IQL + z - ZQ : il;
                iu = (isJ || isJp) ? IJU + z : iu; il = (isJ || isJp) ? IJL + z : il;
                const double tgt = (isQ ? 1.0 : 0.0) * PAR[po.qd + (isQ ? z - ZQ : 0)];      // clamped index + 0/1 factor: no load under a branch
                const double v = 2 * w[wi] * (Zn[z] - tgt) + (nuv[iu] - nuv[il]);
                WL[on ? sc.GH + kb * NZ + z : sc.GVP + 6] = v;
            }
        }
    WIDE_END
    }
}

// inputs of adjoint stage j: gradient row j, kinematics records of node j+1 (predicted point and velocity point); j = -1: record
// of node 0.  Register set PO (0 or 5) of the lane's prefetch array; LDS buffer set by stage parity.
#define BMPC_ADJ_LOADS(j_, PO_) { double *pf = LR[LIDX].pf + (PO_); const int j0 = (j_), j = j0 >= -1 ? j0 : -1, jc = j >= 0 ? j : 0, jr = j + 1 < N ? j + 1 : N - 1; \
    const int l2 = lane < KREC - 64 ? 64 + lane : KREC - 1; \
    pf[0] = WL[sc.GH + jc * NZ + (lane < NZ ? lane : NZ - 1)]; \
    pf[1] = WL[sc.KIN + jr * KREC + lane]; pf[2] = WL[sc.KIN + jr * KREC + l2]; \
    pf[3] = WL[sc.KIN + (N + jr) * KREC + lane]; pf[4] = WL[sc.KIN + (N + jr) * KREC + l2]; }
#define BMPC_ADJ_COMMIT(j_, PO_) { const double *pf = LR[LIDX].pf + (PO_); const int odd_ = (N - 1 - (j_)) & 1, l2 = lane < KREC - 64 ? 64 + lane : KREC - 1; \
    const int kb = odd_ ? L_K1 : L_K0, vb = odd_ ? L_KV1 : L_KV; \
    L[L_ST + (odd_ ? ST_Z : ST_GH) + (lane < NZ ? lane : NZ - 1)] = pf[0]; \
    L[kb + lane] = pf[1]; L[vb + lane] = pf[3]; L[kb + l2] = pf[2]; L[vb + l2] = pf[4]; }
// Component table of the adjoint sweep, one packed integer per component z of Z (built per sweep into the part of the staging
// area that is idle during the adjoint, under the latency of the sweep's first loads): bits 0-1 field fc (0 q, 1 dq, 2 ddq,
// 3 jerk), 2-4 chain i, 5 "is a chain state", 6 "couples with iota through Ehat" (i < 7, fc <= 1), 7 "is an iw component",
// 8-9 its coordinate, 10 "is a jerk", 11-16 row in lam (or jerk slot), 17-22 index of the ddq multiplier, 23-29 Ehat column base.
BMPC_D inline int adjoint_zcode(int z) {
    const int f = z < 7 ? 3 : (z == ZJPHI ? 3 : (z < ZDQ ? 0 : (z < ZDDQ ? 1 : (z < ZPOS ? 2 : (z >= ZPHI ? z - ZPHI : -1)))));
    const int i = z < 7 ? z : (z == ZJPHI ? 7 : (z < ZDQ ? z - ZQ : (z < ZDDQ ? z - ZDQ : (z < ZPOS ? z - ZDDQ : (z >= ZPHI ? 7 : 0)))));
    const bool has = f >= 0; const int fc = has ? f : 0, i7 = i < 7 ? i : 0;
    const bool isIw = z >= ZIW && z < ZIW + 3; const int cw = isIw ? z - ZIW : 0;
    const bool isJ = z < 7 || z == ZJPHI;
    const int ee = isJ ? (z < 7 ? z : 7) : (z < ZPOS ? z - ZQ : (z < ZPHI ? GPOS + (z - ZPOS) : GPHI + (z - ZPHI)));
    const int mdd = i < 7 ? GDDQ + i : GDDPHI, eb = fc == 0 ? KD + 21 + i7 : KA + i7;
    return fc | (i << 2) | ((has ? 1 : 0) << 5) | (((i < 7 && fc <= 1) ? 1 : 0) << 6) | ((isIw ? 1 : 0) << 7) | (cw << 8) | ((isJ ? 1 : 0) << 10)
         | (ee << 11) | (mdd << 17) | (eb << 23);
}
// one stage of the sequential adjoint sweep (one phase); PO = register set that holds the inputs of stage k-1
template <int PO>
BMPC_D inline void adjoint_stage(Wave &W, const Scr &sc, LaneRegs *LR, int k) {
    const int N = W.N; const double h = W.h, h2 = h * h, h3 = h2 * h;
    double *L = W.L; const GPtr G = W.G; const LPtr WL = BMPC_WL(W);
    const int odd = (N - 1 - k) & 1;
    double *lam1 = L + L_ST + (odd ? ST_LAM0 : ST_LAM1);     // lam_{k+1} (written one step earlier)
    double *lam0 = L + L_ST + (odd ? ST_LAM1 : ST_LAM0);     // lam_k (written now)
    const double *k0 = L + (odd ? L_K1 : L_K0), *kvb = L + (odd ? L_KV1 : L_KV), *ghb = L + L_ST + (odd ? ST_Z : ST_GH);
    LANES_BEGIN   // one lane per component of Z; its kind comes from the component table (adjoint_ztab), decoded with shifts: integer
                  // indices and 0/1 factors, no exec-mask branch
        // mu_q, mu_dq of the lane's own chain, in the lane (round 4): until round 3 eight lanes computed them in a phase of their own and
        // every lane read them back from LDS -- a whole phase boundary (store, fence, load latency) per stage of a sweep whose stages are
        // shorter than a round trip.  Lanes 0..43: the chain of their component; lanes 44..51 (the jerk role below): chain lane - 44.
        double muq, mudq;
        {
            const bool on = lane < NZ; const int z = on ? lane : 0;
            const double *kv = kvb;
            const int code = (int)L[L_ST + ST_REF + z];
            const int fc = code & 3, i = (code >> 2) & 7, cw = (code >> 8) & 3, ee = (code >> 11) & 63;
            const double mh = ((code >> 5) & 1) ? 1.0 : 0.0, me = ((code >> 6) & 1) ? 1.0 : 0.0, mi = ((code >> 7) & 1) ? 1.0 : 0.0;
            const bool isJ = ((code >> 10) & 1) != 0, nxt = k < N - 1;
            const double mdd = lam1[(code >> 17) & 63];
            stage_mu_vals(lam1, k0, h, on ? i : ((lane - NZ) & 7), muq, mudq);
            const double chainv = L[L_CFT + fc] * muq + L[L_CFT + 5 + fc] * mudq + L[L_CFT + 10 + fc] * mdd;
            const int eb = (code >> 23) & 127;                                  // Ehat column of (q_i) or (dq_i): rows at stride 7
            double e = 0;
#pragma unroll
            for (int c = 0; c < 3; c++) e += kv[eb + c * 7] * lam1[GIW + c];
            double tot = ghb[z];
            const double addv = mh * (chainv + me * (0.5 * h * e)) + mi * lam1[GIW + cw];
            if (nxt) tot += addv;               // wave-uniform condition (lam_{k+1} does not exist at the last stage)
            // Stores without branches: one LDS store and one global store per lane, the row kind selects the ADDRESS.
            // jerk rows: the residual of node k still lacks the term of the NEXT sweep step (stage k-1 -> k); it is parked in LDS
            // and completed there (a global read-modify-write would wait for this store to land and come back); their global
            // store goes to a spare slot of the node's GVP row.  Off-lanes evaluate row 0 (a jerk row) with the multipliers of ANOTHER
            // chain (theirs of the jerk role below): their LDS store goes to the dummy word, their global store to the spare slot anyway.
            {
                const int lo_ = on ? (isJ ? L_RJP + (k & 1) * 8 + ee : (int)(lam0 - L) + ee) : L_DUMMY;
                const int gdst = isJ ? sc.GVP + k * 8 + 6 : sc.LAM + k * NE + ee;
                L[lo_] = tot; WL[gdst] = tot;
            }
        }
        {   // jerk of node k+2 enters stage k+1 (lanes 44..51; everyone else, and the last stage, write to the spare GVP slot)
            const bool on = lane >= NZ && lane < NZ + 8 && k < N - 1; const int i = on ? lane - NZ : 0;
            const double mdd = lam1[i < 7 ? GDDQ + i : GDDPHI];
            const double v = L[L_RJP + ((k + 1) & 1) * 8 + i] + (h3 / 24 * muq + h2 / 6 * mudq + h / 2 * mdd);      // (lanes 44..51 hold their own chain's pair)
            WL[on ? sc.RJ + (k + 1) * NU + i : sc.GVP + k * 8 + 7] = v;
        }
        // inputs of the next stage into the other LDS buffer set (loaded two stages ago), then the loads for three stages ahead
        // into the registers this just freed
        BMPC_ADJ_COMMIT(k - 1, PO)
        BMPC_ADJ_LOADS(k - 3, PO)
    LANES_END
}

// Adjoint sweep with multipliers nu (scratch offset oNU; scale = 0 -> objective only is NOT supported here):
// LAM[N][36], RJ[N][8]; GH receives d(f + nu.h)/dZ.
BMPC_D inline void wave_adjoint(Wave &W, const POff &po, const Scr &sc, int oNU, bool use_hat, double mu, LaneRegs *LR) {
    const int N = W.N; const double h = W.h, h2 = h * h, h3 = h2 * h;
    double *L = W.L; const GPtr G = W.G; const LPtr WL = BMPC_WL(W);
    const double *PAR = L + L_PAR, *Zs = W.Zc;
    wave_node_grad_wide(W, po, sc, oNU, use_hat, mu);
    BMPC_PROF(W, 27);
    if (use_hat) return;   // QP gradient only
    SOLO_BEGIN(0)          // the sweep itself is one wave's (teams: the others wait at the barrier behind it)
    // sequential sweep; lam_{k+1} lives in LDS (ping-pong ST_LAM0/ST_LAM1).  A blocking global load per stage would cost a full
    // memory round trip with nothing else in flight, and the stages are short (the round trip is longer than a stage), so the
    // inputs of a stage are loaded into registers THREE stages ahead (two register sets, the stage loop is unrolled by two) and
    // committed to LDS one stage ahead, double-buffered by stage parity (records: L_K0/L_KV and L_K1/L_KV1, gradient row: ST_GH
    // and ST_Z); the commit burst and the next loads ride at the end of a stage's main phase: two phases per stage.
    LANES_BEGIN
        BMPC_ADJ_LOADS(N - 1, 0)
        BMPC_ADJ_LOADS(N - 2, 5)
        L[L_ST + ST_REF + (lane < NZ ? lane : NZ - 1)] = (double)adjoint_zcode(lane < NZ ? lane : NZ - 1);
    LANES_END
    LANES_BEGIN
        BMPC_ADJ_COMMIT(N - 1, 0)
        BMPC_ADJ_LOADS(N - 3, 0)
    LANES_END
    {
        int k = N - 1;
        for (; k >= 1; k -= 2) { adjoint_stage<5>(W, sc, LR, k); adjoint_stage<0>(W, sc, LR, k - 1); }
        if (k == 0) adjoint_stage<5>(W, sc, LR, 0);
    }
    const double *lamz = L + L_ST + (((N - 1) & 1) ? ST_LAM1 : ST_LAM0);   // lam_0
    LANES_BEGIN
        stage_mu(W, lamz, L + ((N & 1) ? L_K1 : L_K0), lane);      // record of node 0: committed as "stage -1"
    LANES_END
    LANES_BEGIN
        if (lane < 8) {
            const int i = lane;
            const double mdd = i < 7 ? lamz[GDDQ + i] : lamz[GDDPHI];
            WL[sc.RJ + i] = L[L_RJP + i] + (h3 / 24 * L[L_MU + i] + h2 / 6 * L[L_MU + 8 + i] + h / 2 * mdd);
        }
    LANES_END
    SOLO_END
    TEAM_SYNC();
}

// ========================================================================================
// Block ("chain-pair") form of the node cost and of the Riccati stage.
// The stage map of the chain part is the Kronecker product I_8 (x) CF of the 4-state integrator chain, so the
// congruence F^T P' F acts independently on every 4x4 block P'[(.,i)][(.,l)] of a pair of chains (i,l):
// ONE LANE PER PAIR (64 pairs = 64 lanes), 16 LDS reads + ~200 FMAs per lane and stage.  A lane always evaluates
// the canonical pair (min,max) and transposes, so the stored matrix is symmetric bit for bit.
// ========================================================================================
BMPC_D inline int pbi(int f, int g, int i, int l) { return (f * 4 + g) * 64 + i * 8 + l; }   // plane-major: lane-contiguous
BMPC_D inline int pci(int a, int f, int i) { return a * 32 + f * 8 + i; }
BMPC_D inline int mci(int a, int f, int i) { return a * 40 + f * 8 + i; }                      // f = 0..4

// Curvature entries sum lambda . d2F / dy_a dy_b of the kinematic maps of a stage, from the stage's record and its table of per-joint vectors
// (KHV_*, formed once per iterate by wave_stage_data_wide): with x . (y x z) = z . (x x y) every double cross product of the direct
// differentiation turns into a dot product of one vector of joint i with one of joint l.  i <= l.
BMPC_D inline double kh_qq(const double *rec, const double *khv, int i, int l) {
    double val = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) val += rec[KW + c * 7 + l] * khv[KHV_X + c * 7 + i] + khv[KHV_Y + c * 7 + l] * khv[KHV_N + c * 7 + i] + khv[KHV_G + c * 7 + l] * khv[KHV_O + c * 7 + i];
    return val;
}
BMPC_D inline double kh_qdq(const double *rec, const double *khv, int i, int j) {   // d2/(dq_i d dq_j)
    const int lo = i <= j ? i : j, hi = i <= j ? j : i;
    double v1 = 0, v2 = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) { v1 += rec[KW + c * 7 + hi] * khv[KHV_N + c * 7 + lo]; v2 += rec[KA + c * 7 + j] * khv[KHV_O + c * 7 + lo]; }
    return v1 + (i < j ? 1.0 : 0.0) * v2;      // 0/1 factor, not a branch around loads
}
// the same with only the angular-velocity multiplier of the velocity point of the NEXT node (its position and linear-velocity rows belong to
// that node's own cost); at the last stage that multiplier is zero and so is o'
BMPC_D inline double kh_qq_w(const double *khv, int i, int l) {
    double val = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) val += khv[KHV_G1 + c * 7 + l] * khv[KHV_O1 + c * 7 + i];
    return val;
}
BMPC_D inline double kh_qdq_w(const double *rec1, const double *khv, int i, int j) {
    const int lo = i <= j ? i : j;
    double v2 = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) v2 += rec1[KA + c * 7 + j] * khv[KHV_O1 + c * 7 + lo];
    return (i < j ? 1.0 : 0.0) * v2;
}
BMPC_D inline void kh_prefix(const double *rec, double *hp) {   // sequential over the 7 joints (one lane)
    double wl[3] = {0, 0, 0};
    for (int j = 0; j < 7; j++) { for (int c = 0; c < 3; c++) { hp[3 * j + c] = wl[c]; wl[c] += rec[KDQ + j] * rec[KA + c * 7 + j]; } }
    for (int c = 0; c < 3; c++) hp[21 + c] = wl[c];
    double vg[3] = {0, 0, 0}, wg[3] = {0, 0, 0};
    for (int j = 6; j >= 0; j--) {
        for (int c = 0; c < 3; c++) { hp[45 + 3 * j + c] = wg[c]; vg[c] += rec[KDQ + j] * rec[KW + c * 7 + j]; hp[24 + 3 * j + c] = vg[c];
                                      wg[c] += rec[KDQ + j] * rec[KA + c * 7 + j]; }
    }
}

// q~ row r (reduced-state row, r < NS) of the node cost: gl mapped through the lifting Jacobians; rows >= 14 only copy.
// Predicated straight-line code: every lane evaluates the (q, dq)-row formula on a clamped row.
// (inputs as pointers: gl = the node's Z-space gradient (44), WY = curvature table (14 x 14), gy = (g_q, g_dq): rows 0..13 of g, K0 = record)
BMPC_D inline double node_q_row_p(const double *L, const double *gl, const double *WY, const double *gy, const double *K0, int r, double h, int ex) {
    const bool heavy = r < 14; const int a = heavy ? r : 0; const bool isq = a < 7; const int ai = isq ? a : a - 7;
    const double base = gl[(int)L[L_ZMAP + r] & 255];
    double t1 = 0, t2 = 0, t3 = 0, sW = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        t1 += K0[KW + c * 7 + ai] * gl[ZPOS + c];
        t2 += K0[(isq ? KD + (3 + c) * 7 : KA + c * 7) + ai] * gl[ZIW + c];
    }
#pragma unroll
    for (int c6 = 0; c6 < 6; c6++) t3 += K0[(isq ? KD + c6 * 7 : (c6 < 3 ? KW + c6 * 7 : KA + (c6 - 3) * 7)) + ai] * gl[ZV + c6];
    if (ex) {
#pragma unroll
        for (int b2 = 0; b2 < 14; b2++) sW += WY[a * 14 + b2] * gy[b2];
    }
    return base + (heavy ? (isq ? t1 : 0.0) + 0.5 * h * t2 + t3 - sW : 0.0);
}
BMPC_D inline double node_q_row(const double *L, const double *K0, int r, double h, int ex, int oWY = L_WY) {      // from the one-wave sweep's staging areas
    return node_q_row_p(L, L + L_NC + NC_GL, L + oWY, L + L_ST + ST_G, K0, r, h, ex);
}
// t6 = C rdyn (6): the rdyn side of X^T rdyn = Gv(K1)^T (C rdyn); K0 = the stage's record, rd = its defect vector, dpn = dp_d of its node
BMPC_D inline double stage_t6(Wave &W, const double *K0, const double *rd, const double *dpn, int c6) {
    const int jo = c6 < 3 ? KW + c6 * 7 : KA + (c6 - 3) * 7;
    BMPC_ACC4_DECL(ta);
#pragma unroll
    for (int r = 0; r < 7; r++) { BMPC_ACC4(ta, r, K0[KD + c6 * 7 + r] * rd[r]); BMPC_ACC4(ta, r + 1, K0[jo + r] * rd[7 + r]); }
    return -W.ca * BMPC_ACC4_SUM(ta) + W.cb * dpn[c6] * rd[SDDPHI];
}

// Node cost in block form, for ONE lane = one chain pair (i, l): the lane's 4x4 block of Q~ of node k+1 (index k) is added to the block
// of the value function the lane holds IN REGISTERS (Pb, the lane's own orientation: Pb[f*4+g] = P[(f,i)][(g,l)]), the iota couplings and
// the gradient go to LDS as before.  Since round 3 the value-function blocks of the chain part never touch LDS: the congruence F^T P F
// (S1), the Schur update (S3) and this add are all lane-local; what crosses lanes -- P rdyn for the gradient recursion -- leaves as four
// partial products per lane (PP), which S0 sums over the eight pairs of a chain.
// Inputs of the call: C = the block the Schur phase of stage k+1 just produced (canonical orientation, i.e. of the pair (min, max)), or
// zeros at the last stage; ci3 / pii / pvv = the Schur phase's iota-coupling entries and gradient entry of this lane (or zeros).
// Predicated: every lane evaluates the joint-pair block AND the joint/phi coupling on clamped chain indices (all loads up front), the
// pair kind only selects what is added where.  The stage's data (records oK0 / oKV1, staging area, NC, KHP, L_MU, RD) must be in LDS.
// -- first half: everything that depends on the iterate and the multipliers only (NOT on the recursion): the entries this lane adds to its
//    block (add[16], the planes its pair kind touches), to its iota couplings (c3inc) and to P_ii (piinc), and the predicted-point curvature
//    wpv of its joint pair (for q~).  Inputs as pointers: the one-wave program passes its LDS staging areas, the helper wave of a team the
//    LDS-resident workspace rows of the stage (same layouts).
struct BlkIn { const double *K0, *KV1, *KHV /* per-joint curvature vectors of the stage (KHV_*) */, *NC, *mu4 /* curvature multipliers mu_p 3 | mu_v 3 | mu_w 3 | mu_w of the next node's velocity point 3 */,
               *dpd /* dp_d of the stage's node (6) */, *sgk /* sigma = nu / t rows of the node (57) */; };
BMPC_D inline void blk_prep_lane(Wave &W, const POff &po, int k, double delta, int lane, const BlkIn &in, double (&add)[16], double (&c3inc)[3], double &piinc,
                                 double (&wpv)[2][2]) {
    const int N = W.N; const double h = W.h; const int ex = W.o.exact_hessian;
    double *L = W.L;
    const double *PAR = L + L_PAR, *w = PAR + po.w;
    const double *sgk = in.sgk;
    const double *NC = in.NC, *KHV = in.KHV;
    const double *K0 = in.K0, *KV1 = in.KV1;
    const bool has_next = k < N - 1;
    const int i = lane >> 3, l = lane & 7, ci = i < l ? i : l, cl = i < l ? l : i; const bool tr = i > l;
    const bool both = cl < 7, mix = !both && ci < 7;
    const int cic = ci < 7 ? ci : 0, clc = cl < 7 ? cl : 0;
    const double *A1 = NC + NC_A1, *A2 = NC + NC_A2, cv = NC[NC_SC + 3], *d = in.dpd;
    double e[2][2], vf[2], vd[2], vdd[2];
    // Gv columns of the two chains: [D | J] columns (q part f = 0, dq part f = 1)
    double gi[2][6], gl_[2][6];
#pragma unroll
    for (int c6 = 0; c6 < 6; c6++) {
        const int jo = c6 < 3 ? KW + c6 * 7 : KA + (c6 - 3) * 7;
        gi[0][c6] = K0[KD + c6 * 7 + cic]; gi[1][c6] = K0[jo + cic];
        gl_[0][c6] = K0[KD + c6 * 7 + clc]; gl_[1][c6] = K0[jo + clc];
    }
#pragma unroll
    for (int f = 0; f < 2; f++) {
#pragma unroll
        for (int g = 0; g < 2; g++) {
            const int b = g * 7 + clc;
            double v = 0;
            if (f == 0 && g == 0) for (int c = 0; c < 3; c++) v += K0[KW + c * 7 + cic] * A1[c * 7 + clc];
#pragma unroll
            for (int c = 0; c < 3; c++) v += 0.5 * h * gi[f][3 + c] * A2[c * 14 + b];      // Ehat columns are the rotational rows 3..5 of Gv
            double gv = 0;
#pragma unroll
            for (int c6 = 0; c6 < 6; c6++) gv += gi[f][c6] * gl_[g][c6];
            v += cv * gv;
            double wp = 0, wn = 0;
            if (ex && !(f == 1 && g == 1)) {
                if (f == 0 && g == 0) { wp = kh_qq(K0, KHV, cic, clc);
                                        if (has_next) wn = kh_qq_w(KHV, cic, clc); }
                else { const int qi = f == 0 ? cic : clc, dj = f == 0 ? clc : cic;
                       wp = kh_qdq(K0, KHV, qi, dj);
                       if (has_next) wn = kh_qdq_w(KV1, KHV, qi, dj); }
            }
            wpv[f][g] = wp;
            e[f][g] = v + wp + wn;
        }
        // coupling of (q, dq) of chain ci with (phi, dphi, ddphi)
        double f1 = 0, f2 = 0, dsum = 0;
        if (f == 0) for (int c = 0; c < 3; c++) f1 += K0[KW + c * 7 + cic] * NC[NC_HPF + c];
#pragma unroll
        for (int c = 0; c < 3; c++) f2 += gi[f][3 + c] * NC[NC_HRF + c];
#pragma unroll
        for (int c6 = 0; c6 < 6; c6++) dsum += d[c6] * gi[f][c6];
        vf[f] = f1 + 0.5 * h * f2; vd[f] = -2 * w[2] * dsum; vdd[f] = -W.cb * dsum;
    }
    const double dq0 = 2 * w[10] + sgk[IQU + cic] + sgk[IQL + cic] + delta, dq1 = 2 * w[11] + sgk[IDQU + cic] + sgk[IDQL + cic] + delta,
                 dq2 = 2 * w[12] + delta, dq3 = 2 * w[13] + sgk[IJU + cic] + sgk[IJL + cic] + delta;
    const double p0 = NC[NC_SC + 0] + delta, p1 = NC[NC_SC + 1] + delta, p2 = NC[NC_SC + 2] + delta, p3 = 2 * w[9] + sgk[IJU + 7] + sgk[IJL + 7] + delta;
    // iota couplings of this lane's Schur entries: P[(f,i)][iota_a] += (h/2)(Hrr Ehat)[a][(f,i)] for (q, dq) rows of the joints, += Hr,phi for
    // the phi row; P_ii += Hrr + delta I.  (Until round 3 these were read-modify-writes of other lanes' LDS entries in a phase of their own.)
    const int lf = (lane & 31) >> 3, lii = lane & 7;
    const bool yq = lf < 2 && lii < 7, yphi = lf == 0 && lii == 7;
    const int a2i = yq ? lf * 7 + lii : 0;
    const bool onII = lane >= 32 && lane < 32 + 6; const int t = onII ? lane - 32 : 0;
    const int ib = t < 3 ? 0 : (t < 5 ? 1 : 2), ic = t < 3 ? t : (t < 5 ? t - 2 : 2);
#pragma unroll
    for (int b2 = 0; b2 < 3; b2++) c3inc[b2] = (yq ? 1.0 : 0.0) * A2[b2 * 14 + a2i] + (yphi ? 1.0 : 0.0) * NC[NC_HRF + b2];
    piinc = NC[NC_HRR + ib * 3 + ic] + (ib == ic ? delta : 0.0);
    // ---- the planes of Q~ the lane's pair kind touches (static plane indices: the block lives in registers) ----
    {
        const bool dg = both && ci == cl, c77 = !both && !mix;
        const double e00 = e[0][0] + (dg ? dq0 : 0.0), e11 = e[1][1] + (dg ? dq1 : 0.0), e01 = e[0][1], e10 = dg ? e[0][1] : e[1][0];
#pragma unroll
        for (int q = 0; q < 16; q++) add[q] = 0.0;
        add[0] = both ? e00 : (mix ? vf[0] : p0);
        add[1] = both ? (tr ? e10 : e01) : (mix ? (tr ? vf[1] : vd[0]) : 0.0);
        add[2] = (mix && !tr) ? vdd[0] : 0.0;
        add[4] = both ? (tr ? e01 : e10) : (mix ? (tr ? vd[0] : vf[1]) : 0.0);
        add[5] = both ? e11 : (mix ? vd[1] : p1);
        add[6] = (mix && !tr) ? vdd[1] : 0.0;
        add[8] = (mix && tr) ? vdd[0] : 0.0;
        add[9] = (mix && tr) ? vdd[1] : 0.0;
        add[10] = both ? (dg ? dq2 : 0.0) : (c77 ? p2 : 0.0);
        add[15] = both ? (dg ? dq3 : 0.0) : (c77 ? p3 : 0.0);
    }
}
// predicted-point curvature of the joint pairs (for q~, node_q_row in S0) into the 14 x 14 table WY (an LDS offset); all stores
// unconditional: a lane that has nothing to store for a role stores to the dummy word
BMPC_D inline void blk_store_wy(Wave &W, int lane, int oWY, const double (&wpv)[2][2]) {
    double *L = W.L;
    const int i = lane >> 3, l = lane & 7, ci = i < l ? i : l, cl = i < l ? l : i;
    const bool both = cl < 7;
    const int cic = ci < 7 ? ci : 0, clc = cl < 7 ? cl : 0;
#pragma unroll
    for (int f = 0; f < 2; f++)
#pragma unroll
        for (int g = 0; g < 2; g++) {
            const int a = f * 7 + cic, b = g * 7 + clc;
            const int o1 = both ? oWY + a * 14 + b : L_DUMMY, o2 = both ? oWY + b * 14 + a : L_DUMMY;
            L[o1] = wpv[f][g]; L[o2] = wpv[f][g];
        }
}
// -- second half: the recursion-dependent part: the lane's value-function block = Schur result (own orientation) + add, iota couplings,
//    P_ii, gradient, and the partial products of P rdyn
BMPC_D inline void blk_apply_lane(Wave &W, int lane, const double (&C)[4][4], const double (&ci3)[3], double pii, double pvv, const double (&add)[16],
                                  const double (&c3inc)[3], double piinc, double *Pb) {
    double *L = W.L;
    const int i = lane >> 3, l = lane & 7; const bool tr = i > l;
    const int lf = (lane & 31) >> 3, lii = lane & 7;
    const bool onII = lane >= 32 && lane < 32 + 6; const int t = onII ? lane - 32 : 0;
    const int ib = t < 3 ? 0 : (t < 5 ? 1 : 2), ic = t < 3 ? t : (t < 5 ? t - 2 : 2);
    double c3[3];
#pragma unroll
    for (int b2 = 0; b2 < 3; b2++) c3[b2] = ci3[b2] + c3inc[b2];
    const double piin = pii + piinc;
#pragma unroll
    for (int f = 0; f < 4; f++)
#pragma unroll
        for (int g = 0; g < 4; g++) Pb[f * 4 + g] = (tr ? C[g][f] : C[f][g]) + add[f * 4 + g];
    L[L_PCI + pci(0, lf, lii)] = c3[0]; L[L_PCI + pci(1, lf, lii)] = c3[1]; L[L_PCI + pci(2, lf, lii)] = c3[2];   // lanes >= 32 repeat lanes 0..31
    L[onII ? L_PII + ib * 3 + ic : L_DUMMY] = piin; L[onII ? L_PII + ic * 3 + ib : L_DUMMY] = piin;
    L[L_PV + (lane < NS ? lane : 0)] = pvv;
    // partial products of P rdyn over the lane's pair: PP[f][pair] = sum_{g<3} P[(f,i)][(g,l)] rdyn[(g,l)] (rdyn of the jerk states is zero)
    {
        const double r0 = L[L_RD + srow(0, l)], r1 = L[L_RD + srow(1, l)], r2 = L[L_RD + srow(2, l)];
#pragma unroll
        for (int f = 0; f < 4; f++) L[L_PP + f * 64 + lane] = Pb[f * 4 + 0] * r0 + Pb[f * 4 + 1] * r1 + Pb[f * 4 + 2] * r2;
    }
}
// the whole node-cost add of one lane from the one-wave program's staging areas (records oK0 / oKV1, ST, NC, KHP, L_MU, RD in LDS)
BMPC_D inline void blk_add_lane(Wave &W, const POff &po, int k, double delta, int lane, int oK0, int oKV1, const double (&C)[4][4], const double (&ci3)[3],
                                double pii, double pvv, double *Pb) {
    double *L = W.L;
    BlkIn in; in.K0 = L + oK0; in.KV1 = L + oKV1; in.KHV = L + L_KHP; in.NC = L + L_NC; in.mu4 = L + L_MU + 4; in.dpd = L + L_ST + ST_REF + RDP; in.sgk = L + L_ST + ST_SG;
    double add[16], c3inc[3], piinc, wpv[2][2];
    blk_prep_lane(W, po, k, delta, lane, in, add, c3inc, piinc, wpv);
    blk_store_wy(W, lane, L_WY, wpv);
    blk_apply_lane(W, lane, C, ci3, pii, pvv, add, c3inc, piinc, Pb);
}

// Node-cost data of ALL Riccati stages in wide passes, once per iterate and BEFORE the backward sweep (it replaces wave_prepare_rlv and
// the node-cost phases 1 and 2 of rounds 1-2, which ran once per stage inside the sequential sweep):
//   * lifted residuals r_pos (3), r_v (6) of every node, r = g_lifted - G g_y (needed across neighbouring nodes) -> RLV,
//   * the defect vectors rdyn (35: the residual row the row table names; iota rows g_iw - (h/2) Ehat g_y) -> RDY,
//   * the iota couplings AE = (h/2)(Ehat(K1) + Ehat(KV_k)) (3 x 14) -> AES,
//   * the small Hessian blocks over (pos, iw, phi): Hpp, Hrr, Hp,phi, Hr,phi, H phi,phi and the scalar curvatures,
//     A1 = Hpp Jp, A2 = (h/2) Hrr Ehat, the curvature multipliers, dp_d and the non-trivial entries of gl - g^ -> NCS (row layout: NCS_*).
// All of it depends on the iterate and the multipliers only, not on the recursion.  Inside the sweep this work ran as predicated
// roles (every lane executes every role: about half the lanes idle) in chains of dependent LDS round trips: 4.6 k cycles per stage.
// Here one lane owns one (stage, entry) item, the items of all stages are independent and every lane has one.
// What costs in a wide pass is the number of DEPENDENT round trips to the workspace (~1.7 k cycles each, measured; a load that rides
// in a batch costs ~25): so each phase is written as batches -- all loads of all the item kinds of a batch first, then the
// arithmetic and the stores -- two batches in the first phase (inputs written by earlier phases), two in the second (which reads what
// the first wrote: a phase boundary).  One batch covers 10 stages; longer horizons loop.
// The results reach LDS with the other inputs of a stage through the register prefetch of the sweeps.
// The acceleration cross block XT = C^T Gv(K1) (15x14, rank 6) is never formed: its consumers contract the two rank-6 factors on
// the fly (t6 in S0, chain-pair entries in S1).
BMPC_D inline void wave_stage_data_wide(Wave &W, const POff &po, const Scr &sc) {
    const int N = W.N; const double h = W.h; const int ex = W.o.exact_hessian;
    double *L = W.L; const GPtr G = W.G; const LPtr WL = BMPC_WL(W);
    const double *PAR = L + L_PAR, *w = PAR + po.w;
    const int npass = (N + 9) / 10;
    WIDE_BEGIN
        for (int pass = 0; pass < npass; pass++) {
            // ================= batch 1: lifted residuals + iota rows (R), curvature multipliers (M), chain rows of rdyn (Y), AE (E) ==========
            constexpr int RR = cdiv_(2, NW), RM = cdiv_(2, NW), RY = cdiv_(5, NW), RE = cdiv_(7, NW);      // items in flight per lane: one batch of WS lanes covers ten stages
            double ra1[RR][7], ra2[RR][7], rg1[RR][7], rg2[RR][7], rb0[RR];
            double ml[RM][5];
            double yv[RY];
            double e1[RE], e2[RE];
#pragma unroll
            for (int u = 0; u < RR; u++) {   // R: a residual minus two 7-term dot products of a record row with g_q, g_dq; the row kind selects bases
                const int id0 = pass * WS * RR + wl + WS * u, id = id0 < N * 12 ? id0 : N * 12 - 1, k = id / 12, c = id - 12 * k;
                const int c6 = c >= 3 ? (c < 9 ? c - 3 : c - 6) : 0;                       // velocity rows 0..5; iota rows use the rotational rows 3..5
                const int p1 = c < 3 ? KW + c * 7 : KD + c6 * 7;
                const int p2 = c < 3 ? KA : (c < 9 ? (c6 < 3 ? KW + c6 * 7 : KA + (c6 - 3) * 7) : KA + (c - 9) * 7);
                const int bs = c < 3 ? GPOS + c : (c < 9 ? GV + c - 3 : GIW + c - 9);
                const LPtr kp = WL + sc.KIN + k * KREC, gk = WL + sc.G + k * NE;
                rb0[u] = gk[bs];
#pragma unroll
                for (int i = 0; i < 7; i++) { ra1[u][i] = kp[p1 + i]; ra2[u][i] = kp[p2 + i]; rg1[u][i] = gk[GQ + i]; rg2[u][i] = gk[GDQ + i]; }
            }
#pragma unroll
            for (int u = 0; u < RM; u++) {   // M: mu_p, mu_v, mu_w of the node and mu_w of the next node's velocity point (item = 3 g + c)
                const int id0 = pass * WS * RM + wl + WS * u, id = id0 < N * 12 ? id0 : N * 12 - 1, k = id / 12, ln = id - 12 * k, c = ln % 3;
                const int kn = k < N - 1 ? k + 1 : k;
                const LPtr lam = WL + sc.LAM + k * NE;
                ml[u][0] = lam[GPOS + c]; ml[u][1] = lam[GV + c]; ml[u][2] = lam[GW + c]; ml[u][3] = lam[GIW + c]; ml[u][4] = WL[sc.LAM + kn * NE + GIW + c];
            }
#pragma unroll
            for (int u = 0; u < RY; u++) {   // Y: chain rows of rdyn = the residual row the row table names
                const int id0 = pass * WS * RY + wl + WS * u, id = id0 < N * 32 ? id0 : N * 32 - 1, k = id >> 5, r = id & 31;
                yv[u] = WL[sc.G + k * NE + (((int)L[L_ZMAP + r] >> 8) & 255)];
            }
#pragma unroll
            for (int u = 0; u < RE; u++) {   // E: Ehat entries of the predicted point k-1 and of the velocity point of node k
                const int id0 = pass * WS * RE + wl + WS * u, id = id0 < N * 42 ? id0 : N * 42 - 1, k = id / 42, ln = id - 42 * k, a = ln / 14, y = ln - 14 * a;
                const int eb = y < 7 ? KD + (3 + a) * 7 + y : KA + a * 7 + y - 7, kp = k >= 1 ? k - 1 : 0;
                e1[u] = WL[sc.KIN + kp * KREC + eb]; e2[u] = WL[sc.KIN + (N + k) * KREC + eb];
            }
            // ---- arithmetic and stores of batch 1 (a clamped duplicate rewrites the last item with the same value) ----
#pragma unroll
            for (int u = 0; u < RR; u++) {
                const int id0 = pass * WS * RR + wl + WS * u, id = id0 < N * 12 ? id0 : N * 12 - 1, k = id / 12, c = id - 12 * k;
                BMPC_ACC4_DECL(sa); BMPC_ACC4_DECL(sb);
#pragma unroll
                for (int i = 0; i < 7; i++) { BMPC_ACC4(sa, i, ra1[u][i] * rg1[u][i]); BMPC_ACC4(sb, i, ra2[u][i] * rg2[u][i]); }
                const double s1 = BMPC_ACC4_SUM(sa), s2 = BMPC_ACC4_SUM(sb);
                const double m2 = c < 3 ? 0.0 : 1.0, f = c < 9 ? 1.0 : 0.5 * h;
                WL[c < 9 ? sc.RLV + k * 12 + c : sc.RDY + k * 36 + SIOTA + (c - 9)] = rb0[u] - f * (s1 + m2 * s2);
            }
#pragma unroll
            for (int u = 0; u < RM; u++) {
                const int id0 = pass * WS * RM + wl + WS * u, id = id0 < N * 12 ? id0 : N * 12 - 1, k = id / 12, ln = id - 12 * k, g = ln / 3;
                // 0/1 factors instead of selects between loaded values
                const double m0 = g == 0 ? 1.0 : 0.0, m1 = g == 1 ? 1.0 : 0.0, m2 = g == 2 ? 1.0 : 0.0, m3 = (g == 3 && k < N - 1) ? 1.0 : 0.0;
                WL[sc.NCS + k * NCS_STRIDE + NCS_MU + ln] = m0 * ml[u][0] + m1 * ml[u][1] + m2 * (ml[u][2] + 0.5 * h * ml[u][3]) + m3 * (0.5 * h * ml[u][4]);
            }
#pragma unroll
            for (int u = 0; u < RY; u++) {
                const int id0 = pass * WS * RY + wl + WS * u, id = id0 < N * 32 ? id0 : N * 32 - 1, k = id >> 5, r = id & 31;
                const bool zero = (((int)L[L_ZMAP + r] >> 16) & 1) != 0;                    // jerk states carry no defect
                WL[sc.RDY + k * 36 + r] = zero ? 0.0 : yv[u];
            }
#pragma unroll
            for (int u = 0; u < RE; u++) {
                const int id0 = pass * WS * RE + wl + WS * u, id = id0 < N * 42 ? id0 : N * 42 - 1;
                const double v = 0.5 * h * (e1[u] + e2[u]);
                WL[sc.AES + id] = id >= 42 ? v : 0.0;                                          // stage 0 has no iota coupling
            }
        }
        for (int pass = 0; pass < npass; pass++) {
            // ================= batch 2: Hpp, Hrr (C, 9 entries per stage); Hp,phi, Hr,phi, H phi,phi, scalar curvatures, dp_d (D, 3 items per stage) =====
            constexpr int RC = cdiv_(2, NW);
            double h0[RC], h1[RC], ss[RC][5], ga[RC][5], gb[RC][5];
#pragma unroll
            for (int u = 0; u < RC; u++) {
                const int id0 = pass * WS * RC + wl + WS * u, id = id0 < N * 9 ? id0 : N * 9 - 1, k = id / 9, ln = id - 9 * k, a = ln / 3, b = ln - 3 * a;
                const LPtr rr = WL + sc.REF + k * RREC, sgk = WL + sc.SG + k * NI;
                h0[u] = rr[RHPPG + ln]; h1[u] = rr[RHRRG + ln];
#pragma unroll
                for (int m = 0; m < 5; m++) { ss[u][m] = sgk[ITUBE + 2 * m] + sgk[ITUBE + 2 * m + 1]; ga[u][m] = rr[RGC + m * 4 + a]; gb[u][m] = rr[RGC + m * 4 + b]; }
            }
            const int idd0 = pass * WS + wl, idd = idd0 < N * 3 ? idd0 : N * 3 - 1, kd = idd / 3, ad = idd - 3 * kd;
            double su[5], sl[5], g3[5], w1[5], gd[5], nu_u[5], nu_l[5], c2[5], w2[5];
            const LPtr rrd = WL + sc.REF + kd * RREC, sgd = WL + sc.SG + kd * NI, nud = WL + sc.NUm + kd * NI;
            const double hp0 = rrd[RHPFG + ad], hr0 = rrd[RHRFG + ad], dpdp = rrd[RDPDP], hffg = rrd[RHFFG];
            const double s_phi0 = sgd[IPHI0], s_phimax = sgd[IPHIMAX], s_dphimax = sgd[IDPHIMAX];
            const double dp_a = rrd[RDP + ad], dp_b = rrd[RDP + 3 + ad];
#pragma unroll
            for (int m = 0; m < 5; m++) {
                su[m] = sgd[ITUBE + 2 * m]; sl[m] = sgd[ITUBE + 2 * m + 1]; g3[m] = rrd[RGC + m * 4 + 3]; w1[m] = rrd[RW1 + m]; gd[m] = rrd[RGC + m * 4 + ad];
                nu_u[m] = nud[ITUBE + 2 * m]; nu_l[m] = nud[ITUBE + 2 * m + 1]; c2[m] = rrd[RC2 + m]; w2[m] = rrd[RW2 + m];
            }
            // ---- arithmetic and stores of batch 2 ----
#pragma unroll
            for (int u = 0; u < RC; u++) {
                const int id0 = pass * WS * RC + wl + WS * u, id = id0 < N * 9 ? id0 : N * 9 - 1, k = id / 9, ln = id - 9 * k;
                double hp = h0[u], hr = h1[u];
#pragma unroll
                for (int m = 0; m < 5; m++) {
                    const double gg = ss[u][m] * ga[u][m] * gb[u][m];
                    if (m == 1 || m == 2) hp += gg; else hr += gg;
                }
                WL[sc.NCS + k * NCS_STRIDE + NC_HPP + ln] = hp; WL[sc.NCS + k * NCS_STRIDE + NC_HRR + ln] = hr;
            }
            {
                double hp = hp0, hr = hr0;
                const double exm = ex ? 1.0 : 0.0;
                double hff = hffg + 2 * w[6] + s_phi0 + s_phimax;
#pragma unroll
                for (int m = 0; m < 5; m++) {
                    const double gpu_ = g3[m] - w1[m], gpl_ = -g3[m] - w1[m];
                    const double gg = su[m] * gd[m] * gpu_ - sl[m] * gd[m] * gpl_;
                    if (m == 1 || m == 2) hp += gg; else hr += gg;
                    hff += su[m] * gpu_ * gpu_ + sl[m] * gpl_ * gpl_;
                    hff += exm * (nu_u[m] * (c2[m] - w2[m]) + nu_l[m] * (-c2[m] - w2[m]));
                }
                const LPtr row = WL + sc.NCS + kd * NCS_STRIDE;
                row[NC_HPF + ad] = hp; row[NC_HRF + ad] = hr;
                // the four scalars: every item of the stage has them, item a writes scalar a; the fourth, the zero word and dp_d ride along
                const double sc1 = 2 * w[2] * dpdp + 2 * w[7] + s_dphimax, sc2 = 2 * w[5] * dpdp + 2 * w[8];
                row[NC_SC + ad] = ad == 0 ? hff : (ad == 1 ? sc1 : sc2);
                row[NC_SC + 3] = 2 * w[2] + W.ca * (kd < N - 1 ? 2.0 : 1.0);      // identical in the three items of a stage
                row[NCS_ZERO] = 0.0;
                row[NCS_RDP + ad] = dp_a; row[NCS_RDP + 3 + ad] = dp_b;
            }
        }
    WIDE_END
    // ---- second phase: what needs the small blocks and the lifted residuals of the first ----
    WIDE_BEGIN
        for (int pass = 0; pass < npass; pass++) {
            // ================= batch 3: A1 = Hpp Jp (21), A2 = (h/2) Hrr Ehat (42): one 3-term product per entry =================
            constexpr int RA = cdiv_(10, NW);
            double cf[RA][3], kc[RA][3];
#pragma unroll
            for (int u = 0; u < RA; u++) {
                const int id0 = pass * WS * RA + wl + WS * u, id = id0 < N * 63 ? id0 : N * 63 - 1, k = id / 63, e = id - 63 * k;
                const bool isA1 = e < 21; const int e2 = isA1 ? 0 : e - 21;
                const int c = isA1 ? e / 7 : e2 / 14, i = isA1 ? e - 7 * c : 0, y = isA1 ? 0 : e2 - 14 * c;
                const int cb = isA1 ? NC_HPP + c * 3 : NC_HRR + c * 3, kb = isA1 ? KW + i : (y < 7 ? KD + 21 + y : KA + y - 7);
                const LPtr row = WL + sc.NCS + k * NCS_STRIDE, K0 = WL + sc.KIN + k * KREC;
#pragma unroll
                for (int b2 = 0; b2 < 3; b2++) { cf[u][b2] = row[cb + b2]; kc[u][b2] = K0[kb + b2 * 7]; }
            }
#pragma unroll
            for (int u = 0; u < RA; u++) {
                const int id0 = pass * WS * RA + wl + WS * u, id = id0 < N * 63 ? id0 : N * 63 - 1, k = id / 63, e = id - 63 * k;
                double sacc = 0;
#pragma unroll
                for (int b2 = 0; b2 < 3; b2++) sacc += cf[u][b2] * kc[u][b2];
                WL[sc.NCS + k * NCS_STRIDE + NC_A1 + e] = e < 21 ? sacc : 0.5 * h * sacc;
            }
        }
        for (int pass = 0; pass < npass; pass++) {
            // ================= batch 5: per-joint vectors of the kinematic curvature (items (stage, joint); KHV_* row layout) =================
            // needs the curvature multipliers of batch M (first phase) and the prefix vectors kin_point left in KHPG
            constexpr int RJ_ = cdiv_(2, NW);
            double ja[RJ_][3], jw[RJ_][3], jW[RJ_][3], jV[RJ_][3], jG[RJ_][3], ja1[RJ_][3], jG1[RJ_][3], jmu[RJ_][12];
#pragma unroll
            for (int u = 0; u < RJ_; u++) {
                const int id0 = pass * WS * RJ_ + wl + WS * u, id = id0 < N * 7 ? id0 : N * 7 - 1, k = id / 7, j = id - 7 * k, kn = k < N - 1 ? k + 1 : k;
                const LPtr rec = WL + sc.KIN + k * KREC, rec1 = WL + sc.KIN + (N + kn) * KREC, row = WL + sc.NCS + k * NCS_STRIDE;
                const GPtr hp = G + sc.KHPG + k * 72, hp1 = G + sc.KHPG + (N + kn) * 72;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    ja[u][c] = rec[KA + c * 7 + j]; jw[u][c] = rec[KW + c * 7 + j]; jW[u][c] = hp[3 * j + c]; jV[u][c] = hp[24 + 3 * j + c]; jG[u][c] = hp[45 + 3 * j + c];
                    ja1[u][c] = rec1[KA + c * 7 + j]; jG1[u][c] = hp1[45 + 3 * j + c];
                }
#pragma unroll
                for (int m = 0; m < 12; m++) jmu[u][m] = row[NCS_MU + m];
            }
#pragma unroll
            for (int u = 0; u < RJ_; u++) {
                const int id0 = pass * WS * RJ_ + wl + WS * u, id = id0 < N * 7 ? id0 : N * 7 - 1, k = id / 7, j = id - 7 * k;
                const double *mu_p = jmu[u], *mu_v = jmu[u] + 3, *mu_w = jmu[u] + 6, *mu_w1 = jmu[u] + 9;
                double m_[3], n_[3], o_[3], c_[3], p_[3], z_[3], s_[3], u_[3], g_[3], g1_[3], o1_[3];
                cross3(mu_p, ja[u], m_); cross3(mu_v, ja[u], n_); cross3(mu_w, ja[u], o_); cross3(mu_v, jW[u], c_); cross3(c_, ja[u], p_); cross3(n_, jW[u], z_);
                cross3(ja[u], jV[u], s_); cross3(jW[u], jw[u], u_); cross3(ja[u], jG[u], g_); cross3(ja1[u], jG1[u], g1_); cross3(mu_w1, ja1[u], o1_);
                const GPtr kv = G + sc.KHV + k * KHV_STRIDE;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    kv[KHV_X + c * 7 + j] = (m_[c] + p_[c]) - z_[c]; kv[KHV_N + c * 7 + j] = n_[c]; kv[KHV_O + c * 7 + j] = o_[c];
                    kv[KHV_Y + c * 7 + j] = s_[c] + u_[c]; kv[KHV_G + c * 7 + j] = g_[c]; kv[KHV_G1 + c * 7 + j] = g1_[c]; kv[KHV_O1 + c * 7 + j] = o1_[c];
                }
            }
        }
        for (int pass = 0; pass < npass; pass++) {
            // ================= batch 4: the 12 rows of gl = g^ + H r + cross terms that differ from g^ (pos 3, v 6, phi, dphi, ddphi) =================
            constexpr int RV = cdiv_(2, NW);
            double nc3[RV][3], rl3[RV][3], rv0[RV], rvm[RV], rvp[RV], cvv[RV], dd[RV][6], r6[RV][6], m6[RV][6];
#pragma unroll
            for (int u = 0; u < RV; u++) {
                const int id0 = pass * WS * RV + wl + WS * u, id = id0 < N * 12 ? id0 : N * 12 - 1, k = id / 12, t = id - 12 * k;
                const bool isPos = t < 3, isV = t >= 3 && t < 9;
                const int c = isV ? t - 3 : 0, pa = isPos ? NC_HPP + t * 3 : NC_HPF;            // 3-vector that multiplies r_pos
                const int kp = k >= 1 ? k - 1 : 0, kn = k < N - 1 ? k + 1 : k;
                const LPtr row = WL + sc.NCS + k * NCS_STRIDE, rl = WL + sc.RLV + k * 12, rm = WL + sc.RLV + kp * 12, rp = WL + sc.RLV + kn * 12;
#pragma unroll
                for (int b2 = 0; b2 < 3; b2++) { nc3[u][b2] = row[pa + b2]; rl3[u][b2] = rl[b2]; }
                rv0[u] = rl[3 + c]; rvm[u] = rm[3 + c]; rvp[u] = rp[3 + c]; cvv[u] = row[NC_SC + 3];
#pragma unroll
                for (int c6 = 0; c6 < 6; c6++) { dd[u][c6] = row[NCS_RDP + c6]; r6[u][c6] = rl[3 + c6]; m6[u][c6] = rm[3 + c6]; }
            }
#pragma unroll
            for (int u = 0; u < RV; u++) {
                const int id0 = pass * WS * RV + wl + WS * u, id = id0 < N * 12 ? id0 : N * 12 - 1, k = id / 12, t = id - 12 * k;
                const bool isPos = t < 3, isV = t >= 3 && t < 9, isPhi = t == 9, isD = t == 10, isDD = t == 11;
                double sA = 0, s1 = 0, s2 = 0;
#pragma unroll
                for (int b2 = 0; b2 < 3; b2++) sA += nc3[u][b2] * rl3[u][b2];
#pragma unroll
                for (int c6 = 0; c6 < 6; c6++) { s1 += dd[u][c6] * r6[u][c6]; s2 += dd[u][c6] * m6[u][c6]; }
                const double vm = k >= 1 ? rvm[u] : 0.0, vp = k < N - 1 ? rvp[u] : 0.0;
                const double tV = cvv[u] * rv0[u] - W.ca * vm - W.ca * vp, tD = -2 * w[2] * s1, tDD = -W.cb * s1 + (k >= 1 ? W.cb * s2 : 0.0);
                double addv = 0.0;
                addv = isDD ? tDD : addv; addv = isD ? tD : addv; addv = isV ? tV : addv; addv = (isPos || isPhi) ? sA : addv;
                WL[sc.NCS + k * NCS_STRIDE + NCS_ADDV + t] = addv;
            }
        }
    WIDE_END
}

// Gv[c6][y] of a kinematics record: d(v)/d(q,dq) = [D | J]
BMPC_D inline double gv_at(const double *rec, int c6, int y) {
    return y < 7 ? rec[KD + c6 * 7 + y] : (c6 < 3 ? rec[KW + c6 * 7 + y - 7] : rec[KA + (c6 - 3) * 7 + y - 7]);
}

// Stage inputs of the Riccati sweep: global -> registers (loads, issued a full stage ahead) -> LDS (commit).  Both are
// lane-level pieces that ride at the end of the previous stage's last phase (the staging area and the record buffers a stage
// reads are dead after its S1 phase), so they cost no phase of their own.
// Branch-free: every lane loads from a clamped, always-valid index (lanes beyond the end of an array repeat its last element;
// a neighbour node that does not exist is replaced by the nearest one -- its data is masked by the consumers), and the commit
// stores to the same clamped slots (identical values), so neither has a single exec-mask branch.
BMPC_D inline void backward_loads_lane(Wave &W, const Scr &sc, int k, double *pf, int lane, bool full) {
    const int N = W.N; const GPtr G = W.G; const LPtr WL = BMPC_WL(W);
    const int kn = k < N - 1 ? k + 1 : k, kp = k >= 1 ? k - 1 : 0;
    const int l2 = lane < KREC - 64 ? 64 + lane : KREC - 1;
    const int lz = lane < NZ ? lane : NZ - 1, li = lane < NI ? lane : NI - 1, le = lane < NE ? lane : NE - 1;
    const int l35 = lane < NS ? lane : NS - 1, l42 = lane < 42 ? lane : 41;
    // of the four kinematics records of a stage (node k, velocity point of node k+1, node k-1, velocity point of node k) the
    // first two are the last two of the previous stage (k+1): they stay in LDS, only the first stage of a sweep loads all four
    // (teams, BMPC_NW > 1: what only the node-cost add reads -- the velocity-point record of the next node, the small Hessian blocks, the
    // barrier ratios, the curvature prefix vectors -- is the helper wave's business (team_blk_prep reads it from the LDS-resident rows): the
    // sweep's wave neither loads nor stages it)
    if (full) {
        pf[0] = WL[sc.KIN + k * KREC + lane]; pf[1] = WL[sc.KIN + k * KREC + l2];
#if BMPC_NW == 1
        pf[2] = WL[sc.KIN + (N + kn) * KREC + lane]; pf[3] = WL[sc.KIN + (N + kn) * KREC + l2];
#endif
    }
    pf[4] = WL[sc.KIN + kp * KREC + lane]; pf[5] = WL[sc.KIN + kp * KREC + l2];
#if BMPC_NW == 1
    pf[6] = WL[sc.KIN + (N + k) * KREC + lane]; pf[7] = WL[sc.KIN + (N + k) * KREC + l2];      // (velocity point of node k: next stage's KV1, read by the node-cost add only)
#endif
    // node-cost data of the stage (wave_stage_data_wide): NCS row (two slots), defects, iota couplings; gl = g^ + its non-trivial entries
#if BMPC_NW == 1
    pf[8] = WL[sc.NCS + k * NCS_STRIDE + lane];
#endif
    pf[9] = WL[sc.NCS + k * NCS_STRIDE + 64 + lane];
    pf[10] = WL[sc.RDY + k * 36 + l35]; pf[11] = WL[sc.GH + k * NZ + lz];
    {   // rows pos (29..31), v (35..40), phi, dphi, ddphi (41..43) of Z have a non-trivial entry, the others add the zero word
        const int t = lz >= ZV ? lz - ZV + 3 : lz - ZPOS; const bool sp = lz >= ZV || (lz >= ZPOS && lz < ZIW);
        pf[13] = WL[sc.NCS + k * NCS_STRIDE + (sp ? NCS_ADDV + t : NCS_ZERO)];
    }
#if BMPC_NW == 1
    pf[14] = WL[sc.G + k * NE + le];
    pf[12] = WL[sc.SG + k * NI + li];
    // per-joint curvature vectors of the stage (147 doubles in three slots)
    pf[15] = G[sc.KHV + k * KHV_STRIDE + lane]; pf[16] = G[sc.KHV + k * KHV_STRIDE + 64 + lane]; pf[17] = G[sc.KHV + k * KHV_STRIDE + 128 + (lane < 24 ? lane : 23)];
#endif
    pf[20] = WL[sc.AES + k * 42 + l42];
}
// record buffers of stage k: (K0, K1) and (KV1, KV) swap roles from stage to stage
BMPC_D inline void backward_buffers(int N, int k, int &oK0, int &oK1, int &oKV, int &oKV1) {
    const bool odd = ((N - 1 - k) & 1) != 0;
    oK0 = odd ? L_K1 : L_K0; oK1 = odd ? L_K0 : L_K1; oKV1 = odd ? L_KV : L_KV1; oKV = odd ? L_KV1 : L_KV;
}
BMPC_D inline void backward_commit_lane(Wave &W, int k, const double *pf, int lane, bool first) {
    double *L = W.L;
    int oK0, oK1, oKV, oKV1; backward_buffers(W.N, k, oK0, oK1, oKV, oKV1);
    const int l2 = lane < KREC - 64 ? 64 + lane : KREC - 1;
    const int lz = lane < NZ ? lane : NZ - 1, li = lane < NI ? lane : NI - 1, le = lane < NE ? lane : NE - 1;
    const int l35 = lane < NS ? lane : NS - 1, l42 = lane < 42 ? lane : 41;
#if BMPC_NW == 1
    if (first) { L[oK0 + lane] = pf[0]; L[oKV1 + lane] = pf[2]; L[oK0 + l2] = pf[1]; L[oKV1 + l2] = pf[3]; }
#else
    if (first) { L[oK0 + lane] = pf[0]; L[oK0 + l2] = pf[1]; }
#endif
    L[oK1 + lane] = pf[4]; L[oK1 + l2] = pf[5];
#if BMPC_NW == 1
    L[oKV + lane] = pf[6]; L[oKV + l2] = pf[7];
#endif
#if BMPC_NW == 1
    L[L_NC + lane] = pf[8];
#endif
    {   // second slot of the NCS row: the rest of the L_NC mirror, the curvature multipliers, dp_d (flat chain of selects on the address)
        const int idx = 64 + lane;
        int dst = L_DUMMY;
        dst = idx < NCS_RDP + 6 ? L_ST + ST_REF + RDP + (idx - NCS_RDP) : dst;
#if BMPC_NW > 1 && defined(BMPC_WSG)
        dst = idx < NCS_RDP ? L_DUMMY : dst;      // (pairs: L_NC[0..91) and the curvature multipliers belong to the helper wave's stage, helper_commit_lane)
#else
        dst = idx < NCS_RDP ? L_MU + 4 + (idx - NCS_MU) : dst;
        dst = idx < NCS_MU ? L_NC + idx : dst;
#endif
        L[dst] = pf[9];
    }
    L[L_RD + l35] = pf[10];
    L[L_NC + NC_GL + lz] = pf[11] + pf[13];
#if BMPC_NW == 1
    L[L_ST + ST_G + le] = pf[14];
    L[L_ST + ST_SG + li] = pf[12];
    L[L_KHP + lane] = pf[15]; L[L_KHP + 64 + lane] = pf[16]; L[L_KHP + 128 + (lane < 24 ? lane : 23)] = pf[17];
#endif
    L[L_AE + l42] = pf[20];
}

// ----------------------------------------------------------------------------------------
// Riccati backward sweep, block form.  Returns false (wave-uniform) if a stage's 8x8 jerk block is not positive definite.
// ----------------------------------------------------------------------------------------
#if BMPC_NW > 1 && defined(BMPC_WSG)
// Helper wave of a PAIR's Riccati sweep.  The workspace is in the global slab, so the helper has the sweep's own discipline: the inputs of
// stage j are loaded into registers a stage ahead (helper_loads_lane) and dropped into LDS in one burst (helper_commit_lane) -- into the areas
// the sweep's wave leaves idle (layout note at L_PREP).  Then the recursion-independent half of the node-cost add (blk_prep_lane from LDS,
// exactly the one-wave program's operands), the curvature table, the q~ rows and t6 of the stage.
BMPC_D inline void helper_loads_lane(Wave &W, const Scr &sc, int j0, double *pf, int lane) {
    const int N = W.N; const GPtr G = W.G;
    const int j = j0 >= 0 ? j0 : 0, jn = j < N - 1 ? j + 1 : j;
    const int lz = lane < NZ ? lane : NZ - 1, li = lane < NI ? lane : NI - 1, le = lane < NE ? lane : NE - 1, l36 = lane < 36 ? lane : 35;
    pf[0] = G[sc.KIN + (N + jn) * KREC + (lane < 24 ? lane : 23)];      // axes of the velocity point of the next node (kh_qdq_w reads nothing else of that record)
    pf[1] = G[sc.NCS + j * NCS_STRIDE + lane]; pf[2] = G[sc.NCS + j * NCS_STRIDE + 64 + lane];
    pf[3] = G[sc.SG + j * NI + li]; pf[4] = G[sc.G + j * NE + le]; pf[5] = G[sc.GH + j * NZ + lz];
    {   // gl = g^ + its non-trivial entries (backward_commit_lane forms the same sum for the sweep's wave)
        const int t = lz >= ZV ? lz - ZV + 3 : lz - ZPOS; const bool sp = lz >= ZV || (lz >= ZPOS && lz < ZIW);
        pf[6] = G[sc.NCS + j * NCS_STRIDE + (sp ? NCS_ADDV + t : NCS_ZERO)];
    }
    pf[7] = G[sc.KHV + j * KHV_STRIDE + lane]; pf[8] = G[sc.KHV + j * KHV_STRIDE + 64 + lane]; pf[9] = G[sc.KHV + j * KHV_STRIDE + 128 + (lane < 24 ? lane : 23)];
    pf[10] = G[sc.RDY + j * 36 + l36];
}
BMPC_D inline void helper_commit_lane(Wave &W, const double *pf, int lane) {
    double *L = W.L;
    const int lz = lane < NZ ? lane : NZ - 1, li = lane < NI ? lane : NI - 1, le = lane < NE ? lane : NE - 1, l36 = lane < 36 ? lane : 35;
    L[L_HKV + (lane < 24 ? lane : 23)] = pf[0];
    L[L_NC + lane] = pf[1];
    {   // second slot of the NCS row: the rest of the small blocks / A2 (-> L_NC), dp_d (-> the helper's own six words); the rest is not read here
        const int idx = 64 + lane;
        int dst = L_DUMMY;
        dst = (idx >= NCS_RDP && idx < NCS_RDP + 6) ? L_HDP + (idx - NCS_RDP) : dst;
        dst = idx < NCS_MU ? L_NC + idx : dst;
        L[dst] = pf[2];
    }
    L[L_ST + ST_SG + li] = pf[3]; L[L_ST + ST_G + le] = pf[4]; L[L_HGL + lz] = pf[5] + pf[6];
    L[L_HKHP + lane] = pf[7]; L[L_HKHP + 64 + lane] = pf[8]; L[L_HKHP + 128 + (lane < 24 ? lane : 23)] = pf[9];
    L[L_HRD + l36] = pf[10];
}
// prep of stage j (pf holds its inputs).  sync2: the second barrier of a stage -- the sweep's wave has read L_PREP of the previous hand-over and
// finished with the Schur result that overlays it -- sits between the commit and the first store to L_PREP.
BMPC_D inline void team_blk_prep(Wave &W, const POff &po, const Scr &sc, int j, double delta, LaneRegs *LR, bool sync2) {
    const int N = W.N;
    double *L = W.L;
    const double *K0 = L + (((N - 1 - j) & 1) ? L_K1 : L_K0);      // record of stage j: the sweep's wave committed it as oK1 of stage j + 1 (oK0 of stage N - 1)
    LANES_BEGIN
        helper_commit_lane(W, LR[LIDXH].pf, lane);
        helper_loads_lane(W, sc, j - 1, LR[LIDXH].pf, lane);
    LANES_END
    if (sync2) { TEAM_SYNC_LDS(); }
    LANES_BEGIN
        BlkIn in; in.K0 = K0; in.KV1 = L + L_HKV; in.KHV = L + L_HKHP; in.NC = L + L_NC; in.mu4 = nullptr; in.dpd = L + L_HDP; in.sgk = L + L_ST + ST_SG;
        double add[16], c3inc[3], piinc, wpv[2][2];
        blk_prep_lane(W, po, j, delta, lane, in, add, c3inc, piinc, wpv);
        blk_store_wy(W, lane, L_WY, wpv);
        double *o = L + L_PREP + lane;
        o[0] = add[0]; o[64] = add[1]; o[128] = add[2]; o[192] = add[4]; o[256] = add[5]; o[320] = add[6]; o[384] = add[8]; o[448] = add[9];
        o[512] = add[10]; o[576] = add[15];
        {   // the iota increments depend on lane & 31 only (lanes >= 32 repeat 0..31: identical values to the same words), P_ii's on six lanes
            double *c = L + L_PREP + PREP_C3 + (lane & 31);
            c[0] = c3inc[0]; c[32] = c3inc[1]; c[64] = c3inc[2];
            const bool onII = lane >= 32 && lane < 32 + 6;
            L[onII ? L_PREP + PREP_PII + (lane - 32) : L_DUMMY] = piinc;
        }
    LANES_END
    LANES_BEGIN      // q~ rows (32 chain rows) and t6 of the stage (they need the curvature table this wave just wrote)
        {
            const int r = lane < 32 ? lane : 0;
            const double qr = node_q_row_p(L, L + L_HGL, L + L_WY, L + L_ST + ST_G, K0, r, W.h, W.o.exact_hessian);
            L[lane < 32 ? L_QRB + (j & 1) * 40 + r : L_DUMMY] = qr;
        }
        {
            const bool on = lane >= 48 && lane < 54; const int c6 = on ? lane - 48 : 0;
            const double v = stage_t6(W, K0, L + L_HRD, L + L_HDP, c6);
            L[on ? L_QRB + (j & 1) * 40 + 32 + c6 : L_DUMMY] = v;
        }
    LANES_END
}
// the sweep's wave picks the helper's results up: into registers at the TOP of the Schur phase (the MFMA result overlays L_PREP)
struct PrepRegs { double add[16], c3inc[3], piinc; };
BMPC_D inline void team_prep_fetch(Wave &W, int lane, PrepRegs &r) {
    const double *o = W.L + L_PREP + lane;
#pragma unroll
    for (int q = 0; q < 16; q++) r.add[q] = 0.0;
    r.add[0] = o[0]; r.add[1] = o[64]; r.add[2] = o[128]; r.add[4] = o[192]; r.add[5] = o[256]; r.add[6] = o[320]; r.add[8] = o[384]; r.add[9] = o[448];
    r.add[10] = o[512]; r.add[15] = o[576];
    const double *c = W.L + L_PREP + PREP_C3 + (lane & 31);
    r.c3inc[0] = c[0]; r.c3inc[1] = c[32]; r.c3inc[2] = c[64];
    const bool onII = lane >= 32 && lane < 32 + 6;
    r.piinc = W.L[L_PREP + PREP_PII + (onII ? lane - 32 : 0)];
}
#elif BMPC_NW > 1
// Helper wave of a team's Riccati sweep: the recursion-independent half of the node-cost block add of stage j (blk_prep_lane), computed
// from the LDS-resident workspace rows of the stage while the sweep's wave works on stage j+1; results to L_PREP[j & 1] (plane-major) and the
// curvature table of parity j.
BMPC_D inline void team_blk_prep(Wave &W, const POff &po, const Scr &sc, int j, double delta) {
    const int N = W.N;
    double *L = W.L; const GPtr G = W.G; const LPtr WL = BMPC_WL(W);
    const int jn = j < N - 1 ? j + 1 : j;
    LANES_BEGIN      // per-joint curvature vectors of the stage from the global slab
        const double a_ = G[sc.KHV + j * KHV_STRIDE + lane], b_ = G[sc.KHV + j * KHV_STRIDE + 64 + lane], c_ = G[sc.KHV + j * KHV_STRIDE + 128 + (lane < 24 ? lane : 23)];
        L[L_HKHP + lane] = a_; L[L_HKHP + 64 + lane] = b_; L[L_HKHP + 128 + (lane < 24 ? lane : 23)] = c_;
    LANES_END
    LANES_BEGIN
        const double *row = WL + sc.NCS + j * NCS_STRIDE;
        BlkIn in; in.K0 = WL + sc.KIN + j * KREC; in.KV1 = WL + sc.KIN + (N + jn) * KREC; in.KHV = L + L_HKHP; in.NC = row; in.mu4 = row + NCS_MU;
        in.dpd = row + NCS_RDP; in.sgk = WL + sc.SG + j * NI;
        double add[16], c3inc[3], piinc, wpv[2][2];
        blk_prep_lane(W, po, j, delta, lane, in, add, c3inc, piinc, wpv);
        blk_store_wy(W, lane, (j & 1) ? L_WY2 : L_WY, wpv);
        double *o = L + L_PREP + (j & 1) * PREP_N * 64 + lane;
        o[0] = add[0]; o[64] = add[1]; o[128] = add[2]; o[192] = add[4]; o[256] = add[5]; o[320] = add[6]; o[384] = add[8]; o[448] = add[9];
        o[512] = add[10]; o[576] = add[15]; o[640] = c3inc[0]; o[704] = c3inc[1]; o[768] = c3inc[2]; o[832] = piinc;
        // gl of the stage = QP-gradient row + the non-trivial entries of gl - g^ (what backward_commit_lane forms for the one-wave sweep), into the
        // helper's own staging (L_HGL: the velocity-point record buffer the sweep's wave of a team no longer uses)
        {
            const int lz = lane < NZ ? lane : NZ - 1;
            const int t = lz >= ZV ? lz - ZV + 3 : lz - ZPOS; const bool sp = lz >= ZV || (lz >= ZPOS && lz < ZIW);
            L[L_HGL + lz] = WL[sc.GH + j * NZ + lz] + row[sp ? NCS_ADDV + t : NCS_ZERO];
        }
    LANES_END
    LANES_BEGIN      // q~ rows (32 chain rows) and t6 of the stage: recursion-independent too (they need the curvature table this wave just wrote)
        const double *row = WL + sc.NCS + j * NCS_STRIDE, *K0 = WL + sc.KIN + j * KREC;
        {
            const int r = lane < 32 ? lane : 0;
            const double qr = node_q_row_p(L, L + L_HGL, L + ((j & 1) ? L_WY2 : L_WY), WL + sc.G + j * NE, K0, r, W.h, W.o.exact_hessian);
            L[lane < 32 ? L_QRB + (j & 1) * 40 + r : L_DUMMY] = qr;
        }
        {
            const bool on = lane >= 48 && lane < 54; const int c6 = on ? lane - 48 : 0;
            const double v = stage_t6(W, K0, WL + sc.RDY + j * 36, row + NCS_RDP, c6);
            L[on ? L_QRB + (j & 1) * 40 + 32 + c6 : L_DUMMY] = v;
        }
    LANES_END
}
// the sweep's wave picks the helper's results of stage j up and finishes the block add
BMPC_D inline void team_blk_apply(Wave &W, int j, int lane, const double (&C)[4][4], const double (&ci3)[3], double pii, double pvv, double *Pb) {
    const double *o = W.L + L_PREP + (j & 1) * PREP_N * 64 + lane;
    double add[16], c3inc[3];
#pragma unroll
    for (int q = 0; q < 16; q++) add[q] = 0.0;
    add[0] = o[0]; add[1] = o[64]; add[2] = o[128]; add[4] = o[192]; add[5] = o[256]; add[6] = o[320]; add[8] = o[384]; add[9] = o[448];
    add[10] = o[512]; add[15] = o[576]; c3inc[0] = o[640]; c3inc[1] = o[704]; c3inc[2] = o[768];
    blk_apply_lane(W, lane, C, ci3, pii, pvv, add, c3inc, o[832], Pb);
}
#endif

BMPC_D inline bool wave_backward_blk(Wave &W, const POff &po, const Scr &sc, double mu, double delta, LaneRegs *LR) {
    const int N = W.N; const double h = W.h, h2 = h * h, h3 = h2 * h;
    double *L = W.L; const GPtr G = W.G; const LPtr WL = BMPC_WL(W);
    const double *PAR = L + L_PAR, *w = PAR + po.w;
    // Teams: every wave of the team runs this function (same control flow, one barrier per stage); the recursion is wave 0's (SOLO(0)), wave 1
    // prepares the node-cost block of the NEXT stage of the sweep beside it (SOLO(1): team_blk_prep), the other waves only keep the barriers.
#if BMPC_NW > 1 && defined(BMPC_WSG)
    SOLO_BEGIN(1)
    LANES_BEGIN
        helper_loads_lane(W, sc, N - 1, LR[LIDXH].pf, lane);
    LANES_END
    SOLO_END
#elif BMPC_NW > 1
    SOLO_BEGIN(1 % NW)
    team_blk_prep(W, po, sc, N - 1, delta);
    SOLO_END
#endif
    SOLO_BEGIN(0)
    LANES_BEGIN
        for (int id = lane; id < 96 + 12; id += 64) L[L_PCI + id] = 0.0;
        if (lane < 36) L[L_PV + lane] = 0.0;
        backward_loads_lane(W, sc, N - 1, LR[LIDX].pf, lane, true);
    LANES_END
    LANES_BEGIN
        backward_commit_lane(W, N - 1, LR[LIDX].pf, lane, true);
        backward_loads_lane(W, sc, N >= 2 ? N - 2 : 0, LR[LIDX].pf, lane, false);
    LANES_END
    SOLO_END
    backward_buffers(N, N - 1, W.oK0, W.oK1, W.oKV, W.oKV1);
#if BMPC_NW > 1 && defined(BMPC_WSG)
    // pairs: the helper's prep of the last stage reads that stage's record from the buffer the sweep's wave just committed (first barrier), and
    // the sweep's wave waits for the result (second); once per sweep -- inside the loop the helper runs a stage ahead, beside the recursion
    TEAM_SYNC_LDS();
    SOLO_BEGIN(1)
    team_blk_prep(W, po, sc, N - 1, delta, LR, false);
    SOLO_END
#endif
    TEAM_SYNC_LDS();      // (the helper's block data of the last stage is in LDS)
    SOLO_BEGIN(0)
    LANES_BEGIN   // value function of the last node = its node cost: the block add on a zero block
        const double Z4[4][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}}, Z3[3] = {0, 0, 0};
#if BMPC_NW > 1 && defined(BMPC_WSG)
        PrepRegs pq; team_prep_fetch(W, lane, pq);
        blk_apply_lane(W, lane, Z4, Z3, 0.0, 0.0, pq.add, pq.c3inc, pq.piinc, LR[LIDX].mc);
#elif BMPC_NW > 1
        team_blk_apply(W, N - 1, lane, Z4, Z3, 0.0, 0.0, LR[LIDX].mc);
#else
        blk_add_lane(W, po, N - 1, delta, lane, W.oK0, W.oKV1, Z4, Z3, 0.0, 0.0, LR[LIDX].mc);
#endif
    LANES_END
#if BMPC_NW > 1 && defined(BMPC_WSG)
    if (N >= 2) { TEAM_SYNC_LDS(); }      // the second barrier of "stage N": L_PREP has been read (matches the helper's prep of stage N - 2)
#endif
    SOLO_END
    for (int k = N - 1; k >= 0; k--) {
#if BMPC_NW > 1
        if (k >= 1) {
            SOLO_BEGIN(1 % NW)
#ifdef BMPC_WSG
            team_blk_prep(W, po, sc, k - 1, delta, LR, true);      // beside the recursion's stage k; handed over at the barrier below
#else
            team_blk_prep(W, po, sc, k - 1, delta);      // beside the recursion's stage k; handed over at the barrier below
#endif
            SOLO_END
        }
        const int oWYk = (k & 1) ? L_WY2 : L_WY, oFLAGk = L_FLAG + 2 + (k & 1), oQRk = L_QRB + (k & 1) * 40, oT6k = oQRk + 32;
#else
        constexpr int oWYk = L_WY, oFLAGk = L_FLAG, oT6k = L_T6;
#endif
        SOLO_BEGIN(0)
        BMPC_PROF(W, 6);
        backward_buffers(N, k, W.oK0, W.oK1, W.oKV, W.oKV1);
        BMPC_PROF(W, 24);
        // (the lanes' register blocks + PCI / PII / PV hold the value function of node k+1 including its node cost: blk_add_lane, in the
        // prologue for the last stage and at the end of the Schur phase of stage k+1 otherwise)
        BMPC_PROF(W, 5);
        BMPC_PROF(W, 11);
        // ---- S0: PR = P' rdyn + p ; C^T P_c,iota ; P_ii E ----
        // The five roles of this phase are written as PREDICATED straight-line code (every lane runs every role on a clamped,
        // always-valid index; only the final stores are conditional): one basic block, so the scheduler overlaps the LDS
        // round trips of the roles instead of running them one after the other.
        LANES_BEGIN
            {   // chain rows (f,i) of PR
                const bool on = lane < 32; const int r = on ? lane : 0;
                const int code = (int)L[L_ZMAP + r], f = (code >> 17) & 7, i = (code >> 20) & 7;     // (field, chain) of the row, from the row table
                BMPC_ACC4_DECL(pa);
#pragma unroll
                for (int l = 0; l < 8; l++) BMPC_ACC4(pa, l, L[L_PP + f * 64 + i * 8 + l]);        // partial products of the eight pairs of chain i (blk_add_lane)
#pragma unroll
                for (int a = 0; a < 3; a++) BMPC_ACC4(pa, a, L[L_PCI + pci(a, f, i)] * L[L_RD + SIOTA + a]);
#if BMPC_NW > 1
                const double qr = L[oQRk + r];          // q~ of node k+1, from the helper wave (team_blk_prep)
#else
                const double qr = node_q_row(L, L + W.oK0, r, h, W.o.exact_hessian, oWYk);          // q~ of node k+1 joins the value-function gradient here
#endif
                L[L_PR + r] = (L[L_PV + r] + qr) + BMPC_ACC4_SUM(pa);      // off-lanes repeat row 0 (same value): no conditional store
            }
            {   // iota rows of PR
                const bool on = lane >= 32 && lane < NS; const int a = on ? lane - SIOTA : 0;
                BMPC_ACC4_DECL(pa);
#pragma unroll
                for (int l = 0; l < 8; l++)
#pragma unroll
                    for (int g = 0; g < 3; g++) BMPC_ACC4(pa, g, L[L_PCI + pci(a, g, l)] * L[L_RD + srow(g, l)]);
#pragma unroll
                for (int b2 = 0; b2 < 3; b2++) BMPC_ACC4(pa, b2, L[L_PII + a * 3 + b2] * L[L_RD + SIOTA + b2]);
                L[L_PR + SIOTA + a] = (L[L_PV + SIOTA + a] + L[L_NC + NC_GL + ZIW + a]) + BMPC_ACC4_SUM(pa);   // iota rows of q~: gl[iw]
            }
            {   // U[(f',i)][a] = sum_f CF[f][f'] P[(f,i)][iota_a]
                const bool on = lane < 40; const int ln = on ? lane : 0, fp = ln >> 3, i = ln & 7;
                double u[3];
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    u[a] = 0;
#pragma unroll
                    for (int f = 0; f < 4; f++) u[a] += L[L_CFT + f * 5 + fp] * L[L_PCI + pci(a, f, i)];
                }
                L[L_MCI + mci(0, fp, i)] = u[0]; L[L_MCI + mci(1, fp, i)] = u[1]; L[L_MCI + mci(2, fp, i)] = u[2];
            }
            {   // PE = P_ii E
                const bool on = lane < 42; const int ln = on ? lane : 0, a = ln / 14, y = ln % 14; double sacc = 0;
#pragma unroll
                for (int b2 = 0; b2 < 3; b2++) sacc += L[L_PII + a * 3 + b2] * L[L_AE + b2 * 14 + y];
                L[L_PE + ln] = sacc;
            }
            {   // t6 = C rdyn: the rdyn side of X^T rdyn = Gv(K1)^T (C rdyn)
#if BMPC_NW == 1
                const bool on = k >= 1 && lane >= 48 && lane < 54; const int c6 = on ? lane - 48 : 0;
                const double v = stage_t6(W, L + W.oK0, L + L_RD, L + L_ST + ST_REF + RDP, c6);
                L[on ? L_T6 + c6 : L_DUMMY] = v;
#endif      // (teams: the helper wave delivered t6 with the q~ rows, team_blk_prep)
            }
        LANES_END
        BMPC_PROF(W, 21);
        // ---- S0b: M_c,iota = U + E^T P_ii ; gradient column m = F^T PR + S^T X^T rdyn ----
        LANES_BEGIN   // predicated straight-line code
            {
                const bool on = lane < 40; const int ln = on ? lane : 0, fp = ln >> 3, i = ln & 7;
                const bool yq = fp <= 1 && i < 7;                   // (q, dq) rows couple with iota through E and with the next node through X
                const int y = yq ? fp * 7 + i : 0, ic = i < 7 ? i : 0;
                double mc3[3];
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    double sacc = 0;
#pragma unroll
                    for (int b2 = 0; b2 < 3; b2++) sacc += L[L_AE + b2 * 14 + y] * L[L_PII + b2 * 3 + a];
                    mc3[a] = L[L_MCI + mci(a, fp, i)] + sacc;
                }
                double v = 0, ve = 0, sx = 0;
#pragma unroll
                for (int f = 0; f < 4; f++) v += L[L_CFT + f * 5 + fp] * L[L_PR + srow(f, i)];
#pragma unroll
                for (int a = 0; a < 3; a++) ve += L[L_AE + a * 14 + y] * L[L_PR + SIOTA + a];
                {
                    const double *K1 = L + W.oK1;
#pragma unroll
                    for (int c6 = 0; c6 < 6; c6++) sx += K1[(fp == 0 ? KD + c6 * 7 : (c6 < 3 ? KW + c6 * 7 : KA + (c6 - 3) * 7)) + ic] * L[oT6k + c6];
                }
                v += (yq ? 1.0 : 0.0) * ve + ((yq && k >= 1) ? 1.0 : 0.0) * sx;
                {   // unconditional stores, the row kind selects the address (lanes without a row write to the dummy word)
                    const bool sm = on && yq;
                    L[sm ? L_MCI + mci(0, fp, i) : L_DUMMY] = mc3[0]; L[sm ? L_MCI + mci(1, fp, i) : L_DUMMY] = mc3[1]; L[sm ? L_MCI + mci(2, fp, i) : L_DUMMY] = mc3[2];
                    int vd = L_DUMMY; vd = (on && fp == 4) ? L_GS + i * 36 + 35 : vd; vd = (on && fp < 4) ? L_MV + srow(fp, i) : vd;
                    L[vd] = v;
                }
            }
            {
                const bool on = lane >= 40 && lane < 43; const int a = on ? lane - 40 : 0; const double v = L[L_PR + SIOTA + a];
                L[L_MV + SIOTA + a] = v;
            }
            {   // jerk rows of the iota columns: M[u_i][iota_a] = M_c,iota[(4,i)][a] (rows f' = 4 of U are final after S0; lanes >= 24
                // repeat a = 0: identical values)
                const int i = lane & 7, a = lane < 24 ? lane >> 3 : 0; const double v = L[L_MCI + mci(a, 4, i)];
                L[L_GS + i * 36 + SIOTA + a] = v;
            }
        LANES_END
        BMPC_PROF(W, 22);
        // ---- S1: one lane per chain pair: 5x5 block of M = F^T P' F (+ iota and acceleration cross terms) ----
        LANES_BEGIN
            const int i = lane >> 3, l = lane & 7, ci = i < l ? i : l, cl = i < l ? l : i; const bool tr = i > l;
            double B[4][4], T[4][5], M5[5][5];
            {   // the canonical pair's block from the lane's own registers (a mirrored lane holds the transpose)
                const double *Pb = LR[LIDX].mc;
#pragma unroll
                for (int f = 0; f < 4; f++)
#pragma unroll
                    for (int g = 0; g < 4; g++) B[f][g] = tr ? Pb[g * 4 + f] : Pb[f * 4 + g];
            }
#pragma unroll
            for (int f = 0; f < 4; f++) {
                T[f][0] = B[f][0]; T[f][1] = h * B[f][0] + B[f][1]; T[f][2] = h2 / 2 * B[f][0] + h * B[f][1] + B[f][2];
                T[f][3] = h3 / 8 * B[f][0] + h2 / 3 * B[f][1] + h / 2 * B[f][2];
                T[f][4] = h3 / 24 * B[f][0] + h2 / 6 * B[f][1] + h / 2 * B[f][2] + B[f][3];
            }
#pragma unroll
            for (int g = 0; g < 5; g++) {
                M5[0][g] = T[0][g]; M5[1][g] = h * T[0][g] + T[1][g]; M5[2][g] = h2 / 2 * T[0][g] + h * T[1][g] + T[2][g];
                M5[3][g] = h3 / 8 * T[0][g] + h2 / 3 * T[1][g] + h / 2 * T[2][g];
                M5[4][g] = h3 / 24 * T[0][g] + h2 / 6 * T[1][g] + h / 2 * T[2][g] + T[3][g];
            }
            // ---- all remaining operands are loaded up front (clamped indices, 0/1 masks instead of branches) so that
            //      the LDS latency is paid once per phase, not once per term ----
            const double ml = cl < 7 ? 1.0 : 0.0, mi = ci < 7 ? 1.0 : 0.0, mx = k >= 1 ? 1.0 : 0.0;
            const int cic = ci < 7 ? ci : 0, clc = cl < 7 ? cl : 0;
            double Ei[2][3], El[2][3], Ui[5][3], Ul[5][3], PEl[2][3], Xl[2][3], Xi[2][3];
#pragma unroll
            for (int g = 0; g < 2; g++)
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    El[g][a] = ml * L[L_AE + a * 14 + g * 7 + clc]; Ei[g][a] = mi * L[L_AE + a * 14 + g * 7 + cic];
                    PEl[g][a] = ml * L[L_PE + a * 14 + g * 7 + clc];
                }
#pragma unroll
            for (int f = 0; f < 5; f++)
#pragma unroll
                for (int a = 0; a < 3; a++) { Ui[f][a] = L[L_MCI + mci(a, f, ci)]; Ul[f][a] = L[L_MCI + mci(a, f, cl)]; }
            // acceleration cross block entries for chain ci / cl: X[q+_c], X[dq+_c] (chains < 7) or X[ddphi+] (chain 7), contracted
            // on the fly from the rank-6 factors: X[r][c] = sum_c6 C[c6][r] Gv(K1)[c6][c], C = -2 w_a/h^2 Gv(K0) (rows < 14), 2 w_a/h dpn
            {
                const double *K0 = L + W.oK0, *K1 = L + W.oK1, *dpn = L + L_ST + ST_REF + RDP;
                const double fx = -W.ca * mx * ml * mi, fphi = W.cb * mx * mi * (1.0 - ml);
                double xl0[2] = {0, 0}, xl1[2] = {0, 0}, xi0[2] = {0, 0}, xi1[2] = {0, 0}, xi2[2] = {0, 0};
#pragma unroll
                for (int c6 = 0; c6 < 6; c6++) {
                    const int jo = c6 < 3 ? KW + c6 * 7 : KA + (c6 - 3) * 7;       // J row of the record ([J_v; J_w])
                    const double a0 = K0[KD + c6 * 7 + cic], a1 = K0[jo + cic], b0 = K0[KD + c6 * 7 + clc], b1 = K0[jo + clc];
                    const double cl0 = K1[KD + c6 * 7 + clc], cl1 = K1[jo + clc], ci0 = K1[KD + c6 * 7 + cic], ci1 = K1[jo + cic], dp = dpn[c6];
                    xl0[0] += a0 * cl0; xl0[1] += a0 * cl1; xl1[0] += a1 * cl0; xl1[1] += a1 * cl1;
                    xi0[0] += b0 * ci0; xi0[1] += b0 * ci1; xi1[0] += b1 * ci0; xi1[1] += b1 * ci1;
                    xi2[0] += dp * ci0; xi2[1] += dp * ci1;
                }
#pragma unroll
                for (int g = 0; g < 2; g++) {
                    Xl[g][0] = fx * xl0[g]; Xl[g][1] = fx * xl1[g]; Xl[g][2] = 0.0;
                    Xi[g][0] = fx * xi0[g]; Xi[g][1] = fx * xi1[g]; Xi[g][2] = fphi * xi2[g];
                }
            }
            // iota coupling: + Mci E + (Mci E)^T - E^T Pii E ; acceleration cross term: + F^T X S + S^T X^T F
#pragma unroll
            for (int g = 0; g < 2; g++)
#pragma unroll
                for (int f = 0; f < 5; f++)
                    M5[f][g] += Ui[f][0] * El[g][0] + Ui[f][1] * El[g][1] + Ui[f][2] * El[g][2]
                              + chain_cf(h, 0, f) * Xl[g][0] + chain_cf(h, 1, f) * Xl[g][1] + chain_cf(h, 2, f) * Xl[g][2];
#pragma unroll
            for (int f = 0; f < 2; f++) {
#pragma unroll
                for (int g = 0; g < 5; g++)
                    M5[f][g] += Ul[g][0] * Ei[f][0] + Ul[g][1] * Ei[f][1] + Ul[g][2] * Ei[f][2]
                              + chain_cf(h, 0, g) * Xi[f][0] + chain_cf(h, 1, g) * Xi[f][1] + chain_cf(h, 2, g) * Xi[f][2];
#pragma unroll
                for (int g = 0; g < 2; g++) M5[f][g] -= Ei[f][0] * PEl[g][0] + Ei[f][1] * PEl[g][1] + Ei[f][2] * PEl[g][2];
            }
            if (ci == cl) {   // exact symmetry of the diagonal pairs
#pragma unroll
                for (int f = 0; f < 5; f++)
#pragma unroll
                    for (int g = 0; g < f; g++) M5[f][g] = M5[g][f];
            }
            double *mc = LR[LIDX].mc;
#pragma unroll
            for (int f = 0; f < 4; f++)
#pragma unroll
                for (int g = 0; g < 4; g++) mc[f * 4 + g] = M5[f][g];
            // publish the jerk rows: GS[u_l][(f,i)] = own[f][4], R8[i][l] = M[u_i][u_l]
#pragma unroll
            for (int f = 0; f < 4; f++) L[L_GS + l * 36 + gcol(f, i)] = tr ? M5[4][f] : M5[f][4];
            L[L_R8 + i * 8 + l] = M5[4][4];
        LANES_END
        BMPC_PROF(W, 12);
        // ---- S2: 8x8 Cholesky (identical data in every lane), gains ----
        LANES_BEGIN
            if (k >= 1) {   // inputs of stage k-1 (loaded a stage ago) replace this stage's in the staging area and the record buffers,
                            // all dead since S1; then the loads for stage k-2 into the registers this frees
                backward_commit_lane(W, k - 1, LR[LIDX].pf, lane, false);
                backward_loads_lane(W, sc, k >= 2 ? k - 2 : 0, LR[LIDX].pf, lane, false);
            }
            BMPC_PROF(W, 19);
            double Lc[NU][NU], dinv[NU]; bool pd = true;
#pragma unroll
            for (int a = 0; a < NU; a++) {
#pragma unroll
                for (int b = 0; b <= a; b++) {
                    double sacc = L[L_R8 + a * 8 + b];
#pragma unroll
                    for (int q = 0; q < b; q++) sacc -= Lc[a][q] * Lc[b][q];
                    if (a == b) { if (!(sacc > 1e-13)) { pd = false; sacc = 1.0; } dinv[a] = BMPC_RSQRT(sacc); Lc[a][a] = sacc * dinv[a]; }
                    else Lc[a][b] = sacc * dinv[b];
                }
            }
            BMPC_PROF(W, 20);
            L[oFLAGk] = pd ? 1.0 : 0.0;            // identical in every lane
            {   // gains: one column per lane (lanes >= 36 repeat column 0: identical values, duplicate stores; when the block is not
                // positive definite the values are discarded with the whole sweep)
                const int c = lane < 36 ? lane : 0; double kc[NU];
#pragma unroll
                for (int a = 0; a < NU; a++) kc[a] = -L[L_GS + a * 36 + c];
#pragma unroll
                for (int a = 0; a < NU; a++) { double sacc = kc[a];
#pragma unroll
                    for (int q = 0; q < a; q++) sacc -= Lc[a][q] * kc[q];
                    kc[a] = sacc * dinv[a]; }
#pragma unroll
                for (int a = NU - 1; a >= 0; a--) { double sacc = kc[a];
#pragma unroll
                    for (int q = a + 1; q < NU; q++) sacc -= Lc[q][a] * kc[q];
                    kc[a] = sacc * dinv[a]; }
#pragma unroll
                for (int a = 0; a < NU; a++) L[L_KS + a * 36 + c] = kc[a];
                // gains to the workspace for the forward sweep, control-major ([control][reduced-state index], 8 x 35 per stage): the 36
                // column lanes write neighbouring words of one row per store instruction (measured neutral against the state-major
                // layout: the stores ride behind the triangular solves either way); the feed-forward column goes to KF
                const int gcoff = c < NS ? sc.KT + k * NS * NU + prow(c) : sc.KF + k * NU, gstr = c < NS ? NS : 1;
#pragma unroll
                for (int a = 0; a < NU; a++) G[gcoff + a * gstr] = kc[a];
            }
        LANES_END
        BMPC_PROF(W, 23);
        SOLO_END
        // Team: the stage's one barrier.  Behind it the verdict of the 8x8 factorisation and the helper's half of the node-cost add of stage
        // k-1 (L_PREP, the curvature table) are in LDS.  Only LDS words cross here, so the barrier does not drain the vector-memory
        // counter: the sweep's register prefetch of stage k-2 stays in flight (TEAM_SYNC_LDS).
        TEAM_SYNC_LDS();
        if (L[oFLAGk] == 0.0) return false;            // (teams: every wave reads the same word, written two stages apart per parity)
        // ---- S3: Schur complement, block lanes write the value function of node k ----
        SOLO_BEGIN(0)
        if (k >= 1) {
            LANES_BEGIN
                const int i = lane >> 3, l = lane & 7, ci = i < l ? i : l, cl = i < l ? l : i; const bool tr = i > l;
                const double *mc = LR[LIDX].mc;
                double C[4][4];
#if BMPC_NW > 1 && defined(BMPC_WSG)
                PrepRegs pq; team_prep_fetch(W, lane, pq);      // the helper's half of the node-cost add of stage k - 1: read before the Schur result overlays it
#endif
#ifdef BMPC_MFMA
                // GPU build: the rank-8 update D = GS^T KS of the 32 x 32 chain block is the one dense contraction of the stage and
                // runs on the matrix cores: v_mfma_f64_16x16x4_f64, 2 x 2 tiles x 2 k-steps.  Operand maps (one f64 per lane):
                // A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15]; result register v of a lane holds
                // D[row = (lane >> 4) + 4 v][col = lane & 15].  D is dropped in natural 32 x 32 layout into the PB area (the old
                // value function is dead since S1) and every pair lane picks its 16 entries from there: 8 + 16 LDS reads per lane
                // instead of 128, 8 MFMAs instead of 128 FMAs.  (The emulator and the oracle run the plain loops below; LDS
                // operations of the one wave execute in program order, so the reads of D precede the block stores that overwrite it.)
                {
                    typedef double bmpc_d4 __attribute__((ext_vector_type(4)));
                    const int lr = lane & 15, lk = lane >> 4;
                    double a_[2][2], b_[2][2];
#pragma unroll
                    for (int t = 0; t < 2; t++)
#pragma unroll
                        for (int ks = 0; ks < 2; ks++) { a_[t][ks] = L[L_GS + (4 * ks + lk) * 36 + 16 * t + lr]; b_[t][ks] = L[L_KS + (4 * ks + lk) * 36 + 16 * t + lr]; }
#pragma unroll
                    for (int tr_ = 0; tr_ < 2; tr_++)
#pragma unroll
                        for (int tc = 0; tc < 2; tc++) {
                            bmpc_d4 acc = {0.0, 0.0, 0.0, 0.0};
                            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a_[tr_][0], b_[tc][0], acc, 0, 0, 0);
                            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a_[tr_][1], b_[tc][1], acc, 0, 0, 0);
#pragma unroll
                            for (int v = 0; v < 4; v++) L[L_PB + (16 * tr_ + lk + 4 * v) * 32 + 16 * tc + lr] = acc[v];
                        }
#pragma unroll
                    for (int f = 0; f < 4; f++)
#pragma unroll
                        for (int g = 0; g < 4; g++) C[f][g] = mc[f * 4 + g] + L[L_PB + gcol(f, ci) * 32 + gcol(g, cl)];
                }
#else
#pragma unroll
                for (int f = 0; f < 4; f++)
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        double sacc = mc[f * 4 + g];
#pragma unroll
                        for (int a = 0; a < NU; a++) sacc += L[L_GS + a * 36 + gcol(f, ci)] * L[L_KS + a * 36 + gcol(g, cl)];
                        C[f][g] = sacc;
                    }
#endif
                if (ci == cl) {
#pragma unroll
                    for (int f = 0; f < 4; f++)
#pragma unroll
                        for (int g = 0; g < f; g++) C[f][g] = C[g][f];
                }
#if BMPC_NW > 1 && defined(BMPC_WSG)
                // pairs, second barrier of the stage: L_PREP has been read and the Schur result that overlays it gathered -- the helper (waiting here since
                // its commit, a few hundred cycles after the stage's first barrier) may write the hand-over of stage k - 2.  k >= 2: that helper call exists.
                if (k >= 2) { TEAM_SYNC_LDS(); }
#endif
                BMPC_PROF(W, 14);
                // the small roles (chain x iota, iota x iota, gradient) are predicated and evaluated BEFORE any store of this phase,
                // so that all LDS reads of the phase can be in flight together
                const int lf = (lane & 31) >> 3, lii = lane & 7;
                double ci3[3];
#pragma unroll
                for (int b2 = 0; b2 < 3; b2++) {
                    double sacc = L[L_MCI + mci(b2, lf, lii)];
#pragma unroll
                    for (int a = 0; a < NU; a++) sacc += L[L_GS + a * 36 + gcol(lf, lii)] * L[L_KS + a * 36 + SIOTA + b2];
                    ci3[b2] = sacc;
                }
                const bool onII = lane >= 32 && lane < 32 + 6; const int t = onII ? lane - 32 : 0;
                const int ib = t < 3 ? 0 : (t < 5 ? 1 : 2), ic = t < 3 ? t : (t < 5 ? t - 2 : 2);
                double pii = L[L_PII + ib * 3 + ic];
#pragma unroll
                for (int a = 0; a < NU; a++) pii += L[L_GS + a * 36 + SIOTA + ib] * L[L_KS + a * 36 + SIOTA + ic];
                const bool onPV = lane < NS; const int pr_ = onPV ? lane : 0;
                double pvv = L[L_MV + pr_];
                const int pc_ = pcol(pr_);
#pragma unroll
                for (int a = 0; a < NU; a++) pvv += L[L_GS + a * 36 + pc_] * L[L_KS + a * 36 + 35];
                BMPC_PROF(W, 17);
                // ---- node cost of stage k-1 added to the block just formed (registers), iota couplings, gradient, partial products: no
                //      store of the chain blocks any more ----
#if BMPC_NW > 1 && defined(BMPC_WSG)
                blk_apply_lane(W, lane, C, ci3, pii, pvv, pq.add, pq.c3inc, pq.piinc, LR[LIDX].mc);      // (the recursion-independent half came from the helper wave)
#elif BMPC_NW > 1
                team_blk_apply(W, k - 1, lane, C, ci3, pii, pvv, LR[LIDX].mc);      // (the recursion-independent half came from the helper wave)
#else
                {
                    int q0_, q1_, q2_, q3_; backward_buffers(N, k - 1, q0_, q1_, q2_, q3_);
                    blk_add_lane(W, po, k - 1, delta, lane, q0_, q3_, C, ci3, pii, pvv, LR[LIDX].mc);
                }
#endif
                BMPC_PROF(W, 30);
            LANES_END
        }
        SOLO_END
        BMPC_PROF(W, 13);
    }
    return true;
}

// forward sweep: dZ[N][44].  The stages are short (shorter than a memory round trip), so the inputs of a stage (gains, defects,
// kinematics record) are loaded into registers three stages ahead (two register sets, the stage loop is unrolled by two) and
// committed to LDS one stage ahead, double-buffered by stage parity (staging area: L_ST / the idle gain area L_GS; record:
// L_K0 / L_K1); the commit burst and the next loads ride at the end of a stage's last phase: three phases per stage.
// (what only the dZ rows read: lifted residuals, the kinematics record, the QP-gradient entry of the component of dZ the lane writes; a team
// forms the dZ rows of all stages in a wide pass behind the sweep -- wave_dz_wide -- from the LDS-resident rows and does not stage them)
#if BMPC_NW == 1
#define BMPC_FWD_LOADS_DZ(j) \
    pf[8] = WL[sc.RLV + j * 12 + (lane < 12 ? lane : 11)]; \
    pf[9] = WL[sc.KIN + j * KREC + lane]; pf[10] = WL[sc.KIN + j * KREC + (lane < KREC - 64 ? 64 + lane : KREC - 1)]; \
    { const int t_ = lane < NZ ? lane : 0, r_ = t_ < NS ? t_ : 0; int z_ = (int)L[L_ZMAP + r_] & 255; z_ = t_ >= NS ? (t_ < NS + 3 ? ZPOS + t_ - NS : ZV + t_ - NS - 3) : z_; \
      pf[11] = WL[sc.GH + j * NZ + z_]; }
#define BMPC_FWD_COMMIT_DZ() \
    sb_[ST_RLVF + (lane < 12 ? lane : 11)] = pf[8]; \
    kb_[lane] = pf[9]; kb_[lane < KREC - 64 ? 64 + lane : KREC - 1] = pf[10]; sb_[ST_GHF + lane] = pf[11];
#else
#define BMPC_FWD_LOADS_DZ(j)
#define BMPC_FWD_COMMIT_DZ()
#endif
#define BMPC_FWD_LOADS(j_, PO_) { double *pf = LR[LIDX].pf + (PO_); const int j = (j_) < N ? (j_) : N - 1; \
    _Pragma("unroll") for (int u = 0; u < 5; u++) { const int id = lane + 64 * u; pf[u] = G[sc.KT + j * NS * NU + (id < NS * NU ? id : NS * NU - 1)]; } \
    pf[5] = G[sc.KF + j * NU + (lane < NU ? lane : NU - 1)]; \
    pf[6] = WL[sc.RDY + j * 36 + (lane < 36 ? lane : 35)]; \
    pf[7] = WL[sc.AES + j * 42 + (lane < 42 ? lane : 41)]; \
    BMPC_FWD_LOADS_DZ(j) }
#define BMPC_FWD_COMMIT(j_, PO_) { const double *pf = LR[LIDX].pf + (PO_); const int odd_ = (j_) & 1; double *sb_ = L + (odd_ ? L_GS : L_ST), *kb_ = L + (odd_ ? L_K1 : L_K0); \
    _Pragma("unroll") for (int u = 0; u < 5; u++) { const int id = lane + 64 * u; sb_[ST_KT + (id < NS * NU ? id : NS * NU - 1)] = pf[u]; } \
    sb_[ST_KF + (lane < NU ? lane : NU - 1)] = pf[5]; \
    sb_[ST_RDY + (lane < 36 ? lane : 35)] = pf[6]; \
    sb_[ST_AES + (lane < 42 ? lane : 41)] = pf[7]; \
    BMPC_FWD_COMMIT_DZ() }
// dZ rows of stage k from the stage's next reduced state dn (LDS): lanes 0..34 scatter the reduced state through the row map (iota rows add
// their lifting term), lanes 35..43 evaluate the lifted rows (pos 3, v 6); contiguous lane ranges = shallow selects, no branch nest.
// sb / K0: the staging buffer and the kinematics record of stage k.
// rlv: the stage's lifted residuals (12), gh: QP-gradient row of the stage indexed by the component of Z (one-wave: null -- the lane's entry was
// staged at sb[ST_GHF + lane]); item lane t = 0..43; returns the lane's share of (QP gradient) . dZ.
template <class PR, class PK, class PG>
BMPC_D inline double forward_dz_item(Wave &W, int k, int t0, const double *dn, const PR rlv, const PK K0, const PG ghrow, bool has_row, const double *ghf) {
    double *L = W.L; const double h = W.h;
    const bool on = t0 < NZ; const int t = on ? t0 : 0;
    const bool isIw = t >= SIOTA && t < NS, isPos = t >= NS && t < NS + 3, isV = t >= NS + 3;
    const int c = isIw ? t - SIOTA : (isPos ? t - NS : (isV ? t - NS - 3 : 0));              // c6 for the v rows
    const int r = t < NS ? t : 0;
    // flat chains of selects on integers and 0/1 factors on values: no exec-mask branch in the phase
    int z = (int)L[L_ZMAP + r] & 255; z = isPos ? ZPOS + c : z; z = isV ? ZV + c : z;
    int p1 = KD + c * 7; p1 = isIw ? KD + (3 + c) * 7 : p1; p1 = isPos ? KW + c * 7 : p1;
    int p2 = c < 3 ? KW + c * 7 : KA + (c - 3) * 7; p2 = isIw ? KA + c * 7 : p2;
    BMPC_ACC4_DECL(za);
#pragma unroll
    for (int i = 0; i < 7; i++) { BMPC_ACC4(za, i, K0[p1 + i] * dn[SQ + i]); }
    BMPC_ACC4_DECL(zb);
#pragma unroll
    for (int i = 0; i < 7; i++) { BMPC_ACC4(zb, i, K0[p2 + i] * dn[SDQ + i]); }
    const double s1 = BMPC_ACC4_SUM(za), s2 = BMPC_ACC4_SUM(zb);
    const double ml = (isPos || isV) ? 1.0 : 0.0, addv = ml * rlv[isPos ? c : 3 + c] + (1.0 - ml) * dn[r];
    double fa = 0.0; fa = isV ? 1.0 : fa; fa = isIw ? 0.5 * h : fa; fa = isPos ? 1.0 : fa;
    const double v = addv + fa * (s1 + ((isIw || isV) ? 1.0 : 0.0) * s2);
    W.Dz[k * NZ + z] = v;
    const double ghe = has_row ? ghrow[z] : ghf[t0];      // (has_row: a compile-time constant at every call site)
    return on ? ghe * v : 0.0;      // (QP gradient) . dZ for the line search, summed where dZ is made
}
BMPC_D inline void forward_dz_lane(Wave &W, LaneRegs *LR, int k, int lane, const double *dn, const double *sb, const double *K0) {
    LR[LIDX].ghd += forward_dz_item(W, k, lane, dn, sb + ST_RLVF, K0, sb, false, sb + ST_GHF);
}
// one stage of the forward sweep (two phases since round 4: the reduced state ping-pongs between L_DS and L_DSN by stage parity instead of
// being copied back in a phase of its own, and the dZ rows of stage k-1 -- which need that stage's complete next state -- ride in the
// first phase of stage k, beside the partial sums of du: the two share no data); PO = register set that holds the inputs of stage k+1
template <int PO>
BMPC_D inline void forward_stage(Wave &W, const Scr &sc, LaneRegs *LR, int k) {
    const int N = W.N; const double h = W.h;
    double *L = W.L; const GPtr G = W.G; const LPtr WL = BMPC_WL(W);
    const double *sb = L + ((k & 1) ? L_GS : L_ST), *K0 = L + ((k & 1) ? L_K1 : L_K0);
    const double *sbp = L + ((k & 1) ? L_ST : L_GS), *K0p = L + ((k & 1) ? L_K0 : L_K1);      // stage k-1's (their buffers are rewritten at the END of stage k)
    const double *ds = L + ((k & 1) ? L_DSN : L_DS); double *dsn = L + ((k & 1) ? L_DS : L_DSN);
    LANES_BEGIN   // du = kff + K ds: partial sums on all 64 lanes (control u = lane & 7, every 8th state b), reduced by the consumers
        {
            const int u = lane & 7, part = lane >> 3; double acc = 0.0;
#pragma unroll
            for (int j = 0; j < 5; j++) { const int b0 = part + 8 * j, b = b0 < NS ? b0 : NS - 1; const double pr_ = sb[ST_KT + u * NS + b] * ds[b]; acc += b0 < NS ? pr_ : 0.0; }
            L[L_RED + part * 8 + u] = acc;
        }
#if BMPC_NW == 1
        if (k >= 1) forward_dz_lane(W, LR, k - 1, lane, ds, sbp, K0p);      // wave-uniform condition; ds = the next state of stage k-1
#endif
    LANES_END
    LANES_BEGIN   // next reduced state, predicated: chain rows and iota rows evaluated by every lane on clamped indices
        {
            const bool on = lane < NS; const int r = on ? lane : 0;
            const bool chain = r < SIOTA;
            const int code = (int)L[L_ZMAP + r], f = (code >> 17) & 7, i = chain ? (code >> 20) & 7 : 7, a = chain ? 0 : r - SIOTA;
            const double *dp_ = L + L_RED + i;   // fixed-order tree over the 8 partial sums of du
            const double du_i = sb[ST_KF + i] + (((dp_[0] + dp_[8]) + (dp_[16] + dp_[24])) + ((dp_[32] + dp_[40]) + (dp_[48] + dp_[56])));
            double vc = 0;
#pragma unroll
            for (int fc = 0; fc < 4; fc++) vc += L[L_CFT + f * 5 + fc] * ds[srow(fc, i)];
            vc += L[L_CFT + f * 5 + 4] * du_i;
            BMPC_ACC4_DECL(ia);
#pragma unroll
            for (int y = 0; y < 14; y++) BMPC_ACC4(ia, y, sb[ST_AES + a * 14 + y] * ds[y]);
            const double mc_ = chain ? 1.0 : 0.0;            // 0/1 factors, not a select between loaded values (that would be a branch)
            const double v = sb[ST_RDY + r] + (mc_ * vc + (1.0 - mc_) * (ds[r] + BMPC_ACC4_SUM(ia)));
            dsn[r] = v;            // (off-lanes repeat row 0 with the same value)
#if BMPC_NW > 1
            L[L_DSA + k * 36 + r] = v;      // teams: kept for the wide dZ pass behind the sweep (wave_dz_wide)
#endif
        }
        // inputs of stage k+1 into the other LDS buffer set (loaded two stages ago), then the loads of stage k+3 (clamped to the
        // last stage) into the registers this just freed
        BMPC_FWD_COMMIT(k + 1, PO)
        BMPC_FWD_LOADS(k + 3, PO)
    LANES_END
}
BMPC_D inline void wave_forward(Wave &W, const Scr &sc, LaneRegs *LR) {
    const int N = W.N;
    double *L = W.L; const GPtr G = W.G; const LPtr WL = BMPC_WL(W);
    static_assert(ST_GHF + 64 <= 288 + 64 + 288 && ST_GHF + 64 <= 460, "forward staging buffers must fit into L_ST and into the idle GS/R8/KS area");
    LANES_BEGIN
        if (lane < 36) L[L_DS + lane] = 0.0;
        LR[LIDX].ghd = 0.0;
        BMPC_FWD_LOADS(0, 0)
        BMPC_FWD_LOADS(1, 12)
    LANES_END
    LANES_BEGIN
        BMPC_FWD_COMMIT(0, 0)
        BMPC_FWD_LOADS(2, 0)
    LANES_END
    int k = 0;
    for (; k + 1 < N; k += 2) { forward_stage<12>(W, sc, LR, k); forward_stage<0>(W, sc, LR, k + 1); }
    if (k < N) forward_stage<12>(W, sc, LR, k);
#if BMPC_NW == 1
    LANES_BEGIN      // dZ rows of the last stage
        forward_dz_lane(W, LR, N - 1, lane, L + ((N & 1) ? L_DSN : L_DS), L + (((N - 1) & 1) ? L_GS : L_ST), L + (((N - 1) & 1) ? L_K1 : L_K0));
    LANES_END
#endif
}
#if BMPC_NW > 1
// Teams: the dZ rows of ALL stages in one wide pass behind the forward sweep (items (stage, component): 44 N over 64 NW lanes), from the
// reduced states the sweep left in L_DSA and the LDS-resident workspace rows (kinematics records, lifted residuals, QP gradient).  In the
// one-wave program these rows ride in the sweep (a phase of 44 lanes per stage); here the sweep's wave does the recursion only.  Every lane
// keeps its share of (QP gradient) . dZ in a register for row pass B (same lane there).
BMPC_D inline void wave_dz_wide(Wave &W, const Scr &sc, LaneRegs *LR) {
    const int N = W.N;
    double *L = W.L; const LPtr WL = BMPC_WL(W);
    WIDE_BEGIN
        double ghd = 0.0;
        for (int t_ = 0; t_ < (N * NZ + WS - 1) / WS; t_++) {      // wave-uniform trip count, clamped item (duplicate store of the same value)
            const int id0 = wl + WS * t_, id = id0 < N * NZ ? id0 : N * NZ - 1, k = id / NZ, t = id - k * NZ;
            const double g_ = forward_dz_item(W, k, t, L + L_DSA + k * 36, WL + sc.RLV + k * 12, WL + sc.KIN + k * KREC, WL + sc.GH + k * NZ, true, (const double *)nullptr);
            ghd += id0 < N * NZ ? g_ : 0.0;
        }
        LR[LIDXW].ghd = ghd;
    WIDE_END
}
#endif

// The Riccati sweep: one wave's in the one-wave program; in a team wave 0 runs the recursion, wave 1 the recursion-independent half of every
// stage's node-cost add beside it, and all waves hear the verdict (positive definite or not) through an LDS word behind the stage's barrier.
BMPC_D inline bool team_backward(Wave &W, const POff &po, const Scr &sc, double mu, double delta, LaneRegs *LR) {
    // (every wave of a team runs the sweep function: wave 0 the recursion, wave 1 the helper's half, all of them its barriers and verdict)
    const bool ok_ = wave_backward_blk(W, po, sc, mu, delta, LR);
    TEAM_SYNC();
    return ok_;
}

// ----------------------------------------------------------------------------------------
// main driver for one problem
// ----------------------------------------------------------------------------------------
// ZLDS: the iterate / trial iterate / direction live in LDS (horizons N <= 11); a compile-time switch so that the compiler
// knows the address space of every access (a run-time select would degrade them to FLAT instructions).
// RT: real-time instantiation (closed-loop ticks): the iteration loop also ends -- status 1, like the iteration cap -- once the wall clock
// has passed W.deadline (bmpc_stream_set_time_budget): every stream gets the iterations that fit the tick instead of the same fixed number,
// and the tick is bounded whatever a stream's Riccati retries or line-search trials cost.  Not part of the batch solver kernels.
#ifndef BMPC_NOW
#define BMPC_NOW() 0LL
#endif
// RESTO: this instantiation carries the restoration phase (oracle/bmpc_oracle.c solve_one).  The batch kernels are compiled WITHOUT it (the elastic
// row code costs the hot path 6 % through register allocation alone, measured): a problem whose main phase is jammed or stalled leaves them with
// the internal status 4 and its iterate in x, and a second kernel (bmpc_resto_kernel, RESTO = true, started by the library right behind) picks it
// up via Problem::resto_from -- entering the restoration phase discards everything but the iterate, so the hand-over loses nothing and both
// paths compute the same numbers.  The fused closed-loop ticks carry the phase in the kernel (their post-processing needs the final solution).
template <bool ZLDS, bool RT = false, bool RESTO = false>
BMPC_D inline void wave_solve(Wave &W, const Problem &pr) {
    const int N = W.N, S = W.S;
    double *L = W.L; const GPtr G = W.G; const LPtr WL = BMPC_WL(W);
    const POff po = make_poff_lds(S, L_ZL);      // LDS-relative (S > 4: the tail of p sits in the free iterate area, ZLDS is false then)
    Scr sc = make_scr(N);
    const Opts &o = W.o;
    const int np = po.size, nw = N * NZ, ni = N * NI, ne = N * NE;
    BMPC_LANE_REGS(LRs);
    constexpr bool zlds = ZLDS;
    const bool longh = !ZLDS && N > 11;      // long-horizon rules of the algorithm (oracle/bmpc_oracle.c): the instantiation without the LDS iterate also serves S > 4 at short horizons
    // (the lines of wave_load_point, its twin, kept here: calling it changes this function's compiled code -- profiles/point_maps_refactor.txt)
    if (ZLDS) { W.Zc = L + L_ZL; W.Zt = L + L_PB; W.Dz = L + L_PB + 512; } else { W.Zc = (G + sc.Z).ptr(); W.Zt = (G + sc.ZT).ptr(); W.Dz = (G + sc.DZ).ptr(); }
    WIDE_BEGIN
        for (int id = wl; id < np; id += WS) L[L_PAR + (ZLDS ? id : lds_index_of_p(S, id, L_ZL))] = pr.p[id];
        for (int id = wl; id < nw; id += WS) W.Zc[id] = pr.x0[id];
    WIDE_END
    wave_init_tables(W, po);
    const double *PAR = L + L_PAR;
    // the integrator chains of the iterate rolled out from node 0 with the iterate's own jerks (oracle/bmpc_oracle.c rollout_chains): one lane per
    // chain (7 joints + the path parameter); the evaluation that follows projects the lifted variables
#define BMPC_ROLLOUT() \
            SOLO_BEGIN(0) \
            LANES_BEGIN \
                if (lane < 8) { \
                    const double h_ = W.h, h2_ = h_ * h_, h3_ = h2_ * h_; \
                    const int zx = lane < 7 ? ZQ + lane : ZPHI, zd = lane < 7 ? ZDQ + lane : ZDPHI, za = lane < 7 ? ZDDQ + lane : ZDDPHI, zj = lane < 7 ? ZJ + lane : ZJPHI; \
                    const int px = lane < 7 ? po.q0 + lane : po.phi0, pd = lane < 7 ? po.dq0 + lane : po.phi0 + 1, pa = lane < 7 ? po.ddq0 + lane : po.phi0 + 2, pj = lane < 7 ? po.jerk + lane : po.jerkphi; \
                    for (int k = 0; k < N; k++) { \
                        const double x_ = ndv(PAR, po, W.Zc, k, zx, px), d_ = ndv(PAR, po, W.Zc, k, zd, pd), a_ = ndv(PAR, po, W.Zc, k, za, pa), j0_ = ndv(PAR, po, W.Zc, k, zj, pj); \
                        double *Zn_ = W.Zc + k * NZ; const double j1_ = Zn_[zj]; \
                        Zn_[zx] = x_ + h_ * d_ + h2_ / 2 * a_ + h3_ / 8 * j0_ + h3_ / 24 * j1_; \
                        Zn_[zd] = d_ + h_ * a_ + h2_ / 3 * j0_ + h2_ / 6 * j1_; \
                        Zn_[za] = a_ + h_ / 2 * (j0_ + j1_); \
                    } \
                } \
            LANES_END \
            SOLO_END \
            TEAM_SYNC();
    // warm start (oracle/bmpc_oracle.c solve_one): barrier restarts at clamp(stored mu, mu_warm, mu_init); the stored
    // multiplier of a row bounds its initial slack from below by mu/nu, so active rows keep their multiplier
    const double mu_state = pr.state ? pr.state[ni] : 0.0;
    const bool warm = mu_state > 0.0;
    double mu = warm ? BMPC_FMIN(o.mu_init, BMPC_FMAX(mu_state, o.mu_warm)) : o.mu_init; const double mu_min = o.tol * o.mu_min_fac;
    const double mu_entry = mu;      // (hold_mu: the level of the main phase; the restoration phase walks its own barrier down and hands this level back)
    double delta_last = 0.0, delta_prev = 0.0, filt_mu = -1.0, theta_min = -1.0, theta_max = 0.0; int nfilt = 0, gn_run = 0;
    // A cold start that is not a trajectory (oracle/bmpc_oracle.c solve_one: a residual of the integrator chains of x0 above START_ROLLOUT_TOL -- noise,
    // zeros, the plan of another problem) is made one first: the chains rolled out with x0's own jerks, the lifted variables projected by the first
    // evaluation.  Solves that carry a dual state (the ticks of a closed loop -- also the cold one behind a failed restoration --, the drop-in shim) and
    // continued solves are not touched.
    bool roll0_ = false;
    if (!pr.state && o.start_rollout && o.max_iter > 0 && !(RESTO && pr.resto_from >= 0)) {      // stateless solves only; (max_iter = 0 is the evaluation of f, g AT x0)
        WIDE_BEGIN
            double gm_ = 0;
            const double h_ = W.h, h2_ = h_ * h_, h3_ = h2_ * h_;
            for (int t_ = 0; t_ < (N * 8 + WS - 1) / WS; t_++) {      // items (node, chain); wave-uniform trip count, clamped item
                const int id0 = wl + WS * t_, id = id0 < N * 8 ? id0 : N * 8 - 1, k = id >> 3, c = id & 7;
                const int zx = c < 7 ? ZQ + c : ZPHI, zd = c < 7 ? ZDQ + c : ZDPHI, za = c < 7 ? ZDDQ + c : ZDDPHI, zj = c < 7 ? ZJ + c : ZJPHI;
                const int px = c < 7 ? po.q0 + c : po.phi0, pd = c < 7 ? po.dq0 + c : po.phi0 + 1, pa = c < 7 ? po.ddq0 + c : po.phi0 + 2, pj = c < 7 ? po.jerk + c : po.jerkphi;
                const double x_ = ndv(PAR, po, W.Zc, k, zx, px), d_ = ndv(PAR, po, W.Zc, k, zd, pd), a_ = ndv(PAR, po, W.Zc, k, za, pa), j0_ = ndv(PAR, po, W.Zc, k, zj, pj);
                const double *Zn_ = W.Zc + k * NZ; const double j1_ = Zn_[zj];
                const double r0_ = BMPC_FABS(x_ + h_ * d_ + h2_ / 2 * a_ + h3_ / 8 * j0_ + h3_ / 24 * j1_ - Zn_[zx]);
                const double r1_ = BMPC_FABS(d_ + h_ * a_ + h2_ / 3 * j0_ + h2_ / 6 * j1_ - Zn_[zd]), r2_ = BMPC_FABS(a_ + h_ / 2 * (j0_ + j1_) - Zn_[za]);
                gm_ = r0_ > gm_ ? r0_ : gm_; gm_ = r1_ > gm_ ? r1_ : gm_; gm_ = r2_ > gm_ ? r2_ : gm_;
            }
            WRED_PUT_MAX(L_REDW, 4, gm_);
        WIDE_END
        roll0_ = WRED_GET_MAX(L_REDW, 4) > START_ROLLOUT_TOL;
        TEAM_SYNC();
        if (roll0_) { BMPC_ROLLOUT() }
    }
    BMPC_PROF(W, 15);
    double fval = wave_eval(W, po, sc, W.Zc, sc.G, sc.HIN, roll0_);
    BMPC_PROF(W, 0);
    // Row pass "A" (57 rows per node, lane-strided, three rows in flight per lane): multipliers nu, barrier ratios
    // sigma = nu/t, 1/t, sigma*(h+t), and the inequality part of the KKT error.  first = initialisation of t, nu.
    double ad = 1.0;
    // Row pass "A0": slacks and multipliers from the inequality values -- at the start of the solve (warm: slack bounded from below by
    // the stored multiplier) and again at every barrier restart of a stalled long-horizon solve (re-centred on a high barrier level).
#define BMPC_ROWS_INIT(WARM_, PUSH_) \
        WIDE_BEGIN \
            double ep = 0, cmax = -1e300, cmin = 1e300, sn = 0; \
            for (int tr_ = 0; tr_ < (ni + WS * RUW - 1) / (WS * RUW); tr_++) { const int base = wl + tr_ * WS * RUW;      /* wave-uniform trip count */ \
                double hv[RUW], tv[RUW]; \
_Pragma("unroll") \
                for (int u = 0; u < RUW; u++) { \
                    const int id = base + WS * u; hv[u] = id < ni ? WL[sc.HIN + id] : -1.0; \
                    const double ns = ((WARM_) && id < ni) ? pr.state[id] : 0.0; \
                    tv[u] = ns > 0.0 ? BMPC_FMIN(mu / ns, (PUSH_)) : (PUSH_); \
                } \
_Pragma("unroll") \
                for (int u = 0; u < RUW; u++) { \
                    const int id = base + WS * u; \
                    if (id < ni) { \
                        const double t = (-hv[u] > tv[u]) ? -hv[u] : tv[u], ti = 1.0 / t, nu = mu * ti, r = hv[u] + t; \
                        WL[sc.T + id] = t; WL[sc.NUm + id] = nu; WL[sc.SG + id] = nu * ti; WL[sc.TI + id] = ti; WL[sc.SR + id] = nu * ti * r; \
                        const double v = BMPC_FABS(r), c = nu * t; \
                        ep = v > ep ? v : ep; cmax = c > cmax ? c : cmax; cmin = c < cmin ? c : cmin; sn += nu; \
                    } \
                } \
            } \
            WRED_PUT_MAX(L_KKPW, 0, ep); WRED_PUT_MAX(L_KKPW, 1, cmax); WRED_PUT_MIN(L_KKPW, 2, cmin); WRED_PUT_SUM(L_KKPW, 3, sn); \
        WIDE_END
    BMPC_ROWS_INIT(warm, o.slack_push)
    // Restoration phase (oracle/bmpc_oracle.c solve_one): elastic rows h + t - e = 0 with nu t = mu, (rho - nu) e = mu.  Row pass "A0e": the
    // centred start of every row at the barrier level mu (elastic_centre of the oracle), and what the Newton system reads from a row:
    // SG = sigma = 1 / (t/nu + e/z), and the barrier-modified multiplier nu^ = nu + sigma (h + mu/nu - mu/z) split as SR + mu * TI with
    // SR = nu + sigma h, TI = sigma (1/nu - 1/z), so that the consumers (mu * TI + SR) follow a barrier update between this pass and the system.
#define BMPC_ROWS_CENTRE() \
        WIDE_BEGIN \
            double ep = 0, cmax = -1e300, cmin = 1e300, sn = 0, hm = -1e300; \
            for (int tr_ = 0; tr_ < (ni + WS * RUW - 1) / (WS * RUW); tr_++) { const int base = wl + tr_ * WS * RUW; \
                double hv[RUW]; \
_Pragma("unroll") \
                for (int u = 0; u < RUW; u++) { const int id = base + WS * u; hv[u] = id < ni ? WL[sc.HIN + id] : -1.0; } \
_Pragma("unroll") \
                for (int u = 0; u < RUW; u++) { \
                    const int id = base + WS * u; \
                    if (id < ni) { \
                        const double hh = hv[u], nu = 2.0 * mu * RESTO_RHO / (2.0 * mu - hh * RESTO_RHO + BMPC_SQRT(4.0 * mu * mu + hh * hh * RESTO_RHO * RESTO_RHO)); \
                        const double z = RESTO_RHO - nu, t = mu / nu, e = mu / z, sgm = 1.0 / (t / nu + e / z); \
                        WL[sc.T + id] = t; WL[sc.NUm + id] = nu; G[sc.E + id] = e; WL[sc.SG + id] = sgm; WL[sc.TI + id] = sgm * (1.0 / nu - 1.0 / z); WL[sc.SR + id] = nu + sgm * hh; \
                        const double v = BMPC_FABS(hh + t - e), c = nu * t, c2 = z * e; \
                        ep = v > ep ? v : ep; cmax = c > cmax ? c : cmax; cmin = c < cmin ? c : cmin; cmax = c2 > cmax ? c2 : cmax; cmin = c2 < cmin ? c2 : cmin; sn += nu; hm = hh > hm ? hh : hm; \
                    } \
                } \
            } \
            WRED_PUT_MAX(L_KKPW, 0, ep); WRED_PUT_MAX(L_KKPW, 1, cmax); WRED_PUT_MIN(L_KKPW, 2, cmin); WRED_PUT_SUM(L_KKPW, 3, sn); WRED_PUT_MAX(L_KKPW, 4, hm); \
        WIDE_END
    // the objective weights in the LDS copy of p: zero inside the restoration phase, from p again behind it (ca, cb: wave_init_tables)
#define BMPC_WEIGHTS(ZERO_) \
        WIDE_BEGIN \
            const double wv_ = pr.p[make_poff(S).w + (wl < 15 ? wl : 14)];      /* (unconditional load on a clamped index) */ \
            if (wl < 15) L[L_PAR + po.w + wl] = (ZERO_) ? 0.0 : wv_; \
        WIDE_END \
        W.ca = 2 * L[L_PAR + po.w + 5] / (W.h * W.h); W.cb = 2 * L[L_PAR + po.w + 5] / W.h;
    // into the restoration phase: objective weights zero (the records carry weight-dependent Hessian entries: rebuilt by an evaluation, which
    // returns f = 0), every row elastic and centred on the level RESTO_MU, filter and inertia history cleared
    // An iterate that is far off its dynamics (a bad warm start: an equality residual above RESTO_ROLLOUT_TOL) is first made dynamically consistent:
    // one lane per integrator chain (7 joints + the path parameter) rolls q, dq, ddq / phi, dphi, ddphi of every node out from node 0 with the
    // iterate's own jerks (oracle/bmpc_oracle.c rollout_chains), and the evaluation that follows projects the lifted variables.
#define BMPC_ENTER_RESTO() \
        n_resto++; it_resto = it; el = true; mu = RESTO_MU; \
        BMPC_WEIGHTS(true) \
        WIDE_BEGIN \
            double gm_ = 0; \
            for (int t_ = 0; t_ < (ne + WS - 1) / WS; t_++) { const int id0 = wl + WS * t_, id = id0 < ne ? id0 : ne - 1; const double v_ = BMPC_FABS(WL[sc.G + id]); gm_ = v_ > gm_ ? v_ : gm_; } \
            WRED_PUT_MAX(L_REDW, 4, gm_); \
        WIDE_END \
        const bool roll_ = WRED_GET_MAX(L_REDW, 4) > RESTO_ROLLOUT_TOL; \
        TEAM_SYNC(); \
        if (roll_) { BMPC_ROLLOUT() } \
        fval = wave_eval(W, po, sc, W.Zc, sc.G, sc.HIN, roll_); \
        BMPC_ROWS_CENTRE() \
        nfilt = 0; filt_mu = -1.0; theta_min = -1.0; delta_last = 0.0; delta_prev = 0.0; gn_run = 0; n_short = 0;
    int n_restart = 0, it_restart = 0, n_resto = 0, it_resto = 0, n_short = 0; bool el = false;      // el: inside the restoration phase
    int it = 0, status = 1; double E0 = 0, ep_old = 0, ep_mid = 0;
    if (RESTO && pr.resto_from >= 0) {      // continuation of a solve whose main phase jammed in a kernel without the restoration phase
        it = pr.resto_from & 0xfffff; n_restart = pr.resto_from >> 20; ep_old = ep_mid = 1e300;      // (the hand-over carries the restart count of a long horizon)
        BMPC_ENTER_RESTO()
        it++;
    }
    for (; it <= o.max_iter; it++) {
        BMPC_PROF(W, 10);
        wave_adjoint(W, po, sc, sc.NUm, false, 0.0, LRs);
        BMPC_PROF(W, 1);
        // ---- KKT error (Ipopt-style scaling), deterministic reductions; the inequality part comes from row pass A ----
        WIDE_BEGIN
#if BMPC_NW > 1
            double ed = 0, ep = 0, sl = 0, g1 = 0, gm = 0;      // (the row pass's share of the primal infeasibility joins behind the barrier)
#else
            double ed = 0, ep = L[L_KKPW + wl], sl = 0, g1 = 0, gm = 0;
#endif
            // the jerk-gradient entries ride in the first batch of the residual rows (one round trip to the workspace for the whole pass;
            // clamped duplicates do not change a maximum)
            const int nrj = N * NU;
            for (int tr_ = 0; tr_ < (ne + WS * RUW - 1) / (WS * RUW); tr_++) { const int base = wl + tr_ * WS * RUW;      /* wave-uniform trip count */
                double gv[RUW], lv[RUW], rj[RUW];
#pragma unroll
                for (int u = 0; u < RUW; u++) { const int id0 = base + WS * u, id = id0 < ne ? id0 : ne - 1; gv[u] = WL[sc.G + id]; lv[u] = WL[sc.LAM + id];
                                               rj[u] = WL[sc.RJ + (id0 < nrj ? id0 : nrj - 1)]; }
#pragma unroll
                for (int u = 0; u < RUW; u++) { const double v = BMPC_FABS(rj[u]); ed = v > ed ? v : ed; }
#pragma unroll
                for (int u = 0; u < RUW; u++) { const bool ok_ = base + WS * u < ne; const double v = ok_ ? BMPC_FABS(gv[u]) : 0.0; ep = v > ep ? v : ep; gm = v > gm ? v : gm; g1 += v; sl += ok_ ? BMPC_FABS(lv[u]) : 0.0; }
            }
            WRED_PUT_MAX(L_REDW, 0, ed); WRED_PUT_MAX(L_REDW, 1, ep); WRED_PUT_SUM(L_REDW, 2, sl); WRED_PUT_SUM(L_REDW, 3, g1);
            if (RESTO && el) { WRED_PUT_MAX(L_REDW, 4, gm); }      // restoration phase: the largest equality residual on its own (wave-uniform)
        WIDE_END
        const double theta_eq = WRED_GET_SUM(L_REDW, 3);      // ||c||_1 of the current iterate, for the filter's theta (row pass B)
#if BMPC_NW > 1
        const double ep = BMPC_FMAX(WRED_GET_MAX(L_REDW, 1), WRED_GET_MAX(L_KKPW, 0));
#else
        const double ep = WRED_GET_MAX(L_REDW, 1);
#endif
        const double ed = WRED_GET_MAX(L_REDW, 0), cmax = WRED_GET_MAX(L_KKPW, 1), cmin = WRED_GET_MIN(L_KKPW, 2),
                     sl = WRED_GET_SUM(L_REDW, 2), sn = WRED_GET_SUM(L_KKPW, 3);
        double hmax = 0.0, gmax = 0.0;
        if (RESTO && el) { hmax = WRED_GET_MAX(L_KKPW, 4); gmax = WRED_GET_MAX(L_REDW, 4); }
        TEAM_SYNC();      // (teams: every wave has read the partials before a barrier restart below, or the next pass, rewrites them)
        const double sd = BMPC_FMAX(100.0, (sl + sn) / (N * (NE + NI))) / 100.0, scl = BMPC_FMAX(100.0, sn / (N * NI)) / 100.0;
        E0 = BMPC_FMAX(BMPC_FMAX(ed / sd, ep), BMPC_FMAX(cmax, -cmin) / scl);
#ifdef BMPC_EMU
        if (o.verbose) fprintf(stderr, "it %3d f %.8e dual %.2e prim %.2e compl %.2e mu %.1e\n", it, fval, ed, ep, BMPC_FMAX(cmax, -cmin), mu);
#endif
        if (!(RESTO && el)) { if (E0 <= o.tol) { status = 0; break; } }
        else {      // restoration phase: back to the main phase from a feasible point, locally infeasible (status 2), or go on (oracle/bmpc_oracle.c solve_one)
            const double vmax = BMPC_FMAX(hmax, gmax), rtol = BMPC_FMAX(BMPC_FMAX(o.tol, 1e-6), RESTO_REL * RESTO_RHO * vmax);
            const bool back = (hmax <= -RESTO_MARGIN && gmax <= RESTO_GTOL) || (E0 <= rtol && vmax <= 1e-6);
            if (!back && (E0 <= rtol || it - it_resto >= o.resto_cap)) { status = 2; break; }
            if (back) {
                el = false; mu = o.hold_mu ? mu_entry : RESTO_MU_BACK;
                BMPC_WEIGHTS(false)
                fval = wave_eval(W, po, sc, W.Zc, sc.G, sc.HIN, false);      // the objective of the original problem (and the records with its weights)
                BMPC_ROWS_INIT(false, RESTO_PUSH_BACK)
                nfilt = 0; filt_mu = -1.0; theta_min = -1.0; delta_last = 0.0; delta_prev = 0.0; gn_run = 0; n_short = 0;
                ep_old = ep_mid = 1e300; it_restart = it;
                continue;
            }
        }
        if (it == o.max_iter) break;
        if (RT && W.deadline) {      // real-time tick: out of time (teams: one lane reads the clock, every wave hears the verdict behind a barrier)
#if BMPC_NW > 1
            LANES_BEGIN
                if (lane == 0 && W.wv == 0) L[L_TFLAG + 4] = BMPC_NOW() > W.deadline ? 1.0 : 0.0;
            LANES_END
            TEAM_SYNC_LDS();
            const bool late_ = L[L_TFLAG + 4] != 0.0;
            TEAM_SYNC_LDS();
            if (late_) break;
#else
            if (BMPC_NOW() > W.deadline) break;
#endif
        }
        // stalled primal feasibility -> status 2, numerical breakdown -> status 3 (oracle/bmpc_oracle.c solve_one)
        if (it == 0) ep_old = ep_mid = 1e300;
        if (!(RESTO && el)) {
            // (the floor of the tests scales with the tolerance: a solve that is asked for 1e-5 and sits at 1e-5 is converging, not stalled)
            const bool open_ = ep > BMPC_FMAX(1e-6, 10.0 * o.tol);
            const bool at_check = it > 0 && o.stall_window > 0 && (it - it_restart) % (o.stall_window / 2) == 0;
            const bool stalled = at_check && it >= o.stall_window + it_restart && ep >= STALL_FACTOR * ep_old && open_;
            // a dual residual beyond 1e12 is a numerical breakdown of the main phase: with the restoration phase available the solve goes there (the
            // rollout and the re-centred rows discard what broke) instead of ending as status 3
            const bool broken = !(ed < 1e12) && o.restoration > 0;
            // long horizons: barrier restarts come first (below), the restoration phase is the last resort behind them and is not entered on a jam
            const bool jammed = o.restoration == 1 && !longh && o.resto_short > 0 && n_short >= o.resto_short && open_;
            if (stalled || jammed || broken) {
                if (broken || (o.restoration == 1 && (!longh || n_restart >= STALL_RESTARTS))) {
                    if (n_resto >= RESTO_MAX) { status = 2; break; }
                    if (!RESTO) { status = 4; break; }      // (internal) this kernel does not carry the phase: the restoration kernel continues from x
                    BMPC_ENTER_RESTO()
                    continue;
                }
                // Long horizons (a compile-time property of this instantiation, like the Gauss-Newton fallback) without the restoration phase:
                // before giving up, restart the barrier from the CURRENT iterate -- slacks and multipliers re-centred on a high barrier level,
                // filter and inertia history cleared -- at most STALL_RESTARTS times (oracle/bmpc_oracle.c solve_one has the numbers: the
                // stalled problems of the tight 30-stage batch are feasible, their iterate is jammed at the first barrier level).
                if (!longh || n_restart >= ((o.retry_cap > 0 && n_resto == 0 && !(RESTO && pr.resto_from >= 0)) ? STALL_RESTARTS_RETRY : STALL_RESTARTS)) { status = 2; break; }
                n_restart++; it_restart = it;
                mu = STALL_RESTART_MU;
                BMPC_ROWS_INIT(false, STALL_RESTART_PUSH)
                nfilt = 0; filt_mu = -1.0; theta_min = -1.0; delta_last = 0.0; delta_prev = 0.0; gn_run = 0;
                ep_old = ep_mid = 1e300;
                continue;
            }
            if (at_check) { ep_old = ep_mid; ep_mid = ep; }
        }
        if (!(ed < 1e12)) { status = 3; break; }
        for (;;) {   // monotone barrier update (Fiacco-McCormick, Ipopt constants)
            const double ec = BMPC_FMAX(cmax - mu, mu - cmin);
            const double Emu = BMPC_FMAX(BMPC_FMAX(ed / sd, ep), ec / scl);
            if (!(o.hold_mu && !(RESTO && el)) && Emu <= KAPPA_EPS * mu && mu > mu_min) mu = BMPC_FMAX(mu_min, BMPC_FMIN(0.2 * mu, BMPC_POW15(mu))); else break;
        }
        // ---- Newton system: QP gradient, lifted residuals, Riccati ----
        BMPC_PROF(W, 2);
        wave_adjoint(W, po, sc, sc.NUm, true, mu, LRs);
        BMPC_PROF(W, 3);
        wave_stage_data_wide(W, po, sc);
        BMPC_PROF(W, 4);
        // Inertia control (oracle/bmpc_oracle.c solve_one).  A failed factorisation costs most of a Riccati sweep (the indefinite
        // 8x8 block usually shows up at the first stages, the END of the backward sweep), so the attempts are chosen to fail rarely:
        // an iteration that follows a regularised one starts from a third of its delta instead of 0; while the Gauss-Newton
        // fallback (first barrier level, long horizons) keeps being needed, the following iterations start from the Gauss-Newton
        // Hessian directly and only every GN_PROBE-th tries the exact one again.
        double delta = 0.0; bool ok = false, used_gn = false; const int ex_saved = W.o.exact_hessian;
        if (delta_prev > 0.0) { delta = delta_prev / 3.0; if (delta < DELTA_KEEP_MIN) delta = 0.0; }
        // The node records carry the exact-Hessian entries, so for the Gauss-Newton matrix they are rebuilt with the flag off (same
        // f, g, h); the flag stays off until the factorisation of this iteration has succeeded, the next evaluation restores the
        // exact entries.  Long horizons only (N > 11 <=> !ZLDS, a compile-time property of this instantiation): the short-horizon
        // kernel never met the case on any test batch, and carrying the extra path there costs registers (scratch 44 -> 312 B/lane).
        const bool gn_allowed = longh && ex_saved && mu >= GN_MU_GATE;
        if (gn_allowed && gn_run > 0 && gn_run % GN_PROBE != GN_PROBE - 1) {
            used_gn = true; W.o.exact_hessian = 0;
            wave_eval(W, po, sc, W.Zc, sc.G, sc.HIN, false);
            wave_stage_data_wide(W, po, sc);
        }
        for (int tries = 0; tries < 40; tries++) {
            if (team_backward(W, po, sc, mu, delta, LRs)) { ok = true; break; }
            if (gn_allowed && !used_gn) {
                used_gn = true; W.o.exact_hessian = 0;
                wave_eval(W, po, sc, W.Zc, sc.G, sc.HIN, false);
                wave_stage_data_wide(W, po, sc);
                if (team_backward(W, po, sc, mu, 0.0, LRs)) { ok = true; delta = 0.0; break; }
            }
            if (delta == 0.0) delta = delta_last > 0 ? BMPC_FMAX(1e-20, delta_last / 3.0) : DELTA_FIRST;
            else delta *= (delta_last > 0 ? 8.0 : DELTA_UP_FIRST);
            if (delta > 1e20) break;
        }
        gn_run = (used_gn && ok) ? gn_run + 1 : 0;
        W.o.exact_hessian = ex_saved;
        if (!ok) { status = 3; break; }
        if (delta > 0) delta_last = delta;
        delta_prev = delta;
        BMPC_PROF(W, 6);
        SOLO_BEGIN(0)
        wave_forward(W, sc, LRs);
        SOLO_END
        TEAM_SYNC();
#if BMPC_NW > 1
        wave_dz_wide(W, sc, LRs);
#endif
        BMPC_PROF(W, 7);
        // ---- row pass "B": slack / multiplier directions, fraction to the boundary, merit ingredients ----
        const double tau = BMPC_FMAX(0.99, 1.0 - mu);
        WIDE_BEGIN
            double ap = 1.0, adl = 1.0, dbar = 0, nhd = 0, th = 0, bar = 0, pn_ = 1.0, pd_ = 0.0, dn_ = 1.0, dd_ = 0.0;
            for (int tr_ = 0; tr_ < (ni + WS * RUW - 1) / (WS * RUW); tr_++) { const int base = wl + tr_ * WS * RUW;      /* wave-uniform trip count */
                double tv[RUW], nv[RUW], hv[RUW], sg[RUW], tiv[RUW], sr[RUW], hd[RUW], tprod = 1.0;
#pragma unroll
                for (int u = 0; u < RUW; u++) {   // rows past the end are clamped to the last row (branch-free); their contributions are masked below
                    const int id0 = base + WS * u, id = id0 < ni ? id0 : ni - 1;
                    tv[u] = WL[sc.T + id]; nv[u] = WL[sc.NUm + id]; hv[u] = WL[sc.HIN + id];
                    sg[u] = WL[sc.SG + id]; tiv[u] = WL[sc.TI + id]; sr[u] = WL[sc.SR + id];
                }
                {   // hd = grad h_i . dZ with the loads of the whole batch in front (see ineq_dir for the row formulas)
                    double c0[RUW], c1[RUW], c2[RUW], c3[RUW], w1[RUW], d0[RUW], d1[RUW], d2[RUW], dph[RUW];
#pragma unroll
                    for (int u = 0; u < RUW; u++) {
                        const int id0 = base + WS * u, id = id0 < ni ? id0 : ni - 1;
                        const int k = id / NI, i = id - k * NI;
                        // box rows and tube rows run the same instructions: clamped indices, unconditional loads, 0/1 factors (a select
                        // between loaded values would put the loads under an exec-mask branch)
                        const bool tube = i >= ITUBE; const int m = tube ? (i - ITUBE) >> 1 : 0, ti = tube ? 1 : 0; const double mt = tube ? 1.0 : 0.0;
                        const double sgn = L[L_ROWT + i]; const int src = (int)L[L_ROWT + 2 * NI + i];
                        const LPtr rr = WL + sc.REF + k * RREC; const double *dz = W.Dz + k * NZ;
                        const int vo = src + ti * (tube_voff(m) - src);
                        c0[u] = mt * rr[RGC + m * 4 + 0] + (1.0 - mt) * sgn; c1[u] = mt * rr[RGC + m * 4 + 1]; c2[u] = mt * rr[RGC + m * 4 + 2];
                        c3[u] = mt * rr[RGC + m * 4 + 3]; w1[u] = mt * rr[RW1 + m];
                        d0[u] = dz[vo]; d1[u] = dz[vo + ti]; d2[u] = dz[vo + 2 * ti]; dph[u] = dz[ZPHI];
                    }
#pragma unroll
                    for (int u = 0; u < RUW; u++) {
                        const int id0 = base + WS * u, id = id0 < ni ? id0 : ni - 1; const int i = id % NI;
                        const double sv = c0[u] * d0[u] + c1[u] * d1[u] + c2[u] * d2[u] + c3[u] * dph[u];
                        hd[u] = ((i >= ITUBE && ((i - ITUBE) & 1)) ? -1.0 : 1.0) * sv - w1[u] * dph[u];
                    }
                }
                if (RESTO && el) {      // restoration phase (wave-uniform): elastic rows, oracle/bmpc_oracle.c solve_one
                    double ev[RUW], eprod = 1.0;
#pragma unroll
                    for (int u = 0; u < RUW; u++) { const int id0 = base + WS * u, id = id0 < ni ? id0 : ni - 1; ev[u] = G[sc.E + id]; }
#pragma unroll
                    for (int u = 0; u < RUW; u++) {
                        const int id0 = base + WS * u; const bool ok_ = id0 < ni; const int id = ok_ ? id0 : ni - 1;
                        const double t = tv[u], nu = nv[u], e = ev[u], z = RESTO_RHO - nu, nuh = mu * tiv[u] + sr[u];
                        const double dnu = nuh - nu + sg[u] * hd[u], dt = mu / nu - t - t / nu * dnu, de = mu / z - e + e / z * dnu;
                        WL[sc.DT + id] = dt; G[sc.DNU + id] = dnu; G[sc.DE + id] = de;
                        const bool c1 = ok_ && dt < 0 && t * pd_ < pn_ * -dt;
                        pn_ = c1 ? t : pn_; pd_ = c1 ? -dt : pd_;
                        const bool c1e = ok_ && de < 0 && e * pd_ < pn_ * -de;
                        pn_ = c1e ? e : pn_; pd_ = c1e ? -de : pd_;
                        const bool c2 = ok_ && dnu < 0 && nu * dd_ < dn_ * -dnu;
                        dn_ = c2 ? nu : dn_; dd_ = c2 ? -dnu : dd_;
                        const bool c2z = ok_ && dnu > 0 && z * dd_ < dn_ * dnu;
                        dn_ = c2z ? z : dn_; dd_ = c2z ? dnu : dd_;
                        dbar += ok_ ? -mu * dt / t + (RESTO_RHO - mu / e) * de : 0.0; nhd += ok_ ? nuh * hd[u] : 0.0; th += ok_ ? BMPC_FABS(hv[u] + t - e) : 0.0;
                        tprod *= ok_ ? t : 1.0; eprod *= ok_ ? e : 1.0; bar += ok_ ? RESTO_RHO * e : 0.0;
                    }
                    bar -= mu * BMPC_LOG(eprod);
                } else {
#pragma unroll
                for (int u = 0; u < RUW; u++) {
                    const int id0 = base + WS * u; const bool ok_ = id0 < ni; const int id = ok_ ? id0 : ni - 1;
                    const double t = tv[u], nu = nv[u], r = hv[u] + t, mti = mu * tiv[u], nuh = mti + sr[u];
                    const double dt = -r - hd[u], dnu = mti - nu - sg[u] * dt;
                    WL[sc.DT + id] = dt; G[sc.DNU + id] = dnu;          // a clamped row rewrites the last row with the same values
                    // fraction to the boundary: the smallest ratio t/|dt| (nu/|dnu|) is tracked by cross-multiplication, one
                    // division per lane at the end instead of two per row
                    const bool c1 = ok_ && dt < 0 && t * pd_ < pn_ * -dt, c2 = ok_ && dnu < 0 && nu * dd_ < dn_ * -dnu;
                    pn_ = c1 ? t : pn_; pd_ = c1 ? -dt : pd_; dn_ = c2 ? nu : dn_; dd_ = c2 ? -dnu : dd_;
                    dbar += ok_ ? -mti * dt : 0.0; nhd += ok_ ? nuh * hd[u] : 0.0; th += ok_ ? BMPC_FABS(r) : 0.0; tprod *= ok_ ? t : 1.0;
                }
                }
                bar -= mu * BMPC_LOG(tprod);      // one log per batch of RU slacks: sum of logs = log of the product (t in [1e-12, 1e2])
            }
            if (pd_ > 0.0) { const double a = tau * pn_ / pd_; ap = a < ap ? a : ap; }
            if (dd_ > 0.0) { const double a = tau * dn_ / dd_; adl = a < adl ? a : adl; }
            BMPC_PROF(W, 28);
            // (QP gradient) . dZ was summed by the forward sweep (one entry per lane and stage), the 1-norm of the equality residuals by
            // the KKT pass at the top of the iteration: no further trip to the workspace here
                        const double ghd = LRs[LIDXW].ghd;      // (teams: the lane's own share from wave_dz_wide; same item lane)
            th += wl == 0 ? theta_eq : 0.0;
            BMPC_PROF(W, 29);
            WRED_PUT_MIN(L_REDW, 0, ap); WRED_PUT_MIN(L_REDW, 1, adl); WRED_PUT_SUM(L_REDW, 2, dbar); WRED_PUT_SUM(L_REDW, 3, ghd - nhd);
            WRED_PUT_SUM(L_REDW, 4, th); WRED_PUT_SUM(L_REDW, 5, bar);
        WIDE_END
        const double ap = WRED_GET_MIN(L_REDW, 0), dbar = WRED_GET_SUM(L_REDW, 2), gfd = WRED_GET_SUM(L_REDW, 3),
                     theta = WRED_GET_SUM(L_REDW, 4), bar = WRED_GET_SUM(L_REDW, 5);
        ad = WRED_GET_MIN(L_REDW, 1);
        TEAM_SYNC();
        BMPC_PROF(W, 8);
        // ---- filter line search (Waechter & Biegler 2006, Ipopt constants) on theta and phi = f - mu sum log t ----
        const double dphi = gfd + dbar, phi0 = fval + bar;
        if (mu != filt_mu) { nfilt = 0; filt_mu = mu; }
        if (theta_min < 0) { theta_min = 1e-4 * BMPC_FMAX(1.0, theta); theta_max = 1e4 * BMPC_FMAX(1.0, theta); }
        double alpha = ap, ft = 0; bool accepted = false, armijo_step = false;
        for (int ls = 0; ls < 14; ls++) {
            WIDE_BEGIN
                // wave-uniform trip count, clamped index (the lanes past the end rewrite the last entry with the same value)
                for (int t_ = 0; t_ < (nw + WS - 1) / WS; t_++) { const int id0 = wl + WS * t_, id = id0 < nw ? id0 : nw - 1; W.Zt[id] = W.Zc[id] + alpha * W.Dz[id]; }
            WIDE_END
            BMPC_PROF(W, 9);
            const LsRows lsr = {alpha, mu, RESTO && el};
            ft = wave_eval(W, po, sc, W.Zt, sc.GT, sc.HT, ls > 0 || (RESTO && el), &lsr);      // (restoration phase: every trial projected onto the lifted equalities)      // also: trial slacks -> TT, theta and barrier sums -> L_RED
            BMPC_PROF(W, 0);
            const double tht = WRED_GET_SUM(L_REDW, 1), phit = ft + WRED_GET_SUM(L_REDW, 2);
            bool okk = (phit - phit == 0.0) && tht <= theta_max;
            for (int j = 0; j < nfilt && okk; j++) if (!(tht < L[L_FILT + 2 * j] || phit < L[L_FILT + 2 * j + 1])) okk = false;
            armijo_step = false;
            if (okk) {
                if (theta <= theta_min && dphi < 0 && alpha * BMPC_POW(-dphi, 2.3) > BMPC_POW(theta, 1.1)) {
                    armijo_step = true;
                    okk = phit <= phi0 + 1e-8 * alpha * dphi + 1e-13 * BMPC_FABS(phi0);
                } else okk = (tht <= (1 - 1e-5) * theta) || (phit <= phi0 - 1e-8 * theta);
            }
            if (okk) { accepted = true; break; }
            if (ls > 0) alpha *= 0.5;     // trial 1 repeats the step length of trial 0 with the lifted variables projected
        }
#ifdef BMPC_EMU
        if (o.verbose) fprintf(stderr, "   alpha_p %.3e (max %.3e) alpha_d %.3e delta %.1e acc %d arm %d nfilt %d theta %.3e dphi %.3e\n", alpha, ap, ad, delta, (int)accepted, (int)armijo_step, nfilt, theta, dphi);
#endif
        n_short = alpha < RESTO_SHORT_ALPHA ? n_short + 1 : 0;      // jam detection (restoration phase)
        if (!accepted) nfilt = 0;          // smallest step taken, filter reset
        else if (!armijo_step && nfilt < 32) {
            LANES_BEGIN      // (teams: every wave writes the same two words)
                if (lane == 0) { L[L_FILT + 2 * nfilt] = (1 - 1e-5) * theta; L[L_FILT + 2 * nfilt + 1] = phi0 - 1e-8 * theta; }
            LANES_END
            nfilt++;
        }
        // accept the last trial: iterate (LDS copy or slab swap), slab swaps for t / g / h; then row pass "A" with the multiplier update
        if (zlds) {
            WIDE_BEGIN
                for (int t_ = 0; t_ < (nw + WS - 1) / WS; t_++) { const int id0 = wl + WS * t_, id = id0 < nw ? id0 : nw - 1; W.Zc[id] = W.Zt[id]; }
            WIDE_END
        } else { double *t_ = W.Zc; W.Zc = W.Zt; W.Zt = t_; }
        { int t_; t_ = sc.T; sc.T = sc.TT; sc.TT = t_; t_ = sc.G; sc.G = sc.GT; sc.GT = t_; t_ = sc.HIN; sc.HIN = sc.HT; sc.HT = t_; t_ = sc.E; sc.E = sc.ET; sc.ET = t_; }
        fval = ft;
        if (RESTO && el) {      // restoration phase: the same pass for elastic rows (see BMPC_ROWS_CENTRE for what it leaves to the Newton system)
        WIDE_BEGIN
            double ep = 0, cmax = -1e300, cmin = 1e300, sn = 0, hm = -1e300;
            for (int tr_ = 0; tr_ < (ni + WS * RUW - 1) / (WS * RUW); tr_++) { const int base = wl + tr_ * WS * RUW;
                double tv[RUW], nv[RUW], dv[RUW], hv[RUW], ev[RUW];
#pragma unroll
                for (int u = 0; u < RUW; u++) {
                    const int id0 = base + WS * u, id = id0 < ni ? id0 : ni - 1;
                    tv[u] = WL[sc.T + id]; nv[u] = WL[sc.NUm + id]; dv[u] = G[sc.DNU + id]; hv[u] = WL[sc.HIN + id]; ev[u] = G[sc.E + id];
                }
#pragma unroll
                for (int u = 0; u < RUW; u++) {
                    const int id = base + WS * u; const bool ok_ = id < ni;
                    const double t = tv[u], e = ev[u], ti = 1.0 / t; double nu = nv[u] + ad * dv[u];
                    const double lo = mu * ti * 1e-10, hi = 1e10 * mu * ti, hi2 = RESTO_RHO - mu / (1e10 * e);
                    nu = nu < lo ? lo : (nu > hi ? hi : nu); nu = nu > hi2 ? hi2 : nu;
                    const double z = RESTO_RHO - nu, sgm = 1.0 / (t / nu + e / z);
                    { const int ic = ok_ ? id : ni - 1; WL[sc.NU2 + ic] = nu; WL[sc.SG + ic] = sgm; WL[sc.TI + ic] = sgm * (1.0 / nu - 1.0 / z); WL[sc.SR + ic] = nu + sgm * hv[u]; }
                    const double v = ok_ ? BMPC_FABS(hv[u] + t - e) : 0.0, c = nu * t, c2 = z * e;
                    ep = v > ep ? v : ep; cmax = (ok_ && c > cmax) ? c : cmax; cmin = (ok_ && c < cmin) ? c : cmin; cmax = (ok_ && c2 > cmax) ? c2 : cmax; cmin = (ok_ && c2 < cmin) ? c2 : cmin;
                    sn += ok_ ? nu : 0.0; hm = (ok_ && hv[u] > hm) ? hv[u] : hm;
                }
            }
            WRED_PUT_MAX(L_KKPW, 0, ep); WRED_PUT_MAX(L_KKPW, 1, cmax); WRED_PUT_MIN(L_KKPW, 2, cmin); WRED_PUT_SUM(L_KKPW, 3, sn); WRED_PUT_MAX(L_KKPW, 4, hm);
        WIDE_END
        } else {
        WIDE_BEGIN
            double ep = 0, cmax = -1e300, cmin = 1e300, sn = 0;
            for (int tr_ = 0; tr_ < (ni + WS * RUW - 1) / (WS * RUW); tr_++) { const int base = wl + tr_ * WS * RUW;      /* wave-uniform trip count */
                double tv[RUW], nv[RUW], dv[RUW], hv[RUW];
#pragma unroll
                for (int u = 0; u < RUW; u++) {   // loads on clamped rows (branch-free)
                    const int id0 = base + WS * u, id = id0 < ni ? id0 : ni - 1;
                    tv[u] = WL[sc.T + id]; nv[u] = WL[sc.NUm + id]; dv[u] = G[sc.DNU + id]; hv[u] = WL[sc.HIN + id];
                }
#pragma unroll
                for (int u = 0; u < RUW; u++) {
                    const int id = base + WS * u; const bool ok_ = id < ni;
                    const double t = tv[u], ti = 1.0 / t; double nu = nv[u] + ad * dv[u];
                    const double lo = mu * ti * 1e-10, hi = 1e10 * mu * ti;
                    nu = nu < lo ? lo : (nu > hi ? hi : nu);
                    const double r = hv[u] + t, sgm = nu * ti;
                    // the new multipliers go to the OTHER buffer (ping-pong), so a clamped duplicate of the last row may store too
                    { const int ic = ok_ ? id : ni - 1; WL[sc.NU2 + ic] = nu; WL[sc.SG + ic] = sgm; WL[sc.TI + ic] = ti; WL[sc.SR + ic] = sgm * r; }
                    const double v = ok_ ? BMPC_FABS(r) : 0.0, c = nu * t;
                    ep = v > ep ? v : ep; cmax = (ok_ && c > cmax) ? c : cmax; cmin = (ok_ && c < cmin) ? c : cmin; sn += ok_ ? nu : 0.0;
                }
            }
            WRED_PUT_MAX(L_KKPW, 0, ep); WRED_PUT_MAX(L_KKPW, 1, cmax); WRED_PUT_MIN(L_KKPW, 2, cmin); WRED_PUT_SUM(L_KKPW, 3, sn);
        WIDE_END
        }
        { const int t_ = sc.NUm; sc.NUm = sc.NU2; sc.NU2 = t_; }
    }
    if (RESTO && el) {      // ended inside the restoration phase: the objective of the original problem at the final point
        BMPC_WEIGHTS(false)
        fval = wave_eval(W, po, sc, W.Zc, sc.G, sc.HIN, false);
    }
    // ---- outputs in the reference's conventions (casadi nlpsol: x, g, lam_g, lam_x, f) ----
    // (wave-uniform trip counts on clamped indices -- lanes past the end rewrite the last entry with the same value: a lane-dependent loop exit makes
    // the compiler restore the exec mask behind the loop, which is where this toolchain has placed register copies under the stale mask; build.py lint_isa)
    WIDE_BEGIN
        if (pr.x) for (int t_ = 0; t_ < (nw + WS - 1) / WS; t_++) { const int id0 = wl + WS * t_, id = id0 < nw ? id0 : nw - 1; pr.x[id] = W.Zc[id]; }
        for (int t_ = 0; t_ < (N * NG + WS - 1) / WS; t_++) {
            const int id0 = wl + WS * t_, id = id0 < N * NG ? id0 : N * NG - 1;
            // (twin of out_g_entry, and below of out_lam_x_entry, kept as text: the calls change this function's compiled code -- profiles/point_maps_refactor.txt)
            const int k = id / NG, i = id - k * NG;
            const double *Zn = W.Zc + k * NZ; const LPtr rr = WL + sc.REF + k * RREC, nu = WL + sc.NUm + k * NI;
            double gv, lv;
            if (i < NE) { gv = WL[sc.G + k * NE + i]; lv = WL[sc.LAM + k * NE + i]; }
            else if (i == 36) { gv = Zn[ZPHI] - PAR[po.phimax]; lv = nu[IPHIMAX]; }
            else if (i == 37) { gv = Zn[ZDPHI] - PAR[po.dphimax]; lv = nu[IDPHIMAX]; }
            else { const int m = i - 38; const double c = rr[RC + m], wd = rr[RWD + m]; gv = c * c - wd * wd; lv = wd > 0 ? (nu[ITUBE + 2 * m] + nu[ITUBE + 2 * m + 1]) / (2 * wd) : 0.0; }
            if (pr.g) pr.g[id] = gv;
            if (pr.lam_g) pr.lam_g[id] = lv;
        }
        if (pr.lam_x) for (int t_ = 0; t_ < (nw + WS - 1) / WS; t_++) {
            const int id0 = wl + WS * t_, id = id0 < nw ? id0 : nw - 1;
            const int k = id / NZ, z = id - k * NZ; const LPtr nu = WL + sc.NUm + k * NI; double v = 0;
            if (z < 8) v = nu[IJU + z] - nu[IJL + z]; else if (z < ZDQ) v = nu[IQU + z - ZQ] - nu[IQL + z - ZQ];
            else if (z < ZDDQ) v = nu[IDQU + z - ZDQ] - nu[IDQL + z - ZDQ]; else if (z == ZPHI) v = -nu[IPHI0];
            pr.lam_x[id] = v;
        }
        if (pr.state) for (int t_ = 0; t_ < (ni + WS - 1) / WS; t_++) { const int id0 = wl + WS * t_, id = id0 < ni ? id0 : ni - 1; pr.state[id] = WL[sc.NUm + id]; }
        if (wl == 0) {
            if (pr.f) *pr.f = fval; if (pr.iters) *pr.iters = status == 4 ? (it | (n_restart << 20)) : it + W.it_base; if (pr.status) *pr.status = (W.it_base && status == 1) ? 2 : status; if (pr.kkt) *pr.kkt = E0;
            if (pr.state) { pr.state[ni] = ((RESTO && el) || status == 4) ? 0.0 : mu; pr.state[ni + 1] = (double)it; }      // (a solve that ends inside the restoration phase leaves no dual state worth carrying)
        }
    WIDE_END
    W.last_status = status; W.last_it = it;
}

// Second attempt (round 6).  On the long-horizon batches the solves that end with status 2 ("locally infeasible": the stall test after the barrier
// restarts) are, 24 times of 26 on BASELINE configs[3], FEASIBLE problems on which the barrier start of the long horizons (mu 3, slacks pushed to 0.1)
// leads into a stationary point of the violation; from the same x0 on the barrier start of the short horizons (mu 0.1, push 1e-2) 22 of them converge in
// 30-93 iterations (profiles/r06_h_configs3_failures.txt).  So a STATELESS solve that ends with status 2 is run once more from x0 with that start and
// at most retry_cap iterations; the reported iteration count is the sum, and a second attempt that runs into its cap keeps the verdict of the first
// (status 2, not 1).  One inlined copy of wave_solve in a loop.  oracle/bmpc_oracle.c bmpc_oracle_solve_warm mirrors it.
#define RETRY_MU_INIT 0.1
#define RETRY_PUSH 1e-2
// x0_retry: the x0 of the solve when pr is the CONTINUATION of a solve another kernel began (restoration kernel: pr.x0 is the iterate it left): the second
// attempt is a fresh solve from there.
template <bool ZLDS, bool RT = false, bool RESTO = false>
BMPC_D inline void wave_solve_retry(Wave &W, const Problem &pr, const double *x0_retry = nullptr) {
    const Opts keep = W.o;
    Problem q = pr;
    W.it_base = 0;
    for (int attempt = 0; ; attempt++) {
        wave_solve<ZLDS, RT, RESTO>(W, q);
        if (attempt || keep.retry_cap <= 0 || pr.state || W.last_status != 2 || keep.max_iter <= 0) break;
        W.o.mu_init = RETRY_MU_INIT; W.o.slack_push = RETRY_PUSH; W.o.max_iter = keep.retry_cap; W.it_base = W.last_it;
        W.o.start_rollout = 1;      // (an x0 far off its own dynamics is rolled out for the second attempt even where the caller wanted it taken as given)
        if (x0_retry) { q.x0 = x0_retry; q.resto_from = -1; }
    }
    W.o = keep; W.it_base = 0;
}

}  // namespace BMPC_NAMESPACE
