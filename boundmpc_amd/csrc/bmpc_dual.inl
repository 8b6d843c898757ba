// bmpc_dual.inl -- primal-dual warm start: the dual state of a warm solve ([nu (N x 57) | mu | iterations], bmpc_solve_batch_warm) from
// multipliers in CasADi's convention (lam_g [N][43], lam_x [N][44]: what a solve returns, what Ipopt's warm_start_init_point reads).
//
// The map is the inverse of the output map of wave_solve (bmpc_wave.inl out_g_entry, out_lam_x_entry), per node k, with
// pos(v) = max(v, 0):
//   IJU + j, IJL + j (j < 8)       pos(lam_x[j]), pos(-lam_x[j])             (and the same for IQU / IQL with the q entries, IDQU / IDQL with dq)
//   IPHI0                          pos(-lam_x[ZPHI])                          (phi has the lower bound 0 only)
//   IPHIMAX, IDPHIMAX              pos(lam_g[36]), pos(lam_g[37])
//   ITUBE + 2m, ITUBE + 2m + 1     pos(lam (wd + c)), pos(lam (wd - c))       lam = pos(lam_g[38 + m]), m < 5
// c and wd (>= 0) are the centre value and the half width of the tube row AT x0 -- rr[RC + m], rr[RWD + m] of the record the evaluation
// leaves, the same words the output pass reads: the two rows sum to 2 wd lam and differ by 2 c lam, so the map is the exact inverse of the
// forward map wherever |c| <= wd.  Not read: the equality rows lam_g[0:36] (the adjoint sweep recomputes the equality multipliers at every
// iterate) and lam_x of the unbounded variables.  A non-finite entry counts as 0; a converted multiplier is capped at DUAL_NU_CAP.
// dual_row below is the map, once: it reuses the row table of wave_init_tables (sign and source variable of the box rows); the output map is
// out_g_entry / out_lam_x_entry of bmpc_wave.inl.  The row passes use the output pass's wave-uniform trip counts on clamped indices (build.py lint_isa).
#pragma once

namespace BMPC_NAMESPACE {

// Largest multiplier the conversion writes.  The warm solve starts a row with the slack min(mu / nu, slack_push) at mu >= mu_warm (1e-2 by
// default): with nu <= 1e12 that slack stays a normal positive double (>= 1e-14 at the default levels) however large the caller's entry.
// The largest |lam| the solver returns is 7.9e2 on the BASELINE configs[1] batch and 8.9e5 on configs[3]: the cap sits more
// than six orders of magnitude above both.
#define DUAL_NU_CAP 1e12

struct DualIn {
    const double *p, *x0, *lam_g, *lam_x;      // one problem; lam_g / lam_x may be NULL (= zeros)
    double *state;                             // [N * 57 + 2], written
    double mu;                                 // > 0: the barrier level of the state; else the handle's mu_warm
};

BMPC_D inline double dual_finite(double v) { return bmpc_finite(v) ? v : 0.0; }      // (NaN and +-inf -> 0)
BMPC_D inline double dual_cap(double v) { return v > 0.0 ? (v < DUAL_NU_CAP ? v : DUAL_NU_CAP) : 0.0; }      // pos() with the cap; NaN -> 0

// The map above for one internal row: the capped nu of row id (< 57 N: the caller clamps) from lam_g / lam_x (NULL = zeros), the row table in
// LDS (wave_init_tables) and the reference records the evaluation at the point left.  Every load is unconditional, on a clamped index.
// Callers: the row passes of wave_state_from_multipliers, wave_certify (bmpc_kkt.inl) and wave_sensitivity (bmpc_sens.inl).
BMPC_D inline double dual_row(const double *L, const LPtr WL, const Scr &sc, const double *lam_g, const double *lam_x, int id) {
    const bool hx = lam_x != nullptr, hg = lam_g != nullptr;
    const int k = id / NI, r = id - k * NI;
    const int rb = r <= IPHI0 ? r : IPHI0;                                                  // box row of the table (clamped)
    const int ig = r < ITUBE ? (r > IPHIMAX ? 37 : 36) : 38 + ((r - ITUBE) >> 1);          // lam_g entry of a non-box row
    const int m = r < ITUBE ? 0 : (r - ITUBE) >> 1;
    const double sgn = L[L_ROWT + rb], src = L[L_ROWT + 2 * NI + rb];
    const double vx = hx ? dual_finite(lam_x[k * NZ + (int)src]) : 0.0;
    const double vg = hg ? dual_finite(lam_g[k * NG + ig]) : 0.0;
    const LPtr rr = WL + sc.REF + k * RREC;
    const double c = rr[RC + m], wd = rr[RWD + m];
    double v;
    if (r <= IPHI0) v = sgn * vx;
    else if (r < ITUBE) v = vg;
    else { const double lam = vg > 0.0 ? vg : 0.0; v = ((r - ITUBE) & 1) ? lam * (wd - c) : lam * (wd + c); }
    return dual_cap(v);
}

// One problem: evaluation at x0 exactly as a solve begins (wave_load_point, wave_eval; no start rollout), then the row pass.  State slot mu:
// d.mu when positive, else o.mu_warm; 0 (the cold start of the warm path) when every converted multiplier is 0.  Slot iterations: 0.
template <bool ZLDS>
BMPC_D inline void wave_state_from_multipliers(Wave &W, const DualIn &d) {
    const int N = W.N, S = W.S;
    double *L = W.L; const LPtr WL = BMPC_WL(W);
    const POff po = make_poff_lds(S, L_ZL);
    const Scr sc = make_scr(N);
    const int ni = N * NI;
    wave_load_point<ZLDS>(W, po, sc, d.p, d.x0);
    wave_eval(W, po, sc, W.Zc, sc.G, sc.HIN, false);
    WIDE_BEGIN
        double nmax = 0.0;
        for (int t_ = 0; t_ < (ni + WS - 1) / WS; t_++) {
            const int id0 = wl + WS * t_, id = id0 < ni ? id0 : ni - 1;
            const double nu = dual_row(L, WL, sc, d.lam_g, d.lam_x, id);
            d.state[id] = nu;
            nmax = nu > nmax ? nu : nmax;
        }
        WRED_PUT_MAX(L_REDW, 4, nmax);
    WIDE_END
    const bool any = WRED_GET_MAX(L_REDW, 4) > 0.0;
    TEAM_SYNC();
    WIDE_BEGIN
        if (wl == 0) { d.state[ni] = any ? (d.mu > 0.0 ? d.mu : W.o.mu_warm) : 0.0; d.state[ni + 1] = 0.0; }
    WIDE_END
}

// B problems back to back in every array (NULL stays NULL): what a service launch gets (bmpc_hip.hip) and what the emulator host is called with
struct DualBatch {
    const double *p, *x0, *lam_g, *lam_x; double *state; double mu;
    BMPC_HD DualIn problem(int N, int S, long long b) const {      // problem b of the batch
        const long long np = 141 + 91 * S, nw = N * NZ, ng = N * NG;
        DualIn d; d.p = p + b * np; d.x0 = x0 + b * nw; d.state = state + b * (N * NI + 2); d.mu = mu;
        d.lam_g = lam_g ? lam_g + b * ng : nullptr; d.lam_x = lam_x ? lam_x + b * nw : nullptr;
        return d;
    }
    template <bool ZLDS> BMPC_D void run(Wave &W, int b) const { wave_state_from_multipliers<ZLDS>(W, problem(W.N, W.S, b)); }
};

}  // namespace BMPC_NAMESPACE
