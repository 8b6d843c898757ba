// bmpc_sens.inl -- parametric sensitivity of the solution: the tangent (dx, dLAM, dnu) along a direction dp of the parameter vector, at ANY
// primal-dual point (x, lam_g, lam_x) in CasADi's convention and a barrier level mu.  include/boundmpc_hip.h bmpc_sens_batch has the definition
// (the linearised perturbed barrier KKT system) and the record; this is the wave program behind it, built from the phases of a solver iteration:
//   1. the evaluation at (x, p) and the multipliers nu of the 57 N internal rows by the map of bmpc_dual.inl, as bmpc_kkt.inl does it; the slack
//      of a row s = max(-h, mu / max(nu, mu)) and the barrier ratio Sigma = nu / s, which goes where a solver iteration keeps nu / t (sc.SG);
//   2. the right-hand side by DIFFERENCING THE RESIDUAL: wave_eval + wave_adjoint at p + eps dp and at p - eps dp with x and nu held fixed.  The
//      adjoint sweep recomputes the equality multipliers at either point, so the Lagrangian gradient it leaves is zero in every state and RJ in
//      the jerks BY CONSTRUCTION: the central difference of (RJ, g, h) is d/dt of the residual with the states eliminated, and the shift of the
//      equality multipliers it implies is absorbed by dLAM (see 5);
//   3. evaluation and adjoint at p once more (the records and the equality multipliers the exact Hessian needs); then the "QP gradient" of a
//      solver iteration is replaced by the right-hand side: Jh^T (Sigma h') from wave_node_grad_wide with the objective weights zeroed (every
//      term of grad f carries a weight: what is left is exactly Jh^T v), plus RJ' in the jerk entries; the equality residual by g';
//   4. ONE factorisation -- wave_stage_data_wide, team_backward with the inertia loop of wave_solve (delta 0, 1e-3, x10 ...) -- and ONE forward
//      sweep: the Newton machinery solves K dz = -(gradient, residual), which is the tangent system;
//   5. (only when the caller wants them) dnu = Sigma (Jh dx + h'), and dLAM as the derivative of the adjoint's equality multipliers along the
//      whole tangent: a second central difference of wave_eval + wave_adjoint at (x +- t dx, nu +- t dnu, p +- t dp).  The adjoint zeroes the
//      state part of the Lagrangian gradient identically, so its derivative satisfies the state rows of the stationarity equation with the exact
//      Hessian; with a Gauss-Newton handle or delta > 0 it is the multiplier tangent of the exact system at the dx of the modified one.
// One wave per problem (NW == 1) on the handle's workspace.  Arrays of the slab that a solver iteration uses for trial points, slack and
// multiplier directions hold the differenced residuals here.  The row passes use wave-uniform trip counts on clamped indices (build.py lint_isa).
#pragma once

namespace BMPC_NAMESPACE {

// slots of the record (include/boundmpc_hip.h BMPC_SENS_*)
enum { SENS_STATUS = 0, SENS_DELTA = 1, SENS_RHS = 2, SENS_DX = 3, SENS_LEN = 4 };
#define SENS_EPS 1e-6        // relative step of the central differences (include/boundmpc_hip.h: eps = SENS_EPS max(1, |p|_inf) / |dp|_inf)
#define SENS_TINY 1e-300

struct SensIn {
    const double *p, *x, *lam_g0, *lam_x0, *dp;      // one problem; lam_g0 / lam_x0 may be NULL (= zeros)
    double mu;                                      // barrier level (> 0)
    double *dx;                                     // [44 N], written
    double *dlam_eq, *dnu, *rec;                    // optional outputs [36 N], [57 N], [SENS_LEN]
};

// the parameter vector p + t dp into LDS, and the tables that depend on it
template <bool ZLDS>
BMPC_D inline void sens_load_p(Wave &W, const POff &po, const SensIn &d, double t) {
    double *L = W.L; const int S = W.S, np = po.size;
    WIDE_BEGIN
        for (int t_ = 0; t_ < (np + WS - 1) / WS; t_++) {
            const int id0 = wl + WS * t_, id = id0 < np ? id0 : np - 1;
            L[L_PAR + (ZLDS ? id : lds_index_of_p(S, id, L_ZL))] = d.p[id] + t * d.dp[id];
        }
    WIDE_END
    wave_init_tables(W, po);
}

template <bool ZLDS>
BMPC_D inline void wave_sensitivity(Wave &W, const SensIn &d) {
    static_assert(NW == 1, "the sensitivity program is a one-wave program (one-wave workspace layout)");
    const int N = W.N, S = W.S;
    double *L = W.L; const GPtr G = W.G; const LPtr WL = BMPC_WL(W);
    const POff po = make_poff_lds(S, L_ZL);
    const Scr sc = make_scr(N);
    const int np = po.size, nw = N * NZ, ni = N * NI, ne = N * NE, nrj = N * NU;
    BMPC_LANE_REGS(LRs);
    wave_iterate_ptrs<ZLDS>(W, sc);
    double *DX = (G + sc.DZ).ptr();      // the tangent dx, kept in the slab (the LDS direction area is the block area of the next sweep)
    const double nan_ = __builtin_nan("");
    const bool duals = d.dlam_eq != nullptr || d.dnu != nullptr;
    // ---- the inputs: |p|_inf, |dp|_inf, |x|_inf (the steps of the differences) and whether all of them are finite ----
    WIDE_BEGIN
        double mp = 0, md = 0, mx = 0, bad = 0;
        for (int t_ = 0; t_ < (np + WS - 1) / WS; t_++) {
            const int id0 = wl + WS * t_, id = id0 < np ? id0 : np - 1;
            const double a = BMPC_FABS(d.p[id]), b = BMPC_FABS(d.dp[id]);
            mp = a > mp ? a : mp; md = b > md ? b : md; bad = (bmpc_finite(a) && bmpc_finite(b)) ? bad : 1.0;
        }
        for (int t_ = 0; t_ < (nw + WS - 1) / WS; t_++) {
            const int id0 = wl + WS * t_, id = id0 < nw ? id0 : nw - 1;
            const double a = BMPC_FABS(d.x[id]);
            mx = a > mx ? a : mx; bad = bmpc_finite(a) ? bad : 1.0;
        }
        WRED_PUT_MAX(L_REDW, 0, mp); WRED_PUT_MAX(L_REDW, 1, md); WRED_PUT_MAX(L_REDW, 2, mx); WRED_PUT_MAX(L_REDW, 3, bad);
    WIDE_END
    const double pinf = WRED_GET_MAX(L_REDW, 0), dinf = WRED_GET_MAX(L_REDW, 1), xinf = WRED_GET_MAX(L_REDW, 2);
    const bool bad_in = WRED_GET_MAX(L_REDW, 3) > 0.0;
    TEAM_SYNC();
    // (dp = 0: step 0 and an exactly zero right-hand side; the step is capped so that eps dp stays finite for a denormal direction of a huge p)
    const double eps = dinf > 0.0 ? BMPC_FMIN(SENS_EPS * BMPC_FMAX(1.0, pinf) / BMPC_FMAX(dinf, SENS_TINY), 1e300) : 0.0, inv2e = dinf > 0.0 ? 0.5 / eps : 0.0;
    double delta = 0.0, rhs = 0.0, dxm = 0.0; bool ok = false;
    if (!bad_in) {      // (wave-uniform)
        // ---- 1. the point: evaluation, multipliers of the internal rows (dual_row of bmpc_dual.inl), slacks and barrier ratios ----
        WIDE_BEGIN
            for (int t_ = 0; t_ < (nw + WS - 1) / WS; t_++) { const int id0 = wl + WS * t_, id = id0 < nw ? id0 : nw - 1; W.Zc[id] = d.x[id]; }
        WIDE_END
        sens_load_p<ZLDS>(W, po, d, 0.0);
        wave_eval(W, po, sc, W.Zc, sc.G, sc.HIN, false);
        const double mu = d.mu;
        WIDE_BEGIN
            for (int t_ = 0; t_ < (ni + WS - 1) / WS; t_++) {
                const int id0 = wl + WS * t_, id = id0 < ni ? id0 : ni - 1;
                const double hv = WL[sc.HIN + id];
                const double nu = dual_row(L, WL, sc, d.lam_g0, d.lam_x0, id), nm = nu > mu ? nu : mu, s0 = mu / nm, s = -hv > s0 ? -hv : s0;
                WL[sc.NUm + id] = nu; WL[sc.SG + id] = nu / s;
            }
        WIDE_END
        TEAM_SYNC();
        bool bad_rhs = false;
        // ---- 2., 3. residuals at p + eps dp (-> GT, HT, LAM in TT, RJ in DE), at p - eps dp (-> G, HIN, LAM in ET, RJ in E), then the point itself ----
#pragma nounroll
        for (int leg = 0; leg < 3; leg++) {
            Scr sl = sc;
            if (leg == 0) { sl.LAM = sc.TT; sl.RJ = sc.DE; } else if (leg == 1) { sl.LAM = sc.ET; sl.RJ = sc.E; }
            sens_load_p<ZLDS>(W, po, d, leg == 0 ? eps : (leg == 1 ? -eps : 0.0));
            wave_eval(W, po, sc, W.Zc, leg == 1 ? sc.G : sc.GT, leg == 0 ? sc.HT : sc.HIN, false);
            wave_adjoint(W, po, sl, sc.NUm, false, 0.0, LRs);
            if (leg == 1) {
                // the differences: h' -> DT and v = Sigma h' -> DNU, g' -> G (the equality residual of the Newton system), RJ' -> DE
                WIDE_BEGIN
                    double mr = 0, bad = 0;
                    for (int t_ = 0; t_ < (ni + WS - 1) / WS; t_++) {
                        const int id0 = wl + WS * t_, id = id0 < ni ? id0 : ni - 1;
                        const double hd_ = (WL[sc.HT + id] - WL[sc.HIN + id]) * inv2e, v = WL[sc.SG + id] * hd_, a = BMPC_FABS(hd_);
                        WL[sc.DT + id] = hd_; WL[sc.DNU + id] = v;
                        mr = a > mr ? a : mr; bad = (bmpc_finite(a) && bmpc_finite(v)) ? bad : 1.0;
                    }
                    for (int t_ = 0; t_ < (ne + WS - 1) / WS; t_++) {
                        const int id0 = wl + WS * t_, id = id0 < ne ? id0 : ne - 1;
                        const double gd_ = (WL[sc.GT + id] - WL[sc.G + id]) * inv2e, a = BMPC_FABS(gd_);
                        const bool ok_ = id0 < ne;      // (in place: a clamped duplicate may read what its owner has written -- it stores to a spare word and counts nowhere)
                        WL[ok_ ? sc.G + id : sc.GVP + 6] = gd_;
                        mr = (ok_ && a > mr) ? a : mr; bad = (!ok_ || bmpc_finite(a)) ? bad : 1.0;
                    }
                    for (int t_ = 0; t_ < (nrj + WS - 1) / WS; t_++) {
                        const int id0 = wl + WS * t_, id = id0 < nrj ? id0 : nrj - 1;
                        const double rd_ = (WL[sc.DE + id] - WL[sc.E + id]) * inv2e, a = BMPC_FABS(rd_);
                        const bool ok_ = id0 < nrj;
                        WL[ok_ ? sc.DE + id : sc.GVP + 6] = rd_;
                        mr = (ok_ && a > mr) ? a : mr; bad = (!ok_ || bmpc_finite(a)) ? bad : 1.0;
                    }
                    WRED_PUT_MAX(L_REDW, 0, mr); WRED_PUT_MAX(L_REDW, 1, bad);
                WIDE_END
                rhs = WRED_GET_MAX(L_REDW, 0); bad_rhs = WRED_GET_MAX(L_REDW, 1) > 0.0;      // (read here: the next evaluation reuses the area)
                TEAM_SYNC();
            }
        }
        // ---- 3. the gradient of the Newton system: Jh^T (Sigma h') (objective weights zeroed for the pass) plus RJ' in the jerk entries ----
        WIDE_BEGIN
            if (wl < 15) L[L_PAR + po.w + wl] = 0.0;
        WIDE_END
        wave_node_grad_wide(W, po, sc, sc.DNU, false, 0.0);
        WIDE_BEGIN
            const double wv_ = d.p[make_poff(S).w + (wl < 15 ? wl : 14)];      // (unconditional load on a clamped index)
            if (wl < 15) L[L_PAR + po.w + wl] = wv_;
            for (int t_ = 0; t_ < (nrj + WS - 1) / WS; t_++) {
                const int id0 = wl + WS * t_, id = id0 < nrj ? id0 : nrj - 1, k = id >> 3, z = id & 7;
                const double v = WL[sc.GH + k * NZ + z] + WL[sc.DE + id];
                WL[id0 < nrj ? sc.GH + k * NZ + z : sc.GVP + 6] = v;
            }
        WIDE_END
        TEAM_SYNC();
        // ---- 4. one factorisation (inertia loop of wave_solve from a cold history), one forward sweep ----
        if (!bad_rhs) {
            wave_stage_data_wide(W, po, sc);
            for (int tries = 0; tries < 40; tries++) {
                if (team_backward(W, po, sc, mu, delta, LRs)) { ok = true; break; }
                if (delta == 0.0) delta = DELTA_FIRST; else delta *= DELTA_UP_FIRST;
                if (delta > 1e20) break;
            }
            if (ok) {
                SOLO_BEGIN(0)
                wave_forward(W, sc, LRs);
                SOLO_END
                TEAM_SYNC();
                WIDE_BEGIN
                    double m = 0, bad = 0;
                    for (int t_ = 0; t_ < (nw + WS - 1) / WS; t_++) {
                        const int id0 = wl + WS * t_, id = id0 < nw ? id0 : nw - 1;
                        const double v = W.Dz[id], a = BMPC_FABS(v);
                        if (ZLDS) DX[id] = v;
                        m = a > m ? a : m; bad = bmpc_finite(a) ? bad : 1.0;
                    }
                    WRED_PUT_MAX(L_REDW, 0, m); WRED_PUT_MAX(L_REDW, 1, bad);
                WIDE_END
                dxm = WRED_GET_MAX(L_REDW, 0);
                ok = !(WRED_GET_MAX(L_REDW, 1) > 0.0);
                TEAM_SYNC();
            }
        }
    }
    // ---- dx and the record ----
    WIDE_BEGIN
        for (int t_ = 0; t_ < (nw + WS - 1) / WS; t_++) { const int id0 = wl + WS * t_, id = id0 < nw ? id0 : nw - 1; d.dx[id] = ok ? DX[id] : nan_; }
        if (wl == 0 && d.rec) {
            d.rec[SENS_STATUS] = ok ? (delta > 0.0 ? 1.0 : 0.0) : 3.0; d.rec[SENS_DELTA] = ok ? delta : 0.0;
            d.rec[SENS_RHS] = bad_in ? nan_ : rhs; d.rec[SENS_DX] = ok ? dxm : nan_;
        }
    WIDE_END
    if (!duals) return;      // (wave-uniform)
    if (!ok) {
        WIDE_BEGIN
            if (d.dnu) for (int t_ = 0; t_ < (ni + WS - 1) / WS; t_++) { const int id0 = wl + WS * t_, id = id0 < ni ? id0 : ni - 1; d.dnu[id] = nan_; }
            if (d.dlam_eq) for (int t_ = 0; t_ < (ne + WS - 1) / WS; t_++) { const int id0 = wl + WS * t_, id = id0 < ne ? id0 : ne - 1; d.dlam_eq[id] = nan_; }
        WIDE_END
        return;
    }
    // ---- 5. dnu = Sigma (Jh dx + h'): grad h_i . dx by ineq_dir of bmpc_wave.inl (the row formulas live there), records of the point itself ----
    WIDE_BEGIN
        for (int t_ = 0; t_ < (ni + WS - 1) / WS; t_++) {
            const int id0 = wl + WS * t_, id = id0 < ni ? id0 : ni - 1;
            const int k = id / NI, i = id - k * NI;
            const double hd_ = ineq_dir(DX + k * NZ, (WL + sc.REF + k * RREC).ptr(), i);
            const double v = WL[sc.SG + id] * (hd_ + WL[sc.DT + id]);
            WL[sc.DNU + id] = v;
            if (d.dnu) d.dnu[id] = v;
        }
    WIDE_END
    TEAM_SYNC();
    if (!d.dlam_eq) return;
    // ---- 5. dLAM: the adjoint's equality multipliers differenced along the whole tangent (LAM in TT at +t, in ET at -t) ----
    const double t2 = dinf > 0.0 ? BMPC_FMIN(SENS_EPS * BMPC_FMAX(1.0, BMPC_FMAX(pinf, xinf)) / BMPC_FMAX(BMPC_FMAX(dinf, dxm), SENS_TINY), 1e300) : 0.0, inv2t = dinf > 0.0 ? 0.5 / t2 : 0.0;
#pragma nounroll
    for (int leg = 0; leg < 2; leg++) {
        Scr sl = sc;
        if (leg == 0) { sl.LAM = sc.TT; sl.RJ = sc.DE; } else { sl.LAM = sc.ET; sl.RJ = sc.E; }
        const double t = leg == 0 ? t2 : -t2;
        WIDE_BEGIN
            for (int t_ = 0; t_ < (nw + WS - 1) / WS; t_++) { const int id0 = wl + WS * t_, id = id0 < nw ? id0 : nw - 1; W.Zc[id] = d.x[id] + t * DX[id]; }
            for (int t_ = 0; t_ < (ni + WS - 1) / WS; t_++) { const int id0 = wl + WS * t_, id = id0 < ni ? id0 : ni - 1; WL[sc.NU2 + id] = WL[sc.NUm + id] + t * WL[sc.DNU + id]; }
        WIDE_END
        sens_load_p<ZLDS>(W, po, d, t);
        wave_eval(W, po, sc, W.Zc, sc.GT, sc.HT, false);
        wave_adjoint(W, po, sl, sc.NU2, false, 0.0, LRs);
    }
    WIDE_BEGIN
        for (int t_ = 0; t_ < (ne + WS - 1) / WS; t_++) {
            const int id0 = wl + WS * t_, id = id0 < ne ? id0 : ne - 1;
            d.dlam_eq[id] = (WL[sc.TT + id] - WL[sc.ET + id]) * inv2t;
        }
    WIDE_END
}

// B problems back to back in every array (NULL stays NULL): what a service launch gets (bmpc_hip.hip) and what the emulator host is called with
struct SensBatch {
    const double *p, *x, *lam_g0, *lam_x0, *dp; double mu; double *dx, *dlam_eq, *dnu, *rec;
    BMPC_HD SensIn problem(int N, int S, long long b) const {      // problem b of the batch
        const long long np = 141 + 91 * S, nw = N * NZ, ng = N * NG, ne = N * NE, ni = N * NI;
        SensIn d; d.p = p + b * np; d.x = x + b * nw; d.dp = dp + b * np; d.mu = mu; d.dx = dx + b * nw;
        d.lam_g0 = lam_g0 ? lam_g0 + b * ng : nullptr; d.lam_x0 = lam_x0 ? lam_x0 + b * nw : nullptr;
        d.dlam_eq = dlam_eq ? dlam_eq + b * ne : nullptr; d.dnu = dnu ? dnu + b * ni : nullptr; d.rec = rec ? rec + b * SENS_LEN : nullptr;
        return d;
    }
    template <bool ZLDS> BMPC_D void run(Wave &W, int b) const { wave_sensitivity<ZLDS>(W, problem(W.N, W.S, b)); }
};

}  // namespace BMPC_NAMESPACE
