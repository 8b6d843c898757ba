// bmpc_kkt.inl -- KKT certificate of ANY primal-dual point (x, lam_g, lam_x) in CasADi's convention: the solver's own error measure for a point it
// did not produce (Ipopt's answer, a shifted plan, a candidate warm start, the rows a graph replay just returned).  include/boundmpc_hip.h
// bmpc_kkt_batch has the record; this is the wave program behind it, built from the pieces of a solver iteration:
//   1. wave_load_point as a solve begins, wave_eval -- the point is taken as given: no start rollout, no projection;
//   2. lam_g / lam_x onto the 57 N internal multipliers nu by the map of bmpc_dual.inl (dual_row; its file comment states the map), into sc.NUm;
//   3. wave_adjoint(..., use_hat = false, mu = 0), as at the top of every solver iteration: the equality multipliers LAM [N][36] that zero the
//      state part of the Lagrangian gradient, and the jerk part RJ [N][8] that remains;
//   4. two wide passes with the deterministic WRED_* reductions: the residuals, then the outputs in the reference's convention (out_g_entry /
//      out_lam_x_entry of bmpc_wave.inl, the output map of wave_solve) with the gaps between the caller's multipliers and the consistent ones.
// The error E is that of wave_solve (its "KKT error (Ipopt-style scaling)") with the slack of a row replaced by max(-h_i, 0): a point carries no
// slacks.  The passes use the output pass's wave-uniform trip counts on clamped indices (build.py lint_isa).  A maximum drops NaN (v > m is
// false), so non-finite values are counted on their own: one non-finite f, g, h, LAM or RJ makes the five error slots NaN.
#pragma once

namespace BMPC_NAMESPACE {

// slots of the record (include/boundmpc_hip.h BMPC_KKT_*)
enum { KKT_E = 0, KKT_DUAL = 1, KKT_PRIM_EQ = 2, KKT_PRIM_INEQ = 3, KKT_COMPL = 4, KKT_LAM_EQ_GAP = 5, KKT_LAM_INEQ_GAP = 6, KKT_F = 7, KKT_LEN = 8 };

struct KktIn {
    const double *p, *x, *lam_g0, *lam_x0;      // one problem; lam_g0 / lam_x0 may be NULL (= no multipliers of that kind)
    double *cert;                              // [KKT_LEN], written
    double *g, *lam_g, *rj;                    // optional outputs [43 N], [43 N], [8 N]; must not overlap the inputs
};

// |given - consistent| of one multiplier entry; +inf when the given entry (or the difference) is not finite
BMPC_D inline double kkt_gap(double given, double own) { const double d = BMPC_FABS(given - own); return bmpc_finite(d) ? d : __builtin_inf(); }

template <bool ZLDS>
BMPC_D inline void wave_certify(Wave &W, const KktIn &d) {
    const int N = W.N, S = W.S;
    double *L = W.L; const GPtr G = W.G; const LPtr WL = BMPC_WL(W);
    const POff po = make_poff_lds(S, L_ZL);
    const Scr sc = make_scr(N);
    const int nw = N * NZ, ni = N * NI, ne = N * NE, nrj = N * NU, ngt = N * NG;
    BMPC_LANE_REGS(LRs);
    wave_load_point<ZLDS>(W, po, sc, d.p, d.x);
    const double fval = wave_eval(W, po, sc, W.Zc, sc.G, sc.HIN, false);
    const bool hx = d.lam_x0 != nullptr, hg = d.lam_g0 != nullptr;
    // ---- multipliers of the internal rows (dual_row of bmpc_dual.inl; into the workspace instead of a dual state) ----
    WIDE_BEGIN
        for (int t_ = 0; t_ < (ni + WS - 1) / WS; t_++) {
            const int id0 = wl + WS * t_, id = id0 < ni ? id0 : ni - 1;
            WL[sc.NUm + id] = dual_row(L, WL, sc, d.lam_g0, d.lam_x0, id);
        }
    WIDE_END
    TEAM_SYNC();
    wave_adjoint(W, po, sc, sc.NUm, false, 0.0, LRs);
    // ---- residuals: inequality rows (h, nu), equality rows (g, LAM), jerk gradient RJ ----
    WIDE_BEGIN
        double ed = 0, pe = 0, pi = 0, cm = 0, sl = 0, sn = 0, bad = 0;
        for (int t_ = 0; t_ < (ni + WS - 1) / WS; t_++) {
            const int id0 = wl + WS * t_, id = id0 < ni ? id0 : ni - 1; const bool ok_ = id0 < ni;
            const double hv = WL[sc.HIN + id], nu = WL[sc.NUm + id];
            const double viol = hv > 0.0 ? hv : 0.0, slack = hv < 0.0 ? -hv : 0.0, c = nu * slack;
            pi = viol > pi ? viol : pi; cm = c > cm ? c : cm; sn += ok_ ? nu : 0.0; bad = bmpc_finite(hv) ? bad : 1.0;
        }
        for (int t_ = 0; t_ < (ne + WS - 1) / WS; t_++) {
            const int id0 = wl + WS * t_, id = id0 < ne ? id0 : ne - 1; const bool ok_ = id0 < ne;
            const double gv = WL[sc.G + id], lv = WL[sc.LAM + id], v = BMPC_FABS(gv);
            pe = v > pe ? v : pe; sl += ok_ ? BMPC_FABS(lv) : 0.0; bad = (bmpc_finite(gv) && bmpc_finite(lv)) ? bad : 1.0;
        }
        for (int t_ = 0; t_ < (nrj + WS - 1) / WS; t_++) {
            const int id0 = wl + WS * t_, id = id0 < nrj ? id0 : nrj - 1;
            const double rv = WL[sc.RJ + id], v = BMPC_FABS(rv);
            ed = v > ed ? v : ed; bad = bmpc_finite(rv) ? bad : 1.0;
            if (d.rj) d.rj[id] = rv;
        }
        WRED_PUT_MAX(L_REDW, 0, ed); WRED_PUT_MAX(L_REDW, 1, pe); WRED_PUT_MAX(L_REDW, 2, pi); WRED_PUT_MAX(L_REDW, 3, cm);
        WRED_PUT_SUM(L_REDW, 4, sl); WRED_PUT_SUM(L_REDW, 5, sn); WRED_PUT_MAX(L_KKPW, 0, bad);
    WIDE_END
    const double ed = WRED_GET_MAX(L_REDW, 0), pe = WRED_GET_MAX(L_REDW, 1), pi = WRED_GET_MAX(L_REDW, 2), cm = WRED_GET_MAX(L_REDW, 3),
                 sl = WRED_GET_SUM(L_REDW, 4), sn = WRED_GET_SUM(L_REDW, 5);
    const bool bad = WRED_GET_MAX(L_KKPW, 0) > 0.0 || !bmpc_finite(fval);
    TEAM_SYNC();      // (every partial has been read before the next pass rewrites the area)
    // ---- the consistent multipliers in the reference's convention (out_g_entry, out_lam_x_entry) and the gaps to the caller's ----
    WIDE_BEGIN
        double ge = 0, gi = 0;
        for (int t_ = 0; t_ < (ngt + WS - 1) / WS; t_++) {
            const int id0 = wl + WS * t_, id = id0 < ngt ? id0 : ngt - 1;
            double gv, lv; out_g_entry(W, po, sc, id, gv, lv);
            const double gap = hg ? kkt_gap(d.lam_g0[id], lv) : 0.0;
            const bool eq = id % NG < NE;
            const double gap_e = eq ? gap : 0.0, gap_i = eq ? 0.0 : gap;
            ge = gap_e > ge ? gap_e : ge; gi = gap_i > gi ? gap_i : gi;
            if (d.g) d.g[id] = gv;
            if (d.lam_g) d.lam_g[id] = lv;
        }
        for (int t_ = 0; t_ < (nw + WS - 1) / WS; t_++) {
            const int id0 = wl + WS * t_, id = id0 < nw ? id0 : nw - 1;
            const double v = out_lam_x_entry(W, sc, id);
            const double gap = hx ? kkt_gap(d.lam_x0[id], v) : 0.0;
            gi = gap > gi ? gap : gi;
        }
        WRED_PUT_MAX(L_REDW, 0, ge); WRED_PUT_MAX(L_REDW, 1, gi);
    WIDE_END
    const double ge = WRED_GET_MAX(L_REDW, 0), gi = WRED_GET_MAX(L_REDW, 1);
    TEAM_SYNC();
    // the scaling of wave_solve: sd from the mean multiplier over the 93 rows of a node, scl from the mean inequality multiplier
    const double sd = BMPC_FMAX(100.0, (sl + sn) / (N * (NE + NI))) / 100.0, scl = BMPC_FMAX(100.0, sn / (N * NI)) / 100.0;
    const double nan_ = __builtin_nan("");
    const double E = BMPC_FMAX(BMPC_FMAX(ed / sd, BMPC_FMAX(pe, pi)), cm / scl);
    WIDE_BEGIN
        if (wl == 0) {
            d.cert[KKT_E] = bad ? nan_ : E; d.cert[KKT_DUAL] = bad ? nan_ : ed; d.cert[KKT_PRIM_EQ] = bad ? nan_ : pe; d.cert[KKT_PRIM_INEQ] = bad ? nan_ : pi;
            d.cert[KKT_COMPL] = bad ? nan_ : cm; d.cert[KKT_LAM_EQ_GAP] = ge; d.cert[KKT_LAM_INEQ_GAP] = gi; d.cert[KKT_F] = fval;
        }
    WIDE_END
}

// B problems back to back in every array (NULL stays NULL): what a service launch gets (bmpc_hip.hip) and what the emulator host is called with
struct KktBatch {
    const double *p, *x, *lam_g0, *lam_x0; double *cert, *g, *lam_g, *rj;
    BMPC_HD KktIn problem(int N, int S, long long b) const {      // problem b of the batch
        const long long np = 141 + 91 * S, nw = N * NZ, ng = N * NG, nj = N * NU;
        KktIn d; d.p = p + b * np; d.x = x + b * nw; d.cert = cert + b * KKT_LEN;
        d.lam_g0 = lam_g0 ? lam_g0 + b * ng : nullptr; d.lam_x0 = lam_x0 ? lam_x0 + b * nw : nullptr;
        d.g = g ? g + b * ng : nullptr; d.lam_g = lam_g ? lam_g + b * ng : nullptr; d.rj = rj ? rj + b * nj : nullptr;
        return d;
    }
    template <bool ZLDS> BMPC_D void run(Wave &W, int b) const { wave_certify<ZLDS>(W, problem(W.N, W.S, b)); }
};

}  // namespace BMPC_NAMESPACE
