// bmpc_stream_log.inl -- the logging records of BoundMPC.step() as device code: ref_data / err_data of compute_return_data
// (BoundMPC.py:614-752; host mirror: boundmpc_amd.bound_mpc.BoundMPC._logging_data with _segment_rows).
//
// One function, one stream per 64-lane wave, written as phases over `nl` cooperating lanes like stream_pack / stream_post (the CPU test
// build runs it with one lane).  It runs AFTER the tick's post-processing and reads only what a tick leaves behind:
//   p       as stream_pack wrote it: q0, dq0, p0, the rotation-reference integral before this tick's advance, the initial orientation errors,
//           phi_switch, the SO(3) Jacobians, the window of the path with its bases, tube quartics and dual vectors (offsets: make_poff);
//   traj    as stream_post wrote it: the re-integrated p, v, phi, dphi per stage and n_valid;
//   ss      after the post: SS_PRREF (the advanced rotation reference), SS_SECTOR, SS_ERRCNT;
//   path    PT_RRV of the entries sector + 1 and sector + 2 (re-anchoring of the rotation reference at a segment switch).
// It writes nothing but the log row  [N][LOG_STAGE] | n_valid | error_count | 2 pad,  a stage being
//   ref (55): p 6, dp 6, ddp 6, dp_normed 3, r_par_bound 1, bound_lower 4, bound_upper 4, e_p_off 2, e_r_off 2, bp1, bp2, br1, br2, v1, v2, v3 (3 each)
//   err (33): e_p, de_p, e_p_par, e_p_orth, de_p_par, de_p_orth, e_r, de_r, e_r_par, e_r_orth1, e_r_orth2 (3 each)
// in the key order of the reference's dictionaries (tests/golden/make_g10.py REF_KEYS / ERR_KEYS).  ref p[3:] and e_r are the values of the
// reference's SECOND pass (:712-752): the rotation reference integrated along the plan and the orientation error against it.
// Stages at or beyond n_valid are NaN.  A stream without a plan (error count >= N: step() returns Nones, the fused tick skips it) gets
// n_valid = 0 and an all-NaN body, so that a stale row is never read as a result.  Non-finite inputs give non-finite records: every table
// index (segment row, path entry, stage) is clamped before it is used, loads are unconditional on the clamped index and selects follow.
#pragma once

namespace bmpcs {
enum { LOG_REF = 55, LOG_ERR = 33, LOG_STAGE = LOG_REF + LOG_ERR };
BMPC_HD inline int log_len(int N) { return N * LOG_STAGE + 4; }
// shared workspace: integrated angular velocity [3][STREAM_NMAX] and rotation reference [3][STREAM_NMAX] of the stages
enum { LSH_IW = 0, LSH_PR = 3 * STREAM_NMAX, LSH_LEN = 6 * STREAM_NMAX };

// angular velocity of the end effector, (J(q) dq)[3:]: the angular rows of the geometric Jacobian are the joint axes (forward_kinematics'
// A[j]), so only the rotation part of the chain is run
BMPC_HD inline void angular_velocity(const double *q, const double *dq, double *om) {
    const int ax[7] = {2, 1, 2, -1, 2, 1, 2};
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    om[0] = 0.0; om[1] = 0.0; om[2] = 0.0;
#pragma unroll
    for (int j = 0; j < 7; j++) {
        double cs = cos_b(q[j]), sn = sin_b(q[j]);
        if (ax[j] == 2) {
            for (int c = 0; c < 3; c++) { om[c] += dq[j] * R[c * 3 + 2]; const double c0 = R[c * 3], c1 = R[c * 3 + 1]; R[c * 3] = cs * c0 + sn * c1; R[c * 3 + 1] = -sn * c0 + cs * c1; }
        } else {
            const double sg = (double)ax[j]; sn *= sg;
            for (int c = 0; c < 3; c++) { om[c] += dq[j] * (sg * R[c * 3 + 1]); const double c0 = R[c * 3], c2 = R[c * 3 + 2]; R[c * 3] = cs * c0 - sn * c2; R[c * 3 + 2] = sn * c0 + cs * c2; }
        }
    }
}

// h: the sampling time of the plan.  cap = entries the path table holds.  sh: shared workspace of LSH_LEN doubles.
// The writer of the row.  CUT: only the first `stages` stages (1..N) are written, the row is  [stages][LOG_STAGE] | n_valid | error_count | 2 pad  with
// the n_valid of the WHOLE plan, and the serial parts stop at the last stage that is kept (a stage needs only the stages ahead of it): the rows of a
// rollout (bmpc_rollout_kernel.inl, LG).  Without CUT `stages` is not looked at and the text is the one of the whole row, N in its place.
template <bool CUT>
BMPC_HD inline void stream_log_rows(int N, int S, double h, const double *path, int cap, const double *ss, const double *p, const double *traj, double *log,
                                    int stages, double *sh, int lane, int nl) {
    const double qnan = __builtin_nan("");
    const int K = CUT ? stages : N;                                // stages of the row
    const int TRN = tr_len(N), LL = K * LOG_STAGE + 4;
    // the counts, read so that a non-finite word means "no plan" (the tests are written so that a NaN fails them)
    const double ecd = ss[SS_ERRCNT], nvd = traj[TRN - 4];
    const int ec = (ecd >= 0.0 && ecd < (double)N) ? (int)ecd : N;
    int n = (nvd >= 1.0 && nvd <= (double)N) ? (int)nvd : 0;
    n = n > N - ec ? N - ec : n;
    if (lane == 0) { log[LL - 4] = (double)n; log[LL - 3] = (double)ec; log[LL - 2] = 0.0; log[LL - 1] = 0.0; }
    if (n <= 0) {                                                  // (uniform over the lanes)
        for (int id = lane; id < K * LOG_STAGE; id += nl) log[id] = qnan;
        return;
    }
    const int m = CUT ? (n < K ? n : K) : n;                       // stages the serial parts run to
    const BMPC_NAMESPACE::POff o = BMPC_NAMESPACE::make_poff(S);
    const double *Tp = traj + 4 * 7 * N, *Tv = Tp + 6 * N, *Tphi = Tv + 12 * N, *Tdphi = Tphi + N;
    const double *p0 = p + o.p0;
    // ---- phase 1 (one lane): the two serial parts ----
    if (lane == 0) {
        // integrated angular velocity of the plan: trapezoid from omega(q0, dq0) over the angular rows of v (:574-586), sign flip after failures (:587-589)
        double om[3], acc[3] = {p0[3], p0[4], p0[5]};
        angular_velocity(p + o.q0, p + o.dq0, om);
        for (int i = 0; i < m; i++)
            for (int c = 0; c < 3; c++) {
                const double v = Tv[(3 + c) * N + i];
                acc[c] = acc[c] + 0.5 * h * (om[c] + v); om[c] = v;
                sh[LSH_IW + c * STREAM_NMAX + i] = acc[c];
            }
        const double d0[3] = {p0[3] - sh[LSH_IW], p0[4] - sh[LSH_IW + STREAM_NMAX], p0[5] - sh[LSH_IW + 2 * STREAM_NMAX]};
        if (ec > 0 && norm3(d0) > 3.1)
            for (int i = 0; i < m; i++) for (int c = 0; c < 3; c++) sh[LSH_IW + c * STREAM_NMAX + i] = -sh[LSH_IW + c * STREAM_NMAX + i];
        // rotation reference integrated along the plan from the advanced reference, re-anchored at the via rotations where a stage crosses
        // phi_switch[1] or [2] (:712-752)
        const double sd = ss[SS_SECTOR];
        int sector = (sd >= 0.0 && sd <= (double)(cap - 1)) ? (int)sd : 0;
        const int e1 = sector + 1 < cap ? sector + 1 : cap - 1, e2 = sector + 2 < cap ? sector + 2 : cap - 1;      // clamped to the table
        const double sw1 = p[o.sw + 1], sw2 = p[o.sw + 2];
        double pr[3] = {ss[SS_PRREF], ss[SS_PRREF + 1], ss[SS_PRREF + 2]};
        for (int i = 0; i < m; i++) {
            for (int c = 0; c < 3; c++) sh[LSH_PR + c * STREAM_NMAX + i] = pr[c];
            if (i + 1 < m) {
                const double phi = Tphi[i], nxt = Tphi[i + 1];
                const bool a1 = nxt > sw1 && phi < sw1, a2 = !a1 && nxt > sw2 && phi < sw2;
                const int k = a1 ? 1 : ((a2 || nxt > sw2) ? 2 : (nxt > sw1 ? 1 : 0));
                const int kc = k < S ? k : S - 1;                              // row of the S-row window arrays
                const double *e = path + (a1 ? e1 : e2) * PT_LEN;
                double from[3], w[3];
                for (int c = 0; c < 3; c++) {
                    const double anchor = e[PT_RRV + c];
                    from[c] = (a1 || a2) ? anchor : pr[c];
                    w[c] = p[o.dpref + (3 + c) * S + kc];
                }
                integrate_rotation_reference(from, w, a1 ? sw1 : (a2 ? sw2 : phi), nxt, pr);
            }
        }
    }
    BMPCS_SYNC();
    // ---- phase 2: one lane per stage.  Every lane works on a valid stage (its own, or the last one) and the stores select NaN ----
    for (int i = lane; i < K; i += nl) {
        const bool live = i < n;
        const int ic = live ? i : n - 1;
        double *ref = log + i * LOG_STAGE, *err = ref + LOG_REF;
#define BMPCS_LOG_PUT(dst, v) (dst) = live ? (v) : qnan
        const double phi = Tphi[ic], dphi = Tdphi[ic];
        // segment rows of the nested if_else selections (bound_mpc_functions.py:13-40): S-row arrays, the two-row window of bp1 / bp2,
        // tube coefficients (row S is row S-1, so the row of the S-row arrays serves)
        int seg = S - 1;
        for (int j = S - 2; j >= 0; j--) if (phi < p[o.sw + j + 1]) seg = j;
        const int segb = seg < S - 2 ? seg : S - 2;
        const double x = phi - p[o.sw + seg];
        double dp_d[6], p_d[6], tp[6], tv[6];
        for (int k = 0; k < 6; k++) {
            dp_d[k] = p[o.dpref + k * S + seg]; p_d[k] = dp_d[k] * x + p[o.pref + k * S + seg];
            tp[k] = Tp[k * N + ic]; tv[k] = Tv[k * N + ic];
        }
        double b[9];
        for (int ch = 0; ch < 9; ch++) {
            const int id = ch * (S + 1) + seg;
            b[ch] = (((p[o.a[0] + id] * x + p[o.a[1] + id]) * x + p[o.a[2] + id]) * x + p[o.a[3] + id]) * x + p[o.a[4] + id];
        }
        double dn[3], br1[3], br2[3], v1[3], v2[3], v3[3], iw[3], prr[3];
        for (int c = 0; c < 3; c++) {
            dn[c] = p[o.dpn + c * S + seg]; br1[c] = p[o.br1 + c * S + seg]; br2[c] = p[o.br2 + c * S + seg];
            v1[c] = p[o.v1 + c * S + seg]; v2[c] = p[o.v2 + c * S + seg]; v3[c] = p[o.v3 + c * S + seg];
            iw[c] = sh[LSH_IW + c * STREAM_NMAX + ic]; prr[c] = sh[LSH_PR + c * STREAM_NMAX + ic];
        }
        // ref
        for (int c = 0; c < 3; c++) { BMPCS_LOG_PUT(ref[c], p_d[c]); BMPCS_LOG_PUT(ref[3 + c], prr[c]); }      // p[3:]: second pass
        for (int k = 0; k < 6; k++) { BMPCS_LOG_PUT(ref[6 + k], dp_d[k]); BMPCS_LOG_PUT(ref[12 + k], 0.0 * dp_d[k]); }
        for (int c = 0; c < 3; c++) BMPCS_LOG_PUT(ref[18 + c], dn[c]);
        BMPCS_LOG_PUT(ref[21], b[8]);
        BMPCS_LOG_PUT(ref[22], b[2]); BMPCS_LOG_PUT(ref[23], b[3]); BMPCS_LOG_PUT(ref[24], b[6]); BMPCS_LOG_PUT(ref[25], b[7]);      // bound_lower
        BMPCS_LOG_PUT(ref[26], b[0]); BMPCS_LOG_PUT(ref[27], b[1]); BMPCS_LOG_PUT(ref[28], b[4]); BMPCS_LOG_PUT(ref[29], b[5]);      // bound_upper
        BMPCS_LOG_PUT(ref[30], 0.5 * (b[0] + b[2])); BMPCS_LOG_PUT(ref[31], 0.5 * (b[1] + b[3]));                                    // e_p_off
        BMPCS_LOG_PUT(ref[32], 0.5 * (b[4] + b[6])); BMPCS_LOG_PUT(ref[33], 0.5 * (b[5] + b[7]));                                    // e_r_off
        for (int c = 0; c < 3; c++) {
            BMPCS_LOG_PUT(ref[34 + c], p[o.bp1 + c * S + segb]); BMPCS_LOG_PUT(ref[37 + c], p[o.bp2 + c * S + segb]);
            BMPCS_LOG_PUT(ref[40 + c], br1[c]); BMPCS_LOG_PUT(ref[43 + c], br2[c]);
            BMPCS_LOG_PUT(ref[46 + c], v1[c]); BMPCS_LOG_PUT(ref[49 + c], v2[c]); BMPCS_LOG_PUT(ref[52 + c], v3[c]);
        }
        // position errors in the path frame
        double e[3], de[3];
        for (int c = 0; c < 3; c++) { e[c] = tp[c] - p_d[c]; de[c] = tv[c] - dp_d[c] * dphi; }
        const double ep = dot3(dp_d, e), dep = dot3(dp_d, de);
        for (int c = 0; c < 3; c++) {
            const double e_par = ep * dp_d[c], de_par = dep * dp_d[c];
            BMPCS_LOG_PUT(err[c], e[c]); BMPCS_LOG_PUT(err[3 + c], de[c]);
            BMPCS_LOG_PUT(err[6 + c], e_par); BMPCS_LOG_PUT(err[9 + c], e[c] - e_par);
            BMPCS_LOG_PUT(err[12 + c], de_par); BMPCS_LOG_PUT(err[15 + c], de[c] - de_par);
        }
        // orientation errors of the first pass: linearised with the SO(3) Jacobians around the initial error (p holds their transposes)
        const double *jr = p + o.jacr, *jl = p + o.jacl, *dtau0 = p + o.dtau;
        double dl[3];
        for (int r = 0; r < 3; r++) {
            double s = 0.0, t = 0.0, ds = 0.0, dt = 0.0;
            for (int c = 0; c < 3; c++) {
                s += jl[c * 3 + r] * (iw[c] - p0[3 + c]); t += jr[c * 3 + r] * (p_d[3 + c] - p[o.iwref0 + c]);
                ds += jl[c * 3 + r] * tv[3 + c]; dt += jr[c * 3 + r] * (dp_d[3 + c] * dphi);
            }
            const double e_r = dtau0[r] + s - t;
            dl[r] = e_r - dtau0[r];
            BMPCS_LOG_PUT(err[21 + r], ds - dt);                                                                                    // de_r
        }
        const double d1 = dot3(dl, v1), d2 = dot3(dl, v2), d3 = dot3(dl, v3);
        for (int c = 0; c < 3; c++) {
            BMPCS_LOG_PUT(err[24 + c], p[o.ipar + 3 * seg + c] + d2 * dn[c]);
            BMPCS_LOG_PUT(err[27 + c], p[o.io1 + 3 * seg + c] + d1 * br1[c]);
            BMPCS_LOG_PUT(err[30 + c], p[o.io2 + 3 * seg + c] + d3 * br2[c]);
        }
    }
    // ---- phase 3, one lane per stage: e_r of the second pass, log(R(p) R(ref)^T) against the integrated rotation reference.  (A loop of its
    //      own: with the conversions inside phase 2 the register allocator of this toolchain does not survive the function.) ----
    for (int i = lane; i < K; i += nl) {
        const bool live = i < n;
        const int ic = live ? i : n - 1;
        double *err = log + i * LOG_STAGE + LOG_REF;
        double rv[3], prr[3], Ra[9], Rb[9], er[3];
        for (int c = 0; c < 3; c++) { rv[c] = Tp[(3 + c) * N + ic]; prr[c] = sh[LSH_PR + c * STREAM_NMAX + ic]; }
        rotvec_to_mat(rv, Ra); rotvec_to_mat(prr, Rb); mat3_mul_bt(Ra, Rb, Ra);
        mat_to_rotvec(Ra, er);
        for (int c = 0; c < 3; c++) BMPCS_LOG_PUT(err[18 + c], er[c]);
    }
#undef BMPCS_LOG_PUT
}
// the whole row  [N][LOG_STAGE] | n_valid | error_count | 2 pad  (bmpc_stream_log)
BMPC_HD inline void stream_log(int N, int S, double h, const double *path, int cap, const double *ss, const double *p, const double *traj, double *log,
                               double *sh, int lane, int nl) {
    stream_log_rows<false>(N, S, h, path, cap, ss, p, traj, log, N, sh, lane, nl);
}

// stream_track_init / stream_track: the tracking record of a rollout (bmpc_rollout_kernel.inl, LG) over STAGE 0 of the log rows of its ticks -- the state
// the plant is in behind the tick, in the path frame --,
//   track [TRACK_LEN = 12] = samples | max, tick, sum of squares of ||e_p_orth|| | the same of ||e_p_par|| | the same of ||e_r|| | replayed | pad
// (BMPC_TRACK_* of include/boundmpc_hip.h; host mirror and specification: boundmpc_amd.stream.track_of_rows).  Both are the work of ONE lane (lane 0,
// which wrote stage 0 and the trailer of the row); the record lives in global memory between the ticks.
enum { TRACK_SAMPLES = 0, TRACK_MAX_EP_ORTH, TRACK_TICK_EP_ORTH, TRACK_SUMSQ_EP_ORTH, TRACK_MAX_EP_PAR, TRACK_TICK_EP_PAR, TRACK_SUMSQ_EP_PAR, TRACK_MAX_ER,
       TRACK_TICK_ER, TRACK_SUMSQ_ER, TRACK_REPLAYED, TRACK_PAD, TRACK_LEN };
BMPC_HD inline void stream_track_init(double *track) {
    const double ninf = -__builtin_inf();
    for (int f = 0; f < 3; f++) { track[TRACK_MAX_EP_ORTH + 3 * f] = ninf; track[TRACK_TICK_EP_ORTH + 3 * f] = -1.0; track[TRACK_SUMSQ_EP_ORTH + 3 * f] = 0.0; }
    track[TRACK_SAMPLES] = 0.0; track[TRACK_REPLAYED] = 0.0; track[TRACK_PAD] = 0.0;
}
// stage: stage 0 of the row of tick t; n_valid: the row's; using_previous: the word of the tick's trajectory record.  A tick without a valid stage is
// no sample.  A larger norm replaces the maximum, a non-finite one makes it NaN for good (the audit's rule).
BMPC_HD inline void stream_track(const double *stage, double n_valid, double using_previous, double *track, int t) {
    if (!(n_valid >= 1.0)) return;
    track[TRACK_SAMPLES] += 1.0;
    if (using_previous > 0.0) track[TRACK_REPLAYED] += 1.0;
    const int at[3] = {LOG_REF + 9, LOG_REF + 6, LOG_REF + 18};      // e_p_orth, e_p_par, e_r (second pass)
    for (int f = 0; f < 3; f++) {
        const double *v = stage + at[f];
        const double sq = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2], nrm = BMPC_SQRT(sq);
        const bool bad = !(nrm - nrm == 0.0);
        const double mx = track[TRACK_MAX_EP_ORTH + 3 * f];
        if (bad ? mx == mx : nrm > mx) { track[TRACK_MAX_EP_ORTH + 3 * f] = bad ? __builtin_nan("") : nrm; track[TRACK_TICK_EP_ORTH + 3 * f] = (double)t; }
        track[TRACK_SUMSQ_EP_ORTH + 3 * f] += sq;
    }
}

}  // namespace bmpcs
