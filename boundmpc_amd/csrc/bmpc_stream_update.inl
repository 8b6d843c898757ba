// bmpc_stream_update.inl -- re-planning of a stream as device code: ReferencePath.__init__ (ReferencePath.py:10-163) and the state part of
// BoundMPC.update() (BoundMPC.py:163-217).  Host mirror and specification: boundmpc_amd.reference_path.ReferencePath.__init__,
// boundmpc_amd.stream.path_table and boundmpc_amd.stream.apply_update (fixtures G4, G11).
//
// One function, one stream per 64-lane wave, written as phases over `nl` cooperating lanes like stream_pack / stream_post / stream_log (the CPU
// test build runs it with one lane).  It reads one re-plan record and writes the stream's path table block, the state scalars update() sets
// and, on request, the goal of the robot record:
//   rec   [RP_HEAD + n_max RV_LEN], n_max = cap - S + 1 via points at most (the table holds n + S - 1 slots of a path of n via points):
//         header (32): flag | n | nb | p0 3 | v 3 | a 3 | jerk 3 | weights 15 | 2 pad      (the linear parts update() uses)
//         via entry (32): p 3 | R 9 (row-major) | p_lower 2 | p_upper 2 | r_lower 2 | r_upper 2 | bp1 3 | br1 3 | s | e_p_min | e_r_min |
//                         e_p_max | e_r_max | 1 pad                                             (bp1 / br1 of the first nb entries are read)
//   path  [cap][PT_LEN]: every row is written: slots 0..M-1, M = n + S - 1, as path_table lays them out, rows M..cap-1 copy row M-1
//   ss    SS_SECTOR = 0, the path-parameter state projected onto the first segment, SS_PRREF, SS_IWREF, SS_PHIMAX, the weights, SS_NENT = M, the
//         `updated` flag; an error count >= N goes back to N - 1 (apply_update: a stream that lost its plan gets a new attempt).  The previous
//         solution, its Cartesian arrays and dphi_max (ss_dphimax: the constructor's weights[4], which update() leaves, BoundMPC.py:77-79,194) stay.
//   rb    (may be null) with flag bit 0 (set_goal): RB_XPHID = (phi_max, 0, 0), what the node does right after update() (bound_mpc_node.py:164)
// Flag protocol: flag == 0 leaves the stream alone (table block and state row untouched, info 0).  Otherwise the record is consumed: the flag
// is cleared at the end, so a captured graph that holds this launch re-plans only when someone raises a flag again.  n < 2, n > n_max,
// nb < 1, nb > n or a non-finite n / nb: invalid record, the stream is untouched, the flag cleared, info 1.  Non-finite numbers elsewhere and a
// basis vector parallel to its direction give non-finite entries, as the host mirror does; every index into the record and the table is
// clamped.  The call belongs between a tick's post (or log) and the next pack.
//
// The running sums (integrated-omega reference iw, cumulative arc length) are summed by ONE lane in place in the table, in the order of the
// host's lists (iw[i] + dr[i], np.cumsum): a path has a handful of via points, the serial loop is a few dependent additions, and the result
// is bit-equal run to run and to the host's order of summation by construction; a wave scan would associate differently.
// The same text is compiled by g++ for the CPU tests (tests/emu).
#pragma once

namespace bmpcs {
enum { RP_FLAG = 0, RP_N = 1, RP_NB = 2, RP_P0 = 3, RP_V = 6, RP_A = 9, RP_JERK = 12, RP_W = 15, RP_HEAD = 32 };
enum { RV_P = 0, RV_R = 3, RV_PLO = 12, RV_PUP = 14, RV_RLO = 16, RV_RUP = 18, RV_BP1 = 20, RV_BR1 = 23, RV_S = 26, RV_EPMIN = 27, RV_ERMIN = 28,
       RV_EPMAX = 29, RV_ERMAX = 30, RV_LEN = 32 };
enum { PT_TMP = PT_S + 1 };      // first pad word of a table entry: between the phases "this segment inherits the previous direction"; zero at the end
BMPC_HD inline int replan_len(int S, int cap) { return RP_HEAD + RV_LEN * (cap - S + 1); }

// error-plane basis (ReferencePath.py:111-150): b1 made orthogonal to the unit direction d and normalised, b2 = d x b1
BMPC_HD inline void plane_basis(const double *d, const double *b, double *b1, double *b2) {
    const double s = dot3(d, b);
    const double t[3] = {b[0] - s * d[0], b[1] - s * d[1], b[2] - s * d[2]};
    const double n = norm3(t);
    b1[0] = t[0] / n; b1[1] = t[1] / n; b1[2] = t[2] / n;
    cross3s(d, b1, b2);
}

// cap = entries the path table holds.  info (may be null): 0, or 1 for an invalid record.
BMPC_HD inline void stream_update(int N, int S, double *rec, double *path, int cap, double *ss, double *rb, int *info, int flags, int lane, int nl) {
    const int n_max = cap - S + 1;
    const double fl = rec[RP_FLAG], nd = rec[RP_N], nbd = rec[RP_NB];
    if (fl == 0.0) {                                               // (uniform over the lanes)
        if (lane == 0 && info) *info = 0;
        return;
    }
    // the counts, read so that a non-finite word fails the tests
    const bool n_ok = nd >= 2.0 && nd <= (double)n_max;
    const int n = n_ok ? (int)nd : 2;
    const bool nb_ok = nbd >= 1.0 && nbd <= (double)n;
    const int nb = nb_ok ? (int)nbd : 1;
    BMPCS_SYNC();                                                  // every lane has read the flag before one lane clears it
    if (!(n_ok && nb_ok)) {
        if (lane == 0) { rec[RP_FLAG] = 0.0; if (info) *info = 1; }
        return;
    }
    const int M = n + S - 1;
    const double *via = rec + RP_HEAD;
    // ---- phase 1: one lane per via point j: what is copied, the rotation vector of R[j], and the segment j -> j + 1: direction (a vanishing
    //      segment, < 1e-3, inherits the previous direction in phase 2; the first one becomes [0,1,0]), rotation increment
    //      mat_to_rotvec(R[j+1] R[j]^T), length (a pure rotation: |dr| / pi), dr normalised by the length.  The raw increment and the length go to
    //      the IW / CUM words of entry j + 1, where phase 2 sums them up. ----
    for (int j = lane; j < n; j += nl) {
        const double *e = via + j * RV_LEN;
        double *row = path + j * PT_LEN;
        double rv[3];
        mat_to_rotvec(e + RV_R, rv);
        for (int c = 0; c < 3; c++) { row[PT_P + c] = e[RV_P + c]; row[PT_RRV + c] = rv[c]; }
        for (int c = 0; c < 8; c++) row[PT_PLO + c] = e[RV_PLO + c];
        row[PT_S] = e[RV_S]; row[PT_EPMIN] = e[RV_EPMIN]; row[PT_ERMIN] = e[RV_ERMIN]; row[PT_EPMAX] = e[RV_EPMAX]; row[PT_ERMAX] = e[RV_ERMAX];
        if (j == 0) { row[PT_IW] = 0.0; row[PT_IW + 1] = 0.0; row[PT_IW + 2] = 0.0; row[PT_CUM] = 0.0; }
        if (j + 1 < n) {
            const double *en = e + RV_LEN;
            double *nxt = row + PT_LEN;
            const double d[3] = {en[RV_P] - e[RV_P], en[RV_P + 1] - e[RV_P + 1], en[RV_P + 2] - e[RV_P + 2]};
            const double li = norm3(d);
            const bool vanish = li < 1e-3;
            double dR[9], drr[3];
            mat3_mul_bt(en + RV_R, e + RV_R, dR);
            mat_to_rotvec(dR, drr);
            const double seg = vanish ? norm3(drr) / 3.14159265358979323846 : li;
            for (int c = 0; c < 3; c++) {
                row[PT_DPN + c] = vanish ? (c == 1 && j == 0 ? 1.0 : 0.0) : d[c] / li;
                row[PT_DR + c] = drr[c] / seg;
                nxt[PT_IW + c] = drr[c];
            }
            nxt[PT_CUM] = seg;
            row[PT_TMP] = (vanish && j > 0) ? 1.0 : 0.0;
        }
    }
    BMPCS_SYNC();
    // ---- phase 2 (one lane): the running sums in place, inherited directions, and the padded segment behind the last via point (direction of
    //      the last segment, dr = [1,1,1]) ----
    if (lane == 0) {
        for (int j = 1; j < n; j++) {
            double *row = path + j * PT_LEN;
            const double *prev = row - PT_LEN;
            for (int c = 0; c < 3; c++) row[PT_IW + c] = prev[PT_IW + c] + row[PT_IW + c];
            row[PT_CUM] = prev[PT_CUM] + row[PT_CUM];
            if (j == n - 1 || row[PT_TMP] > 0.5) for (int c = 0; c < 3; c++) row[PT_DPN + c] = prev[PT_DPN + c];
            if (j == n - 1) for (int c = 0; c < 3; c++) row[PT_DR + c] = 1.0;
        }
    }
    BMPCS_SYNC();
    // ---- phase 3: one lane per table row: the S - 1 padding slots behind the last via point as the host lists are padded, rows M.. = row M - 1,
    //      and the Gram-Schmidt bases (computed for slots < nb, the last one beyond).  Reads of other rows touch words no lane writes here. ----
    const double *last = path + (n - 1) * PT_LEN;
    for (int j = lane; j < cap; j += nl) {
        double *row = path + j * PT_LEN;
        if (j >= n) {
            const int jj = j < M ? j : M - 1;
            for (int c = 0; c < PT_BP1; c++) row[c] = last[c];                       // p, iw, direction, dr, rotation vector, limits
            for (int c = PT_EPMIN; c <= PT_S; c++) row[c] = last[c];
            double cum = last[PT_CUM];
            for (int t = n - 1; t < jj; t++) cum += 1.0;                             // the padded lengths are 1 (np.cumsum order)
            row[PT_CUM] = cum;
        }
        const int k = j < nb ? j : nb - 1;
        const double *rk = path + k * PT_LEN, *ek = via + k * RV_LEN;
        const double dn[3] = {rk[PT_DPN], rk[PT_DPN + 1], rk[PT_DPN + 2]};
        double om[3], b1[3], b2[3], c1[3], c2[3];
        unit_or_y(rk + PT_DR, 1e-4, om);
        plane_basis(dn, ek + RV_BP1, b1, b2);
        plane_basis(om, ek + RV_BR1, c1, c2);
        for (int c = 0; c < 3; c++) { row[PT_BP1 + c] = b1[c]; row[PT_BP2 + c] = b2[c]; row[PT_BR1 + c] = c1[c]; row[PT_BR2 + c] = c2[c]; }
        for (int c = PT_TMP; c < PT_LEN; c++) row[c] = 0.0;
    }
    // ---- the state scalars (one lane, beside phase 3; apply_update) ----
    if (lane == nl - 1) {
        const double *e0 = path, *p0 = rec + RP_P0;
        const double dn[3] = {e0[PT_DPN], e0[PT_DPN + 1], e0[PT_DPN + 2]}, dr0[3] = {e0[PT_DR], e0[PT_DR + 1], e0[PT_DR + 2]};
        const double rel[3] = {p0[0] - via[RV_P], p0[1] - via[RV_P + 1], p0[2] - via[RV_P + 2]};
        const double phi = dot3(rel, dn), phi_max = last[PT_CUM] - 0.0001;
        double prr[3];
        integrate_rotation_reference(e0 + PT_RRV, dr0, 0.0, phi, prr);
        ss[SS_SECTOR] = 0.0;
        ss[SS_PHI] = phi; ss[SS_DPHI] = dot3(rec + RP_V, dn); ss[SS_DDPHI] = dot3(rec + RP_A, dn); ss[SS_DDDPHI] = dot3(rec + RP_JERK, dn);
        for (int c = 0; c < 3; c++) { ss[SS_PRREF + c] = prr[c]; ss[SS_IWREF + c] = e0[PT_IW + c] + phi * dr0[c]; }
        ss[SS_PHIMAX] = phi_max;
        for (int c = 0; c < 15; c++) ss[SS_W + c] = rec[RP_W + c];
        ss[SS_NENT] = (double)M;
        ss[ss_updated(N)] = 1.0;
        if (ss[SS_ERRCNT] >= (double)N) ss[SS_ERRCNT] = (double)(N - 1);
        if ((flags & 1) && rb) { rb[RB_XPHID] = phi_max; rb[RB_XPHID + 1] = 0.0; rb[RB_XPHID + 2] = 0.0; }
        rec[RP_FLAG] = 0.0;
        if (info) *info = 0;
    }
}

}  // namespace bmpcs
