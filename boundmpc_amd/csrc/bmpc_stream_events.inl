// bmpc_stream_events.inl -- what happens to a closed-loop stream BETWEEN two ticks, as device code: the splice of the measured state into a
// re-plan record (bound_mpc_node.py:121-137,158-162: what the node takes from the plant before it calls BoundMPC.update) and a disturbance of
// the plant.  Host mirrors and specifications: boundmpc_amd.stream.splice_record and disturb_robot.  Included behind bmpc_stream.inl; used by
// the update and disturb kernels of bmpc_hip.hip and by the rollouts with events (bmpc_rollout_kernel.inl, EV).
//
// Both functions are one forward pass over the kinematic chain of ONE stream, so one lane does the work (`lane`, `nl` as in the neighbours: the
// other lanes of the wave pass through); the caller puts a barrier behind them before other lanes read the record.
// The same text is compiled by g++ for the CPU tests (tests/emu).
#pragma once

#include "bmpc_stream_update.inl"

namespace bmpcs {
enum { DIST_LEN = 21 };      // disturbance row: delta q 7 | delta dq 7 | delta ddq 7   (BMPC_DIST_LEN)

// The words of a RAISED, valid record that the node takes from the plant, from the robot record rb behind a post:
//   via[0].p = p_lie[0:3] + 0.5 h v[0:3]  (:131);  flags bit 2 (the node's scenario 0, :126-129): v[2] < 0 and p_lie[1] via[1].p[1] < 0 ->
//              via[0].p[2] -= 0.05
//   via[0].R = rotation matrix of the rotation vector p_lie[3:6]  (:134)
//   header   p0 = p_lie[0:3], v = v[0:3], a = J ddq + dJ dq, jerk = J u + 2 dJ ddq + ddJ dq (linear rows; q, dq, ddq, u = jerk of rb)
// The robot record carries no Cartesian acceleration or jerk.  The node keeps them from its plant step (util_functions.py:152-161): its `a` is this
// a; its j_cart takes ddJ at the state BEFORE the step and J ddq where the kinematics say J u.  Here the jerk is the time derivative of a.  The
// difference reaches one state word, SS_DDDPHI.
// A record whose flag is 0 and an invalid record (the test of stream_update: info 1) are not touched.  cap: entries of the path table, as there.
BMPC_HD inline void stream_splice(double h, int S, int cap, double *rec, const double *rb, int flags, int lane, int nl) {
    const double fl = rec[RP_FLAG], nd = rec[RP_N], nbd = rec[RP_NB];
    if (fl == 0.0) return;                                         // (uniform over the lanes)
    const bool n_ok = nd >= 2.0 && nd <= (double)(cap - S + 1);
    const bool nb_ok = nbd >= 1.0 && nbd <= (n_ok ? (double)(int)nd : 2.0);
    if (!(n_ok && nb_ok)) return;
    if (lane == 0) {
        const double *pl = rb + RB_P, *v = rb + RB_V;
        double *via = rec + RP_HEAD;
        FkMotion M; fk_motion<true>(rb + RB_Q, rb + RB_DQ, rb + RB_DDQ, rb + RB_JERK, M);
        double R0[9]; rotvec_to_mat(pl + 3, R0);
        const bool poor = (flags & 4) && v[2] < 0.0 && pl[1] * via[RV_LEN + RV_P + 1] < 0.0;
        for (int c = 0; c < 3; c++) {
            via[RV_P + c] = pl[c] + 0.5 * h * v[c];
            rec[RP_P0 + c] = pl[c]; rec[RP_V + c] = v[c]; rec[RP_A + c] = M.a[c]; rec[RP_JERK + c] = M.jk[c];
        }
        if (poor) via[RV_P + 2] -= 0.05;
        for (int c = 0; c < 9; c++) via[RV_R + c] = R0[c];
    }
}

// Plant disturbance: d [DIST_LEN] is added to q, dq, ddq of the robot record, then the pose and the Cartesian velocity of the record are those
// of the disturbed joint state (fk_motion with the record's jerk).  A non-finite entry counts as 0; an all-zero row leaves the record
// untouched, bit for bit.
BMPC_HD inline void stream_disturb(double *rb, const double *d, int lane, int nl) {
    if (lane == 0) {
        double x[DIST_LEN];
        bool any = false;
        for (int i = 0; i < DIST_LEN; i++) {
            const double di = d[i];
            x[i] = (di - di == 0.0) ? di : 0.0;
            any = any || x[i] != 0.0;
        }
        if (any) {
            double q[7], dq[7], ddq[7], u[7];
            for (int j = 0; j < 7; j++) { q[j] = rb[RB_Q + j] + x[j]; dq[j] = rb[RB_DQ + j] + x[7 + j]; ddq[j] = rb[RB_DDQ + j] + x[14 + j]; u[j] = rb[RB_JERK + j]; }
            FkMotion M; fk_motion(q, dq, ddq, u, M);
            for (int j = 0; j < 7; j++) { rb[RB_Q + j] = q[j]; rb[RB_DQ + j] = dq[j]; rb[RB_DDQ + j] = ddq[j]; }
            for (int c = 0; c < 6; c++) { rb[RB_P + c] = M.p[c]; rb[RB_V + c] = M.v[c]; }
        }
    }
}

}  // namespace bmpcs
