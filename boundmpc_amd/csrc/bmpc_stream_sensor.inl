// bmpc_stream_sensor.inl -- a MEASUREMENT MODEL between the plant of a closed-loop stream and its controller, as device code: what an encoder makes of
// the joint state (an offset per joint, a quantisation step, noise on q, dq and ddq, a sample that is one tick old) and how the plant is kept apart from
// it.  The pack and the post of a tick read the robot record, and the record IS the plant; here the record is swapped for the sample ahead of the pack
// (stream_sense; the truth is kept in the sensor state) and swapped back behind the post (stream_truth): where the sample differed from the truth, the
// TRUE plant takes the step the post took on the sample, under the same planned jerk.  A disturbance cannot stand in for this: it moves the plant, and the
// next pack measures the moved plant exactly.  Host mirrors and specifications: boundmpc_amd.stream.sense_robot and truth_robot.  Included behind
// bmpc_stream_events.inl; used by the two sensor kernels of bmpc_rollout_sensor.hip (bmpc_stream_sense, bmpc_stream_unsense) and by the rollouts with a
// sensor table (bmpc_rollout_kernel.inl, SE).
//
// Like stream_disturb and stream_plant: one pass over the kinematic chain of ONE stream, so one lane does the work (`lane`, `nl` as in the neighbours:
// the other lanes of the wave pass through); the caller puts a barrier behind either before other lanes read the record.
// The same text is compiled by g++ for the CPU tests (tests/emu).
#pragma once

#include "bmpc_stream_events.inl"

namespace bmpcs {
static_assert(bmpcse::ST_TRUTH + bmpcse::TRUTH_LEN <= bmpcse::ST_LEN && RB_XPHID == bmpcse::TRUTH_LEN - 7 && RB_V + 6 == RB_XPHID, "the truth: RB_Q..RB_V, then RB_JERK");

// the record of a stream that has taken no sample: the conventions of stream_plant_init
BMPC_HD inline void stream_sensor_init(double *rec) {
    for (int i = 0; i < bmpcse::REC_LEN; i++) rec[i] = 0.0;
    rec[bmpcse::REC_MAX_DQ] = -__builtin_inf(); rec[bmpcse::REC_TICK_DQ] = -1.0; rec[bmpcse::REC_JOINT_DQ] = -1.0;
    rec[bmpcse::REC_MAX_DP] = -__builtin_inf(); rec[bmpcse::REC_TICK_DP] = -1.0;
}

// The sample of tick `tick`, ahead of its pack and behind the lost-plan test.  row [bmpcse::LEN]: the stream's row as the caller gave it (a VALID row,
// bmpc_sensor_check; a NaN slot takes its identity value here as there); noise [DIST_LEN] or NULL: the tick's unit draws, delta q 7 | delta dq 7 |
// delta ddq 7, a non-finite word counts as 0 (stream_disturb); state [bmpcse::ST_LEN]: in and out; rb: the robot record, the TRUTH on entry; rec
// [bmpcse::REC_LEN] or NULL: accumulated.
//   TRUTH = rb[RB_Q..RB_V], rb[RB_JERK], always
//   per joint  m_q = (q + BIAS_j) + NQ n_j, with RES > 0 then RES rint(m_q / RES) (half to even);  m_dq = dq + NDQ n_{7+j};  m_ddq = ddq + NDDQ n_{14+j}
//   out = (HOLD == 1 and HAS) ? HELD : m;  HELD = m, HAS = 1;  SAME = every word of out compares equal to the truth's
// Where SAME == 0 the record's q, dq, ddq become out and p_lie and v are those of out (fk_motion with the record's jerk, as stream_disturb); RB_JERK and
// RB_XPHID are kept.  Where SAME == 1 the record keeps every bit.  The record counts the sample and what it differs from the truth by.
BMPC_HD inline void stream_sense(const double *row, const double *noise, double *state, double *rb, double *rec, int tick, int lane, int nl) {
    if (lane == 0) {
        double w[bmpcse::SLOTS];
        for (int k = 0; k < bmpcse::SLOTS; k++) { const double v = row[k]; w[k] = v != v ? bmpc_sensor_identity(k) : v; }
        for (int i = 0; i < RB_XPHID; i++) state[bmpcse::ST_TRUTH + i] = rb[i];
        for (int j = 0; j < 7; j++) state[bmpcse::ST_TRUTH + RB_XPHID + j] = rb[RB_JERK + j];
        const double res = w[bmpcse::RES];
        const bool held = w[bmpcse::HOLD] == 1.0 && state[bmpcse::ST_HAS] == 1.0;
        double out[DIST_LEN];
        bool same = true;
        for (int i = 0; i < DIST_LEN; i++) {
            const int j = i % 7;
            double ni = noise ? noise[i] : 0.0;
            ni = (ni - ni == 0.0) ? ni : 0.0;
            double m;
            if (i < 7) {
                m = (rb[RB_Q + j] + w[bmpcse::BIAS + j]) + w[bmpcse::NQ] * ni;
                if (res > 0.0) m = res * __builtin_rint(m / res);
            } else m = rb[RB_Q + i] + w[i < 14 ? bmpcse::NDQ : bmpcse::NDDQ] * ni;
            out[i] = held ? state[bmpcse::ST_HELD + i] : m;
            state[bmpcse::ST_HELD + i] = m;
            same = same && out[i] == rb[RB_Q + i];
        }
        state[bmpcse::ST_HAS] = 1.0;
        state[bmpcse::ST_SAME] = same ? 1.0 : 0.0;
        double dp = 0.0;
        double dq[7];
        for (int j = 0; j < 7; j++) dq[j] = out[j] - rb[RB_Q + j];
        if (!same) {
            double u[7];
            for (int j = 0; j < 7; j++) u[j] = rb[RB_JERK + j];
            FkMotion M; fk_motion(out, out + 7, out + 14, u, M);
            double s2 = 0.0;
            for (int c = 0; c < 3; c++) { const double e = M.p[c] - rb[RB_P + c]; s2 += e * e; }
            dp = BMPC_SQRT(s2);
            for (int i = 0; i < DIST_LEN; i++) rb[RB_Q + i] = out[i];
            for (int c = 0; c < 6; c++) { rb[RB_P + c] = M.p[c]; rb[RB_V + c] = M.v[c]; }
        }
        if (rec) {
            rec[bmpcse::REC_SAMPLES] += 1.0;
            for (int j = 0; j < 7; j++) {
                const double e = dq[j] < 0.0 ? -dq[j] : dq[j], m = rec[bmpcse::REC_MAX_DQ];
                const bool bad = !(e - e == 0.0);
                if (bad ? m == m : e > m) { rec[bmpcse::REC_MAX_DQ] = bad ? __builtin_nan("") : e; rec[bmpcse::REC_TICK_DQ] = (double)tick; rec[bmpcse::REC_JOINT_DQ] = (double)j; }
                rec[bmpcse::REC_SUMSQ_DQ] += dq[j] * dq[j];
            }
            const double m = rec[bmpcse::REC_MAX_DP];
            const bool bad = !(dp - dp == 0.0);
            if (bad ? m == m : dp > m) { rec[bmpcse::REC_MAX_DP] = bad ? __builtin_nan("") : dp; rec[bmpcse::REC_TICK_DP] = (double)tick; }
        }
    }
}

// The plant behind the post of a tick that stream_sense opened (behind the barrier behind stream_post, ahead of the plant step).  state: what
// stream_sense left; stepped: the post stepped the record (ss[SS_ERRCNT] < N behind it).  SAME == 1: nothing -- the post has stepped the truth itself,
// bit for bit.  Else, where the post stepped: with c = rb[RB_JERK] the first planned jerk, q, dq, ddq are chain_step(TRUTH q, dq, ddq, TRUTH jerk, c, h),
// p_lie and v those of the new joint state, the jerk stays c -- the step of stream_post on the true plant.  Else (the post exhausted the plan and did not
// step): rb[RB_Q..RB_V] are the truth's again.  RB_XPHID is the post's.
BMPC_HD inline void stream_truth(double h, const double *state, double *rb, bool stepped, int lane, int nl) {
    if (lane == 0 && !(state[bmpcse::ST_SAME] == 1.0)) {
        const double *tr = state + bmpcse::ST_TRUTH;
        if (stepped) {
            double q[7], dq[7], ddq[7], c[7];
            for (int j = 0; j < 7; j++) {
                double a = tr[RB_Q + j], da = tr[RB_DQ + j], dda = tr[RB_DDQ + j];
                c[j] = rb[RB_JERK + j];
                chain_step(a, da, dda, tr[RB_XPHID + j], c[j], h);
                q[j] = a; dq[j] = da; ddq[j] = dda;
            }
            FkMotion M; fk_motion(q, dq, ddq, c, M);
            for (int j = 0; j < 7; j++) { rb[RB_Q + j] = q[j]; rb[RB_DQ + j] = dq[j]; rb[RB_DDQ + j] = ddq[j]; }
            for (int c6 = 0; c6 < 6; c6++) { rb[RB_P + c6] = M.p[c6]; rb[RB_V + c6] = M.v[c6]; }
        } else {
            for (int i = 0; i < RB_XPHID; i++) rb[i] = tr[i];
        }
    }
}

}  // namespace bmpcs
