// bmpc_stream_plant.inl -- an ACTUATOR MODEL between the command of a closed-loop stream and its plant, as device code: what the drive makes of the
// first planned jerk of a tick (gain and offset per joint, a first-order lag, a clip, one tick of dead time) and what the plant then is.  The post
// (stream_post, role RF + 1) moves the robot record with the model's own integrator chain and the planned jerk c; here the record is corrected to the
// one the same chain reaches under the jerk u the drive delivers.  The chain is linear in the new jerk (chain_step: x += h^3/24 u, dx += h^2/6 u,
// ddx += h/2 u), so the correction by D = u - c IS the plant ramped from the old true jerk to u instead of to c.  Host mirror and specification:
// boundmpc_amd.stream.plant_robot.  Included behind bmpc_stream_events.inl; used by the plant kernel of bmpc_hip.hip (bmpc_stream_plant) and by the
// rollouts with a plant table (bmpc_rollout_kernel.inl, PL).
//
// Like stream_disturb: one pass over the kinematic chain of ONE stream, so one lane does the work (`lane`, `nl` as in the neighbours: the other lanes
// of the wave pass through); the caller puts a barrier behind it before other lanes read the record.
// The same text is compiled by g++ for the CPU tests (tests/emu).
#pragma once

#include "bmpc_stream_events.inl"

namespace bmpcs {
// the record of a stream that has taken no plant step: the conventions of stream_audit_init / stream_track_init
BMPC_HD inline void stream_plant_init(double *rec) {
    for (int i = 0; i < bmpcpl::REC_LEN; i++) rec[i] = 0.0;
    rec[bmpcpl::REC_MAX_DU] = -__builtin_inf(); rec[bmpcpl::REC_TICK_DU] = -1.0; rec[bmpcpl::REC_JOINT_DU] = -1.0;
}

// One plant step behind a post that stepped the plant.  row [bmpcpl::LEN]: the stream's row as the caller gave it (a VALID row, bmpc_plant_check; a NaN
// slot takes its identity value here as there); state [bmpcpl::ST_LEN]: in and out; rb: the robot record the post has just stored, c_j = rb[RB_JERK + j]
// the command; rec [bmpcpl::REC_LEN] or NULL: accumulated.  Per joint
//   c' = DELAY ? CMD_j : c_j, CMD_j = c_j;  a = GAIN_j c' + BIAS_j;  f = LAG == 1 ? a : ACT_j + LAG (a - ACT_j), ACT_j = f;  u = clip(f, -SAT, SAT)
// (LAG == 1 is an exact pass-through, a NaN passes the clip), D = u - c_j.  Where any D != 0 the joint state takes the chain's coefficients of D, the
// record's jerk becomes u, and p_lie and v are those of the new joint state (fk_motion, as stream_disturb); where every D == 0 the robot record keeps
// every bit.  Non-finite words give non-finite records.
BMPC_HD inline void stream_plant(double h, const double *row, double *state, double *rb, double *rec, int tick, int lane, int nl) {
    if (lane == 0) {
        double w[bmpcpl::SLOTS];
        for (int k = 0; k < bmpcpl::SLOTS; k++) { const double v = row[k]; w[k] = v != v ? bmpc_plant_identity(k) : v; }
        const double lag = w[bmpcpl::LAG], sat = w[bmpcpl::SAT];
        const bool delay = w[bmpcpl::DELAY] == 1.0;
        double u[7], D[7];
        bool any = false, clipped = false;
        for (int j = 0; j < 7; j++) {
            const double c = rb[RB_JERK + j];
            const double cd = delay ? state[bmpcpl::ST_CMD + j] : c;
            state[bmpcpl::ST_CMD + j] = c;
            const double a = w[bmpcpl::GAIN + j] * cd + w[bmpcpl::BIAS + j];
            const double act = state[bmpcpl::ST_ACT + j];
            const double f = (lag == 1.0) ? a : act + lag * (a - act);
            state[bmpcpl::ST_ACT + j] = f;
            const bool over = f > sat, under = f < -sat;      // (a NaN passes: it is no clip)
            u[j] = over ? sat : (under ? -sat : f);
            clipped = clipped || over || under;
            D[j] = u[j] - c;
            any = any || D[j] != 0.0;
        }
        if (rec) {
            rec[bmpcpl::REC_SAMPLES] += 1.0;
            if (clipped) rec[bmpcpl::REC_N_SAT] += 1.0;
            for (int j = 0; j < 7; j++) {
                const double du = D[j] < 0.0 ? -D[j] : D[j], m = rec[bmpcpl::REC_MAX_DU];
                const bool bad = !(du - du == 0.0);
                if (bad ? m == m : du > m) { rec[bmpcpl::REC_MAX_DU] = bad ? __builtin_nan("") : du; rec[bmpcpl::REC_TICK_DU] = (double)tick; rec[bmpcpl::REC_JOINT_DU] = (double)j; }
                rec[bmpcpl::REC_SUMSQ_DU] += D[j] * D[j];
            }
        }
        if (any) {
            const double k3 = h * h * h / 24, k2 = h * h / 6, k1 = h / 2;
            double q[7], dq[7], ddq[7];
            for (int j = 0; j < 7; j++) { q[j] = rb[RB_Q + j] + k3 * D[j]; dq[j] = rb[RB_DQ + j] + k2 * D[j]; ddq[j] = rb[RB_DDQ + j] + k1 * D[j]; }
            FkMotion M; fk_motion(q, dq, ddq, u, M);
            for (int j = 0; j < 7; j++) { rb[RB_Q + j] = q[j]; rb[RB_DQ + j] = dq[j]; rb[RB_DDQ + j] = ddq[j]; rb[RB_JERK + j] = u[j]; }
            for (int c = 0; c < 6; c++) { rb[RB_P + c] = M.p[c]; rb[RB_V + c] = M.v[c]; }
        }
    }
}

}  // namespace bmpcs
