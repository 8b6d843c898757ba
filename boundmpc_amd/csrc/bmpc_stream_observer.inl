// bmpc_stream_observer.inl -- a STATE OBSERVER between the sample of a closed-loop stream's sensor and its controller, as device code: a predictor-corrector
// on the model's own jerk-integrator chain.  The sensor (bmpc_stream_sensor.inl) hands its sample straight to the pack: offsets, quantisation and noise on
// q, dq and ddq, and under HOLD a sample that is one tick old.  Here the sample corrects a prediction instead of replacing the record: the last posterior
// is advanced with the jerk the record carries (chain_step, the step stream_post and stream_truth take), the sample pulls it by a gain per derivative, a
// sample too far from the prediction is rejected, and a sample that is one tick old is compared with the prediction of ITS time and the corrected estimate
// advanced one more step (LEAD): the sensor's hold can be compensated, not only studied as damage.  Host mirror and specification:
// boundmpc_amd.stream.observe_robot.  Included behind bmpc_stream_sensor.inl; used by the observer kernel of bmpc_rollout_observer.hip
// (bmpc_stream_observe) and by the rollouts with an observer table (bmpc_rollout_kernel.inl, OB).  The way back to the truth behind the post is the
// sensor's, stream_truth: it reads SAME and TRUTH of the sensor state, which stream_observe leaves as stream_sense does.
// KNOWN BLIND SPOT: the observer sees the record's jerk and the samples, nothing else.  A disturbance of the plant, a spliced re-plan and a post that
// exhausted the plan (the plant then did not step) are not announced to it: its prediction is off by what happened and the innovation pulls it back over
// the next samples, as a real filter's would.  The state is NOT reset on any of them.
//
// Like stream_sense: one pass of ONE stream, so one lane does the work (`lane`, `nl` as in the neighbours); the caller puts a barrier behind it before
// other lanes read the record.  The same text is compiled by g++ for the CPU tests (tests/emu).
#pragma once

#include "bmpc_stream_sensor.inl"

namespace bmpcs {
static_assert(bmpcob::ST_LAGS < bmpcob::ST_LEN && bmpcob::ST_JP == DIST_LEN && bmpcob::ST_JL == bmpcob::ST_JP + 7 && bmpcob::ST_HAS == bmpcob::ST_JL + 7, "the observer's state");

// the record of a stream that has made no estimate: the conventions of stream_sensor_init
BMPC_HD inline void stream_observer_init(double *rec) {
    for (int i = 0; i < bmpcob::REC_LEN; i++) rec[i] = 0.0;
    rec[bmpcob::REC_MAX_DQ] = -__builtin_inf(); rec[bmpcob::REC_TICK_DQ] = -1.0; rec[bmpcob::REC_JOINT_DQ] = -1.0;
    rec[bmpcob::REC_MAX_DP] = -__builtin_inf(); rec[bmpcob::REC_TICK_DP] = -1.0;
}

// one chain step of the 21 words x (q 7 | dq 7 | ddq 7) from the jerk up to the jerk u, per joint with the handle's h
BMPC_HD inline void observer_step(const double *x, const double *up, const double *u, double h, double *y) {
    for (int j = 0; j < 7; j++) {
        double a = x[j], da = x[7 + j], dda = x[14 + j];
        chain_step(a, da, dda, up[j], u[j], h);
        y[j] = a; y[7 + j] = da; y[14 + j] = dda;
    }
}

// The sample of tick `tick` AND the estimate made from it, ahead of the tick's pack and behind the lost-plan test: stream_sense with the observer between
// the sample and the record.  row, noise, state, rb, rec: the arguments of stream_sense with their meaning -- the sample's arithmetic is that function's,
// word for word (tests/test_stream_rollout_observer.py holds the two to each other bit for bit), and `rec` keeps describing the SAMPLE against the truth.
// orow [bmpcob::LEN]: the stream's observer row as the caller gave it (a VALID row, bmpc_observer_check; a NaN slot takes its identity value here as
// there); ostate [bmpcob::ST_LEN]: in and out; orec [bmpcob::REC_LEN] or NULL: accumulated, the ESTIMATE against the truth; sample [DIST_LEN] or NULL: the
// raw sample.  With m the sample (behind the sensor's HOLD), J = rb[RB_JERK] and step(x, up, u) = chain_step per joint:
//   fresh (HAS == 0)   post = out = m;  POST = m, JP = JL = J, HAS = 1, LAGS = 0; no gate
//   LEAD == 0          prior = step(POST, JP, J);  post = prior + L (m - prior), the word m itself where L == 1; a rejected sample: post = prior;
//                      out = post;  POST = post, JP = JL = J, LAGS = 0
//   LEAD == 1          prior = LAGS ? step(POST, JP, JL) : POST (the sample's own time);  post as above;  out = step(post, LAGS ? JL : JP, J);
//                      POST = post, where LAGS was 1 JP = the old JL, then JL = J, LAGS = 1
//   rejected: any |m_q,j - prior_q,j| not <= GATE (a NaN is rejected)
// SAME of the sensor state is decided on out against the truth, over all 21 words.  Where it is 0 the record's q, dq, ddq become out and p_lie and v are
// those of out (fk_motion with the record's jerk: one kinematics pass); where it is 1 the record keeps every bit.  A second pass is taken only for the
// position word of `rec`, where `rec` is given and the sample differs from the truth and from the estimate.
// NOT INLINED on the device: a function of its own, called by the kernels.  Inlined into the team rollout kernel with the restoration phase, its lane-0
// section (five arrays of 21 words and a kinematics pass) pushed one of that kernel's scalar-spill registers into an accumulator register, and the copies
// back -- whole-wave copies, at a join inside the solve and at the join behind the tick loop -- carry the signature the build's ISA lint refuses.  Tried on
// that kernel: one validation block and one loop for the rows not run (bmpc_rollout_body.inl), the scalar form of the argument pointers, loops kept rolled:
// both copies stay.  The call alone: the copy inside the solve goes, the one behind the tick loop stays.  The call with the one validation block and the one
// loop: both lints pass on both units, and that is what is built.  The call sits between two solves; it is made by wave 0 alone, with all its lanes on.
#ifndef BMPC_EMU
#define BMPC_OBSERVE_NOINLINE __attribute__((noinline))
#else
#define BMPC_OBSERVE_NOINLINE
#endif
BMPC_OBSERVE_NOINLINE BMPC_HD inline void stream_observe(double h, const double *row, const double *noise, double *state, const double *orow, double *ostate, double *rb, double *rec, double *orec,
                                   double *sample, int tick, int lane, int nl) {
    if (lane == 0) {
        // ---- the sample: stream_sense's lines ----
        double w[bmpcse::SLOTS];
        for (int k = 0; k < bmpcse::SLOTS; k++) { const double v = row[k]; w[k] = v != v ? bmpc_sensor_identity(k) : v; }
        for (int i = 0; i < RB_XPHID; i++) state[bmpcse::ST_TRUTH + i] = rb[i];
        for (int j = 0; j < 7; j++) state[bmpcse::ST_TRUTH + RB_XPHID + j] = rb[RB_JERK + j];
        const double res = w[bmpcse::RES];
        const bool held = w[bmpcse::HOLD] == 1.0 && state[bmpcse::ST_HAS] == 1.0;
        double smp[DIST_LEN];
        bool same_s = true;
        for (int i = 0; i < DIST_LEN; i++) {
            const int j = i % 7;
            double ni = noise ? noise[i] : 0.0;
            ni = (ni - ni == 0.0) ? ni : 0.0;
            double m;
            if (i < 7) {
                m = (rb[RB_Q + j] + w[bmpcse::BIAS + j]) + w[bmpcse::NQ] * ni;
                if (res > 0.0) m = res * __builtin_rint(m / res);
            } else m = rb[RB_Q + i] + w[i < 14 ? bmpcse::NDQ : bmpcse::NDDQ] * ni;
            smp[i] = held ? state[bmpcse::ST_HELD + i] : m;
            state[bmpcse::ST_HELD + i] = m;
            same_s = same_s && smp[i] == rb[RB_Q + i];
        }
        state[bmpcse::ST_HAS] = 1.0;
        if (sample) for (int i = 0; i < DIST_LEN; i++) sample[i] = smp[i];
        // ---- the estimate ----
        double o[bmpcob::SLOTS], J[7];
        for (int k = 0; k < bmpcob::SLOTS; k++) { const double v = orow[k]; o[k] = v != v ? bmpc_observer_identity(k) : v; }
        for (int j = 0; j < 7; j++) J[j] = rb[RB_JERK + j];
        double est[DIST_LEN];
        bool rejected = false;
        if (!(ostate[bmpcob::ST_HAS] == 1.0)) {
            for (int i = 0; i < DIST_LEN; i++) { est[i] = smp[i]; ostate[bmpcob::ST_POST + i] = smp[i]; }
            for (int j = 0; j < 7; j++) { ostate[bmpcob::ST_JP + j] = J[j]; ostate[bmpcob::ST_JL + j] = J[j]; }
            ostate[bmpcob::ST_HAS] = 1.0; ostate[bmpcob::ST_LAGS] = 0.0;
        } else {
            const bool lead = o[bmpcob::LEAD] == 1.0, lags = ostate[bmpcob::ST_LAGS] == 1.0;
            double prior[DIST_LEN], post[DIST_LEN], jl[7];
            for (int j = 0; j < 7; j++) jl[j] = ostate[bmpcob::ST_JL + j];
            if (lead && !lags) { for (int i = 0; i < DIST_LEN; i++) prior[i] = ostate[bmpcob::ST_POST + i]; }
            else observer_step(ostate + bmpcob::ST_POST, ostate + bmpcob::ST_JP, lead ? jl : J, h, prior);
            for (int j = 0; j < 7; j++) {
                const double d = smp[j] - prior[j], ad = d < 0.0 ? -d : d;
                rejected = rejected || !(ad <= o[bmpcob::GATE]);
            }
            for (int i = 0; i < DIST_LEN; i++) {
                const double L = o[i < 7 ? bmpcob::LQ : i < 14 ? bmpcob::LDQ : bmpcob::LDDQ];
                post[i] = rejected ? prior[i] : (L == 1.0) ? smp[i] : prior[i] + L * (smp[i] - prior[i]);
            }
            if (!lead) {
                for (int i = 0; i < DIST_LEN; i++) est[i] = post[i];
                for (int j = 0; j < 7; j++) { ostate[bmpcob::ST_JP + j] = J[j]; ostate[bmpcob::ST_JL + j] = J[j]; }
                ostate[bmpcob::ST_LAGS] = 0.0;
            } else {
                double from[7];
                for (int j = 0; j < 7; j++) from[j] = lags ? jl[j] : ostate[bmpcob::ST_JP + j];
                observer_step(post, from, J, h, est);
                for (int j = 0; j < 7; j++) { if (lags) ostate[bmpcob::ST_JP + j] = jl[j]; ostate[bmpcob::ST_JL + j] = J[j]; }
                ostate[bmpcob::ST_LAGS] = 1.0;
            }
            for (int i = 0; i < DIST_LEN; i++) ostate[bmpcob::ST_POST + i] = post[i];
        }
        // ---- the estimate in the place of the sample ----
        bool same = true, s_is_e = true;
        for (int i = 0; i < DIST_LEN; i++) { same = same && est[i] == rb[RB_Q + i]; s_is_e = s_is_e && smp[i] == est[i]; }
        state[bmpcse::ST_SAME] = same ? 1.0 : 0.0;
        double dqs[7], dqe[7], tp[3], dp[2] = {0.0, 0.0};      // dp: [0] the estimate's, [1] the sample's
        for (int j = 0; j < 7; j++) { dqs[j] = smp[j] - rb[RB_Q + j]; dqe[j] = est[j] - rb[RB_Q + j]; }
        for (int c = 0; c < 3; c++) tp[c] = rb[RB_P + c];
        const bool second = rec && !same_s && !s_is_e;
        for (int pass = 0; pass < 2; pass++) {
            if (pass == 0 ? same : !second) continue;
            const double *x = pass == 0 ? est : smp;
            FkMotion M; fk_motion(x, x + 7, x + 14, J, M);
            double s2 = 0.0;
            for (int c = 0; c < 3; c++) { const double e = M.p[c] - tp[c]; s2 += e * e; }
            dp[pass] = BMPC_SQRT(s2);
            if (pass == 0) {
                for (int i = 0; i < DIST_LEN; i++) rb[RB_Q + i] = est[i];
                for (int c = 0; c < 6; c++) { rb[RB_P + c] = M.p[c]; rb[RB_V + c] = M.v[c]; }
            }
        }
        if (!same_s && s_is_e) dp[1] = dp[0];
        for (int k = 0; k < 2; k++) {
            double *rc = k == 0 ? rec : orec;
            if (!rc) continue;
            // (the two records have their counters in other places and the words from MAX_DQ on in the same order)
            double *mx = rc + (k == 0 ? (int)bmpcse::REC_MAX_DQ : (int)bmpcob::REC_MAX_DQ);
            const double *dq = k == 0 ? dqs : dqe;
            const double dpk = dp[1 - k];
            rc[0] += 1.0;
            if (k == 1 && rejected) rc[bmpcob::REC_N_REJ] += 1.0;
            for (int j = 0; j < 7; j++) {
                const double e = dq[j] < 0.0 ? -dq[j] : dq[j], m = mx[0];
                const bool bad = !(e - e == 0.0);
                if (bad ? m == m : e > m) { mx[0] = bad ? __builtin_nan("") : e; mx[1] = (double)tick; mx[2] = (double)j; }
                mx[5] += dq[j] * dq[j];
            }
            const double m = mx[3];
            const bool bad = !(dpk - dpk == 0.0);
            if (bad ? m == m : dpk > m) { mx[3] = bad ? __builtin_nan("") : dpk; mx[4] = (double)tick; }
        }
    }
}
static_assert(bmpcse::REC_SAMPLES == 0 && bmpcob::REC_SAMPLES == 0 && bmpcse::REC_TICK_DQ == bmpcse::REC_MAX_DQ + 1 && bmpcse::REC_JOINT_DQ == bmpcse::REC_MAX_DQ + 2
              && bmpcse::REC_MAX_DP == bmpcse::REC_MAX_DQ + 3 && bmpcse::REC_TICK_DP == bmpcse::REC_MAX_DQ + 4 && bmpcse::REC_SUMSQ_DQ == bmpcse::REC_MAX_DQ + 5
              && bmpcob::REC_TICK_DQ == bmpcob::REC_MAX_DQ + 1 && bmpcob::REC_JOINT_DQ == bmpcob::REC_MAX_DQ + 2 && bmpcob::REC_MAX_DP == bmpcob::REC_MAX_DQ + 3
              && bmpcob::REC_TICK_DP == bmpcob::REC_MAX_DQ + 4 && bmpcob::REC_SUMSQ_DQ == bmpcob::REC_MAX_DQ + 5, "the two records from MAX_DQ on");

}  // namespace bmpcs
