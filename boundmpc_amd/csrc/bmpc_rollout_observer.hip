// bmpc_rollout_observer.hip -- gfx950 rollout kernels WITH A STATE OBSERVER: the rollout with a sensor model of bmpc_rollout_sensor.hip with a TABLE of state
// estimators per stream -- a correction gain on q, dq and ddq, one step of lead for a sample that is one tick old, an innovation gate -- between the
// sensor's sample and what the pack, the solve and the post of every tick read, which in that rollout IS the noisy sample: "encoder resolution x lag x
// margin x filter" is ONE launch (kernel text and rationale: bmpc_rollout_kernel.inl, OB; the rule of the step: bmpc_stream_observer.inl).  A translation
// unit of its own: four more instantiations of the whole wave program with everything on, compiled beside the others, and the kernels of the other rollout
// units stay the functions they were.  The launch functions are called from the C ABI in bmpc_hip.hip (bmpc_stream_rollout_observer, bmpc_stream_observe).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../include/boundmpc_hip.h"

#include "bmpc_gpu_common.h"
#include "bmpc_wave.inl"
#include "bmpc_stream.inl"

typedef KArgsT<bmpc::Opts> KArgs;

#include "bmpc_rollout_kernel.inl"

static_assert(bmpcob::LQ == BMPC_OBSERVER_LQ && bmpcob::LDQ == BMPC_OBSERVER_LDQ && bmpcob::LDDQ == BMPC_OBSERVER_LDDQ && bmpcob::LEAD == BMPC_OBSERVER_LEAD
              && bmpcob::GATE == BMPC_OBSERVER_GATE && bmpcob::LEN == BMPC_OBSERVER_LEN && bmpcob::SLOTS <= bmpcob::LEN, "row of the header and of the kernel text");
static_assert(bmpcob::ST_POST == BMPC_OBSERVER_STATE_POST && bmpcob::ST_JP == BMPC_OBSERVER_STATE_JP && bmpcob::ST_JL == BMPC_OBSERVER_STATE_JL
              && bmpcob::ST_HAS == BMPC_OBSERVER_STATE_HAS && bmpcob::ST_LAGS == BMPC_OBSERVER_STATE_LAGS && bmpcob::ST_LEN == BMPC_OBSERVER_STATE_LEN,
              "state of the header and of the kernel text");
static_assert(bmpcob::REC_SAMPLES == BMPC_OBSERVER_REC_SAMPLES && bmpcob::REC_N_REJ == BMPC_OBSERVER_REC_N_REJ && bmpcob::REC_MAX_DQ == BMPC_OBSERVER_REC_MAX_DQ
              && bmpcob::REC_TICK_DQ == BMPC_OBSERVER_REC_TICK_DQ && bmpcob::REC_JOINT_DQ == BMPC_OBSERVER_REC_JOINT_DQ && bmpcob::REC_MAX_DP == BMPC_OBSERVER_REC_MAX_DP
              && bmpcob::REC_TICK_DP == BMPC_OBSERVER_REC_TICK_DP && bmpcob::REC_SUMSQ_DQ == BMPC_OBSERVER_REC_SUMSQ_DQ && bmpcob::REC_LEN == BMPC_OBSERVER_REC_LEN,
              "record of the header and of the kernel text");

// The sample and the estimate on their own (bmpc_stream_observe of the C ABI), for per-tick loops: the launch shape of bmpc_stream_sense_kernel, one LANE
// per stream.  An invalid sensor or observer row leaves its mask and touches nothing; a stream without a plan (the tick will skip it) takes no sample and
// makes no estimate, only SAME = 1 is written, as bmpc_stream_sense_kernel does and for its reason.  The way back behind the tick is bmpc_stream_unsense.
__global__ void __launch_bounds__(64) bmpc_stream_observe_kernel(int N, int B, double h, double *rb, const double *ss, const double *sensor, double *state, int *info, double *rec,
                                                                 const double *noise, double *meas, int tick, const double *observer, double *ostate, int *oinfo, double *orec,
                                                                 double *sample) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const double *row = sensor + (long long)b * bmpcse::LEN, *orow = observer + (long long)b * bmpcob::LEN;
    const int bad = bmpc_sensor_check(row, nullptr), obad = bmpc_observer_check(orow, nullptr);
    if (info) info[b] = bad;
    if (oinfo) oinfo[b] = obad;
    if (bad || obad) return;
    if (!(ss[(long long)b * bmpcs::ss_len(N) + bmpcs::SS_ERRCNT] < (double)N)) { state[(long long)b * bmpcse::ST_LEN + bmpcse::ST_SAME] = 1.0; return; }
    bmpcs::stream_observe(h, row, noise ? noise + (long long)b * bmpcs::DIST_LEN : nullptr, state + (long long)b * bmpcse::ST_LEN, orow, ostate + (long long)b * bmpcob::ST_LEN,
                          rb + (long long)b * bmpcs::RB_LEN, rec ? rec + (long long)b * bmpcse::REC_LEN : nullptr, orec ? orec + (long long)b * bmpcob::REC_LEN : nullptr,
                          sample ? sample + (long long)b * bmpcs::DIST_LEN : nullptr, tick, 0, 1);
    if (meas) for (int i = 0; i < bmpcs::RB_LEN; i++) meas[(long long)b * bmpcs::RB_LEN + i] = rb[(long long)b * bmpcs::RB_LEN + i];
}
hipError_t bmpc_stream_observe_launch(int N, int B, double h, double *rb, const double *ss, const double *sensor, double *state, int *info, double *rec, const double *noise,
                                      double *meas, int tick, const double *observer, double *ostate, int *oinfo, double *orec, double *sample, hipStream_t st) {
    hipLaunchKernelGGL(bmpc_stream_observe_kernel, dim3((B + 63) / 64), dim3(64), 0, st, N, B, h, rb, ss, sensor, state, info, rec, noise, meas, tick, observer, ostate, oinfo, orec,
                       sample);
    return hipGetLastError();
}

hipError_t bmpc_rollout_observer_launch(bool zlds, bool resto, const void *kargs, const SArgs *s, const RArgs *r, const NArgs *n, const OArgs *o, int grid, hipStream_t st) {
    bmpc_rollout_observer_run(zlds, resto, kargs, *s, *r, *n, *o, grid, st);
    return hipGetLastError();
}
