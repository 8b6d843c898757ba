// bmpc_rollout_sensor.hip -- gfx950 rollout kernels WITH A SENSOR MODEL: the rollout with events, audit, log, the queue, the settings table and the plant
// table of bmpc_rollout_plant.hip with a TABLE of measurement models per stream -- an encoder offset per joint, a quantisation step, noise on q, dq and
// ddq, a sample that is one tick old -- between the true plant and what the pack, the solve and the post of every tick read, which in every other rollout
// IS the plant: "encoder resolution x lag x margin" is ONE launch whose history answers (kernel text and rationale: bmpc_rollout_kernel.inl, SE; the rule
// of the two steps: bmpc_stream_sensor.inl).  A translation unit of its own: four more instantiations of the whole wave program with everything on,
// compiled beside the others, and the kernels of the other rollout units stay the functions they were.  Null event, audit, log, queue, settings and plant
// pointers switch those off, as they do there; the plant table is asked for at run time.  The launch functions are called from the C ABI in bmpc_hip.hip
// (bmpc_stream_rollout_sensor, bmpc_stream_sense, bmpc_stream_unsense).
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

static_assert(bmpcse::BIAS == BMPC_SENSOR_BIAS && bmpcse::RES == BMPC_SENSOR_RES && bmpcse::NQ == BMPC_SENSOR_NQ && bmpcse::NDQ == BMPC_SENSOR_NDQ
              && bmpcse::NDDQ == BMPC_SENSOR_NDDQ && bmpcse::HOLD == BMPC_SENSOR_HOLD && bmpcse::LEN == BMPC_SENSOR_LEN && bmpcse::SLOTS <= bmpcse::LEN && bmpcse::SLOTS <= 31,
              "row of the header and of the kernel text");
static_assert(bmpcse::ST_HELD == BMPC_SENSOR_STATE_HELD && bmpcse::ST_HAS == BMPC_SENSOR_STATE_HAS && bmpcse::ST_SAME == BMPC_SENSOR_STATE_SAME
              && bmpcse::ST_TRUTH == BMPC_SENSOR_STATE_TRUTH && bmpcse::ST_LEN == BMPC_SENSOR_STATE_LEN, "state of the header and of the kernel text");
static_assert(bmpcse::REC_SAMPLES == BMPC_SENSOR_REC_SAMPLES && bmpcse::REC_MAX_DQ == BMPC_SENSOR_REC_MAX_DQ && bmpcse::REC_TICK_DQ == BMPC_SENSOR_REC_TICK_DQ
              && bmpcse::REC_JOINT_DQ == BMPC_SENSOR_REC_JOINT_DQ && bmpcse::REC_MAX_DP == BMPC_SENSOR_REC_MAX_DP && bmpcse::REC_TICK_DP == BMPC_SENSOR_REC_TICK_DP
              && bmpcse::REC_SUMSQ_DQ == BMPC_SENSOR_REC_SUMSQ_DQ && bmpcse::REC_LEN == BMPC_SENSOR_REC_LEN, "record of the header and of the kernel text");

// The two steps on their own (bmpc_stream_sense, bmpc_stream_unsense of the C ABI), for per-tick loops: one LANE per stream, as the plant kernel.  The
// sample: an invalid row leaves its mask and touches nothing; a stream without a plan (the tick will skip it) takes no sample and only SAME = 1 is
// written, which tells the way back to leave the record alone -- behind the tick the error count alone cannot tell such a stream from one whose post has
// just exhausted the plan, and that one wants its truth back.  (Inside a rollout a stream without a plan has stopped.)  The way back reads the state.
__global__ void __launch_bounds__(64) bmpc_stream_sense_kernel(int N, int B, double *rb, const double *ss, const double *sensor, double *state, int *info, double *rec,
                                                               const double *noise, double *meas, int tick) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const double *row = sensor + (long long)b * bmpcse::LEN;
    const int bad = bmpc_sensor_check(row, nullptr);
    if (info) info[b] = bad;
    if (bad) return;
    if (!(ss[(long long)b * bmpcs::ss_len(N) + bmpcs::SS_ERRCNT] < (double)N)) { state[(long long)b * bmpcse::ST_LEN + bmpcse::ST_SAME] = 1.0; return; }
    bmpcs::stream_sense(row, noise ? noise + (long long)b * bmpcs::DIST_LEN : nullptr, state + (long long)b * bmpcse::ST_LEN, rb + (long long)b * bmpcs::RB_LEN,
                        rec ? rec + (long long)b * bmpcse::REC_LEN : nullptr, tick, 0, 1);
    if (meas) for (int i = 0; i < bmpcs::RB_LEN; i++) meas[(long long)b * bmpcs::RB_LEN + i] = rb[(long long)b * bmpcs::RB_LEN + i];
}
// (one WORKGROUP per stream, lane 0 of it at work, as the splice kernel of bmpc_hip.hip: with a stream per lane the register allocator of this toolchain
// stops with a fault on this function under the build's scheduler flag; the grid is B)
__global__ void __launch_bounds__(64) bmpc_stream_unsense_kernel(int N, int B, double h, double *rb, const double *ss, const double *sensor, const double *state) {
    const int b = blockIdx.x;
    if (b >= B) return;
    if (bmpc_sensor_check(sensor + (long long)b * bmpcse::LEN, nullptr)) return;
    bmpcs::stream_truth(h, state + (long long)b * bmpcse::ST_LEN, rb + (long long)b * bmpcs::RB_LEN, ss[(long long)b * bmpcs::ss_len(N) + bmpcs::SS_ERRCNT] < (double)N, threadIdx.x, 64);
}
hipError_t bmpc_stream_sense_launch(int N, int B, double *rb, const double *ss, const double *sensor, double *state, int *info, double *rec, const double *noise, double *meas,
                                    int tick, hipStream_t st) {
    hipLaunchKernelGGL(bmpc_stream_sense_kernel, dim3((B + 63) / 64), dim3(64), 0, st, N, B, rb, ss, sensor, state, info, rec, noise, meas, tick);
    return hipGetLastError();
}
hipError_t bmpc_stream_unsense_launch(int N, int B, double h, double *rb, const double *ss, const double *sensor, const double *state, hipStream_t st) {
    hipLaunchKernelGGL(bmpc_stream_unsense_kernel, dim3(B), dim3(64), 0, st, N, B, h, rb, ss, sensor, state);
    return hipGetLastError();
}

hipError_t bmpc_rollout_sensor_launch(bool zlds, bool resto, const void *kargs, const SArgs *s, const RArgs *r, const NArgs *n, int grid, hipStream_t st) {
    bmpc_rollout_sensor_run(zlds, resto, kargs, *s, *r, *n, grid, st);
    return hipGetLastError();
}
