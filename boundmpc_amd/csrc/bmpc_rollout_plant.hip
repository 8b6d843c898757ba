// bmpc_rollout_plant.hip -- gfx950 rollout kernels WITH A PLANT MODEL: the rollout with events, audit, log, the queue and the settings table of
// bmpc_rollout_tune.hip with a TABLE of actuator models per stream -- gain and offset per joint, a first-order lag, a clip, one tick of dead time --
// between the first planned jerk of every tick and the plant, which in every other rollout IS the model: "gain error x lag x margin" is ONE launch
// whose audit answers (kernel text and rationale: bmpc_rollout_kernel.inl, PL; the rule of the step: bmpc_stream_plant.inl).  A translation unit of its
// own: four more instantiations of the whole wave program with everything on, compiled beside the others, and the kernels of the other rollout units
// stay the functions they were.  Null event, audit, log, queue and settings pointers switch those off, as they do there.  The launch function is called
// from the C ABI in bmpc_hip.hip (bmpc_stream_rollout_plant).
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

static_assert(bmpcpl::GAIN == BMPC_PLANT_GAIN && bmpcpl::BIAS == BMPC_PLANT_BIAS && bmpcpl::LAG == BMPC_PLANT_LAG && bmpcpl::SAT == BMPC_PLANT_SAT
              && bmpcpl::DELAY == BMPC_PLANT_DELAY && bmpcpl::LEN == BMPC_PLANT_LEN && bmpcpl::SLOTS <= bmpcpl::LEN && bmpcpl::SLOTS <= 31, "row of the header and of the kernel text");
static_assert(bmpcpl::ST_ACT == BMPC_PLANT_STATE_ACT && bmpcpl::ST_CMD == BMPC_PLANT_STATE_CMD && bmpcpl::ST_LEN == BMPC_PLANT_STATE_LEN, "state of the header and of the kernel text");
static_assert(bmpcpl::REC_SAMPLES == BMPC_PLANT_REC_SAMPLES && bmpcpl::REC_N_SAT == BMPC_PLANT_REC_N_SAT && bmpcpl::REC_MAX_DU == BMPC_PLANT_REC_MAX_DU
              && bmpcpl::REC_TICK_DU == BMPC_PLANT_REC_TICK_DU && bmpcpl::REC_JOINT_DU == BMPC_PLANT_REC_JOINT_DU && bmpcpl::REC_SUMSQ_DU == BMPC_PLANT_REC_SUMSQ_DU
              && bmpcpl::REC_LEN == BMPC_PLANT_REC_LEN, "record of the header and of the kernel text");

// The step on its own (bmpc_stream_plant of the C ABI), for per-tick loops: one LANE per stream, as the disturbance kernel; a stream without a plan (the
// post did not step its plant) is skipped, an invalid row leaves its mask and touches nothing.  In this unit, as the tube kernel lives in the audit's: the
// device text of bmpc_hip.hip is not touched by it.
__global__ void __launch_bounds__(64) bmpc_stream_plant_kernel(int N, int B, double h, double *rb, const double *ss, const double *plant, double *state, int *info, double *rec,
                                                               int tick) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const double *row = plant + (long long)b * bmpcpl::LEN;
    const int bad = bmpc_plant_check(row, nullptr);
    if (info) info[b] = bad;
    if (bad || !(ss[(long long)b * bmpcs::ss_len(N) + bmpcs::SS_ERRCNT] < (double)N)) return;
    bmpcs::stream_plant(h, row, state + (long long)b * bmpcpl::ST_LEN, rb + (long long)b * bmpcs::RB_LEN, rec ? rec + (long long)b * bmpcpl::REC_LEN : nullptr, tick, 0, 1);
}
hipError_t bmpc_stream_plant_launch(int N, int B, double h, double *rb, const double *ss, const double *plant, double *state, int *info, double *rec, int tick, hipStream_t st) {
    hipLaunchKernelGGL(bmpc_stream_plant_kernel, dim3((B + 63) / 64), dim3(64), 0, st, N, B, h, rb, ss, plant, state, info, rec, tick);
    return hipGetLastError();
}

hipError_t bmpc_rollout_plant_launch(bool zlds, bool resto, const void *kargs, const SArgs *s, const RArgs *r, int grid, hipStream_t st) {
    bmpc_rollout_run<true, true, true, true, true, true>(zlds, resto, kargs, *s, *r, grid, st);
    return hipGetLastError();
}
