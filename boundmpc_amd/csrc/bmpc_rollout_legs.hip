// bmpc_rollout_legs.hip -- gfx950 rollout kernels WITH A MISSION: the rollout with events, audit and log of bmpc_rollout_log.hip with a QUEUE of
// re-plan records per stream in the place of the one scheduled record, each record fired by a tick number, by the goal of the leg the stream is on or
// by a lost plan -- task sequences and recovery policies inside ONE launch, every stream at its own pace (kernel text and rationale:
// bmpc_rollout_kernel.inl, QU).  A translation unit of its own: four more instantiations of the whole wave program with everything on, compiled beside
// the others, and the kernels of the other rollout units stay the functions they were.  Null event, audit and log pointers switch those off, as they
// do there.  The launch function is called from the C ABI in bmpc_hip.hip (bmpc_stream_rollout_legs).
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

static_assert(bmpcs::LEG_AT_GOAL == BMPC_LEG_AT_GOAL && bmpcs::LEG_ON_LOST == BMPC_LEG_ON_LOST && bmpcs::LEG_WHY_GOAL == BMPC_LEG_WHY_GOAL
              && bmpcs::LEG_WHY_LOST == BMPC_LEG_WHY_LOST && bmpcs::LEG_WHY_TICK == BMPC_LEG_WHY_TICK, "trigger bits of the header and of the kernel text");

hipError_t bmpc_rollout_legs_launch(bool zlds, bool resto, const void *kargs, const SArgs *s, const RArgs *r, int grid, hipStream_t st) {
    bmpc_rollout_run<true, true, true, true>(zlds, resto, kargs, *s, *r, grid, st);
    return hipGetLastError();
}
