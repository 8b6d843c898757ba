// bmpc_rollout_log.hip -- gfx950 rollout kernels WITH THE LOG: the rollout with events and audit of bmpc_rollout_audit.hip with the logging records of
// BoundMPC.step() behind every tick's post -- path reference, tube bounds, position and orientation errors in the path frame, cut to the first stages of
// the plan -- as a row per tick, and a tracking record per stream over stage 0 of those rows (kernel text and rationale: bmpc_rollout_kernel.inl, LG; the
// records themselves: bmpc_stream_log.inl).  A translation unit of its own: four more instantiations of the whole wave program, compiled beside the
// others, and the kernels of bmpc_rollout.hip, bmpc_rollout_events.hip and bmpc_rollout_audit.hip stay the functions they were.  Null event and audit
// pointers switch those off, as they do there.  The launch function is called from the C ABI in bmpc_hip.hip (bmpc_stream_rollout_log).
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

static_assert(bmpcs::TRACK_SAMPLES == BMPC_TRACK_SAMPLES && bmpcs::TRACK_MAX_EP_ORTH == BMPC_TRACK_MAX_EP_ORTH && bmpcs::TRACK_TICK_EP_ORTH == BMPC_TRACK_TICK_EP_ORTH
              && bmpcs::TRACK_SUMSQ_EP_ORTH == BMPC_TRACK_SUMSQ_EP_ORTH && bmpcs::TRACK_MAX_EP_PAR == BMPC_TRACK_MAX_EP_PAR && bmpcs::TRACK_TICK_EP_PAR == BMPC_TRACK_TICK_EP_PAR
              && bmpcs::TRACK_SUMSQ_EP_PAR == BMPC_TRACK_SUMSQ_EP_PAR && bmpcs::TRACK_MAX_ER == BMPC_TRACK_MAX_ER && bmpcs::TRACK_TICK_ER == BMPC_TRACK_TICK_ER
              && bmpcs::TRACK_SUMSQ_ER == BMPC_TRACK_SUMSQ_ER && bmpcs::TRACK_REPLAYED == BMPC_TRACK_REPLAYED && bmpcs::TRACK_LEN == BMPC_TRACK_LEN,
              "tracking slots of the header and of the kernel text");

hipError_t bmpc_rollout_log_launch(bool zlds, bool resto, const void *kargs, const SArgs *s, const RArgs *r, int grid, hipStream_t st) {
    bmpc_rollout_run<true, true, true>(zlds, resto, kargs, *s, *r, grid, st);
    return hipGetLastError();
}
