// bmpc_rollout_events.hip -- gfx950 rollout kernels WITH EVENTS: the rollout of bmpc_rollout.hip with a plant disturbance per tick and one scheduled
// re-plan per stream (measured state spliced in on the device) behind the tick's post (kernel text and rationale: bmpc_rollout_kernel.inl, EV).  A
// translation unit of its own: four more instantiations of the whole wave program, compiled beside the others, and the kernels of bmpc_rollout.hip
// stay the functions they were.  The launch function is called from the C ABI in bmpc_hip.hip (bmpc_stream_rollout_events).
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

static_assert(bmpcs::DIST_LEN == BMPC_DIST_LEN, "disturbance row of the header and of the kernel text");

hipError_t bmpc_rollout_events_launch(bool zlds, bool resto, const void *kargs, const SArgs *s, const RArgs *r, int grid, hipStream_t st) {
    bmpc_rollout_run<true, false, false>(zlds, resto, kargs, *s, *r, grid, st);
    return hipGetLastError();
}
