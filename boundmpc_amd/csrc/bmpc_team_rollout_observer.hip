// bmpc_team_rollout_observer.hip -- gfx950 TEAM rollout kernels WITH A STATE OBSERVER: the team rollout with a sensor model of bmpc_team_rollout_sensor.hip
// with the table of state estimators per stream of bmpc_rollout_observer.hip (kernel text and rationale: bmpc_rollout_kernel.inl, OB and TEAMS -- every wave
// of the team validates the stream's rows itself and reads SAME and the error count behind the post's barrier itself; wave 0 takes the sample, makes the
// estimate and takes the way back).  A translation unit of its own: two more instantiations of the whole team program, with and without the restoration
// phase, compiled beside the others; the kernels of the other team rollout units stay the functions they were.  The launch function is called from the C
// ABI in bmpc_hip.hip (bmpc_stream_rollout_observer under bmpc_set_rollout_waves).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>

#ifndef BMPC_NW
#define BMPC_NW 4
#endif
#define BMPC_NAMESPACE bmpct
#include "bmpc_gpu_common.h"
#include "bmpc_wave.inl"
#include "bmpc_stream.inl"

typedef KArgsT<bmpct::Opts> KArgs;
static_assert(bmpct::NW == BMPC_NW, "team size");

#include "bmpc_rollout_kernel.inl"

hipError_t bmpc_team_rollout_observer_launch(int nw, bool resto, const void *kargs, const SArgs *s, const RArgs *r, const NArgs *n, const OArgs *o, int grid, hipStream_t st) {
    if (nw != BMPC_NW) return hipErrorInvalidValue;
    bmpc_rollout_observer_run(true, resto, kargs, *s, *r, *n, *o, grid, st);
    return hipGetLastError();
}
