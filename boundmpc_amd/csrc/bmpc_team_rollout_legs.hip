// bmpc_team_rollout_legs.hip -- gfx950 TEAM rollout kernels WITH A MISSION: the fully-featured team rollout of bmpc_team_rollout.hip with the queue
// of re-plan records per stream of bmpc_rollout_legs.hip (kernel text and rationale: bmpc_rollout_kernel.inl, QU and TEAMS -- every wave of the team
// takes the trigger decision itself, from memory that is constant between two barriers).  A translation unit of its own: two more instantiations of
// the whole team program, with and without the restoration phase, compiled beside the others; the kernels of bmpc_team_rollout.hip stay the functions
// they were.  The launch function is called from the C ABI in bmpc_hip.hip (bmpc_stream_rollout_legs under bmpc_set_rollout_waves).
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

hipError_t bmpc_team_rollout_legs_launch(int nw, bool resto, const void *kargs, const SArgs *s, const RArgs *r, int grid, hipStream_t st) {
    if (nw != BMPC_NW) return hipErrorInvalidValue;
    bmpc_rollout_run<true, true, true, true>(true, resto, kargs, *s, *r, grid, st);
    return hipGetLastError();
}
