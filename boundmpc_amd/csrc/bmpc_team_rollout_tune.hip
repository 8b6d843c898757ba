// bmpc_team_rollout_tune.hip -- gfx950 TEAM rollout kernels FOR SWEEPS: the fully-featured team rollout of bmpc_team_rollout_legs.hip with the table of
// controller settings per stream of bmpc_rollout_tune.hip (kernel text and rationale: bmpc_rollout_kernel.inl, TU and TEAMS -- every wave of the team
// validates and resolves the stream's row itself, from the read-only table and the kernel arguments).  A translation unit of its own: two more
// instantiations of the whole team program, with and without the restoration phase, compiled beside the others; the kernels of bmpc_team_rollout.hip
// and bmpc_team_rollout_legs.hip stay the functions they were.  The launch function is called from the C ABI in bmpc_hip.hip
// (bmpc_stream_rollout_tuned under bmpc_set_rollout_waves).
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

hipError_t bmpc_team_rollout_tune_launch(int nw, bool resto, const void *kargs, const SArgs *s, const RArgs *r, int grid, hipStream_t st) {
    if (nw != BMPC_NW) return hipErrorInvalidValue;
    bmpc_rollout_run<true, true, true, true, true>(true, resto, kargs, *s, *r, grid, st);
    return hipGetLastError();
}
