// bmpc_team_rollout.hip -- gfx950 TEAM rollout kernels: the rollout of bmpc_rollout.hip (`ticks` closed-loop ticks of every stream in ONE launch, each
// stream at its own pace) on a workgroup of BMPC_NW cooperating waves per stream.  The kernel text is bmpc_rollout_kernel.inl, compiled as bmpc_team.hip
// compiles the fused tick's: BMPC_NW waves, namespace bmpct, iterate in LDS, one team per CU -- wave 0 packs, posts, stores the rows and runs the
// events, the audit and the log, the workgroup solves.  Workgroup w serves streams w, w + grid, ... on workspace slab w (grid = min(B, resident teams)).
// A translation unit of its own: four instantiations of the whole team program -- with and without the restoration phase (RESTO), each plain and
// with EV, AU and LG all on; the fully-featured kernel serves the events, audit and log entries alike (a dormant event, audit or log line costs
// 0.1-0.8 % of a tick; the two middle variants are not built).  The launch function is called from the C ABI in bmpc_hip.hip.
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

hipError_t bmpc_team_rollout_launch(int nw, bool resto, bool full, const void *kargs, const SArgs *s, const RArgs *r, int grid, hipStream_t st) {
    if (nw != BMPC_NW) return hipErrorInvalidValue;
    if (full) bmpc_rollout_run<true, true, true>(true, resto, kargs, *s, *r, grid, st);
    else bmpc_rollout_run<false, false, false>(true, resto, kargs, *s, *r, grid, st);
    return hipGetLastError();
}
