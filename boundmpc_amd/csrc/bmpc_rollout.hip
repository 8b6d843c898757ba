// bmpc_rollout.hip -- gfx950 rollout kernels of the batched BoundMPC OCP solver: `ticks` closed-loop ticks {pack, solve, post} of every stream in
// ONE launch, one wave per stream, each stream at its own pace (kernel text and rationale: bmpc_rollout_kernel.inl).  A translation unit of its
// own for the reason bmpc_tick.hip is one: the kernel exists with and without the restoration phase in the solver (RESTO), for both placements of
// the iterate (ZLDS) -- four instantiations of the whole wave program.  The launch function is called from the C ABI in bmpc_hip.hip.
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

static_assert(bmpcs::RH_ROBOT == BMPC_ROLL_ROBOT && bmpcs::RH_PHI == BMPC_ROLL_PHI && bmpcs::RH_ERRCNT == BMPC_ROLL_ERRCNT && bmpcs::RH_ITERS == BMPC_ROLL_ITERS
              && bmpcs::RH_STATUS == BMPC_ROLL_STATUS && bmpcs::RH_KKT == BMPC_ROLL_KKT && bmpcs::RH_NVALID == BMPC_ROLL_NVALID
              && bmpcs::RH_USINGPREV == BMPC_ROLL_USINGPREV && bmpcs::RH_SUCCESS == BMPC_ROLL_SUCCESS && bmpcs::RH_GVIOL == BMPC_ROLL_GVIOL
              && bmpcs::RH_LEN == BMPC_ROLL_LEN, "history slots of the header and of the kernel text");

hipError_t bmpc_rollout_launch(bool zlds, bool resto, const void *kargs, const SArgs *s, const RArgs *r, int grid, hipStream_t st) {
    bmpc_rollout_run<false, false, false>(zlds, resto, kargs, *s, *r, grid, st);
    return hipGetLastError();
}
