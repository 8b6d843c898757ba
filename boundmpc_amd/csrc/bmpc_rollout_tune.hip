// bmpc_rollout_tune.hip -- gfx950 rollout kernels FOR SWEEPS: the rollout with events, audit, log and the queue of bmpc_rollout_legs.hip with a TABLE of
// controller settings per stream -- iteration cap, tolerance, barrier start and hold, level rule, acceptance threshold and position-row cap,
// joint-limit margin, stall window -- in the place of the one set the handle carries for a whole launch: a grid over settings, or a robustness
// battery with its own margin per stream, is ONE launch of as many streams (kernel text and rationale: bmpc_rollout_kernel.inl, TU).  A translation
// unit of its own: four more instantiations of the whole wave program with everything on, compiled beside the others, and the kernels of the other
// rollout units stay the functions they were.  Null event, audit, log and queue pointers switch those off, as they do there.  The launch function is
// called from the C ABI in bmpc_hip.hip (bmpc_stream_rollout_tuned).
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

static_assert(bmpctu::MAX_ITER == BMPC_TUNE_MAX_ITER && bmpctu::TOL == BMPC_TUNE_TOL && bmpctu::MU_INIT == BMPC_TUNE_MU_INIT && bmpctu::MU_WARM == BMPC_TUNE_MU_WARM
              && bmpctu::MU_MIN_FAC == BMPC_TUNE_MU_MIN_FAC && bmpctu::SLACK_PUSH == BMPC_TUNE_SLACK_PUSH && bmpctu::BOUND_MARGIN == BMPC_TUNE_BOUND_MARGIN
              && bmpctu::HOLD == BMPC_TUNE_HOLD && bmpctu::LVL_C == BMPC_TUNE_LVL_C && bmpctu::LVL_LO == BMPC_TUNE_LVL_LO && bmpctu::LVL_HI == BMPC_TUNE_LVL_HI
              && bmpctu::RT_TOL == BMPC_TUNE_RT_TOL && bmpctu::RT_ROW_CAP == BMPC_TUNE_RT_ROW_CAP && bmpctu::STALL_WINDOW == BMPC_TUNE_STALL_WINDOW
              && bmpctu::LEN == BMPC_TUNE_LEN && bmpctu::SLOTS <= bmpctu::CROSS && bmpctu::CROSS < bmpctu::LEN, "slots of the header and of the kernel text");

hipError_t bmpc_rollout_tune_launch(bool zlds, bool resto, const void *kargs, const SArgs *s, const RArgs *r, int grid, hipStream_t st) {
    bmpc_rollout_run<true, true, true, true, true>(zlds, resto, kargs, *s, *r, grid, st);
    return hipGetLastError();
}
