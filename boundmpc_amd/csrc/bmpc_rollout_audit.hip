// bmpc_rollout_audit.hip -- gfx950 rollout kernels WITH THE AUDIT: the rollout with events of bmpc_rollout_events.hip with the tube and joint-limit
// excess of the state every tick starts from, as a row per tick and a verdict per stream (kernel text and rationale: bmpc_rollout_kernel.inl, AU;
// the measurement itself: bmpc_stream_tube.inl).  A translation unit of its own: four more instantiations of the whole wave program, compiled beside
// the others, and the kernels of bmpc_rollout.hip and bmpc_rollout_events.hip stay the functions they were.  Null event pointers switch the events
// off, as they do there.  The service kernel of the measurement on its own (bmpc_stream_tube) is compiled here too, beside the only other device code
// that runs its text: a kernel added to bmpc_hip.hip moves the code generation of the batch kernels compiled in that unit.  The launch functions are
// called from the C ABI in bmpc_hip.hip (bmpc_stream_rollout_audit, bmpc_stream_tube).
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

static_assert(bmpcs::TUBE_L == BMPC_TUBE_L && bmpcs::TUBE_W == BMPC_TUBE_W && bmpcs::TUBE_EX_POS == BMPC_TUBE_EX_POS && bmpcs::TUBE_EX_ROT == BMPC_TUBE_EX_ROT
              && bmpcs::TUBE_EX_Q == BMPC_TUBE_EX_Q && bmpcs::TUBE_EX_DQ == BMPC_TUBE_EX_DQ && bmpcs::TUBE_SEG == BMPC_TUBE_SEG && bmpcs::TUBE_PHI == BMPC_TUBE_PHI
              && bmpcs::TUBE_LEN == BMPC_TUBE_LEN, "tube slots of the header and of the kernel text");
static_assert(bmpcs::AUDIT_SAMPLES == BMPC_AUDIT_SAMPLES && bmpcs::AUDIT_MAX_POS == BMPC_AUDIT_MAX_POS && bmpcs::AUDIT_TICK_POS == BMPC_AUDIT_TICK_POS
              && bmpcs::AUDIT_MAX_ROT == BMPC_AUDIT_MAX_ROT && bmpcs::AUDIT_TICK_ROT == BMPC_AUDIT_TICK_ROT && bmpcs::AUDIT_MAX_Q == BMPC_AUDIT_MAX_Q
              && bmpcs::AUDIT_MAX_DQ == BMPC_AUDIT_MAX_DQ && bmpcs::AUDIT_N_POS == BMPC_AUDIT_N_POS && bmpcs::AUDIT_N_ROT == BMPC_AUDIT_N_ROT
              && bmpcs::AUDIT_N_JOINT == BMPC_AUDIT_N_JOINT && bmpcs::AUDIT_FIRST_OUT == BMPC_AUDIT_FIRST_OUT && bmpcs::AUDIT_LEN == BMPC_AUDIT_LEN,
              "audit slots of the header and of the kernel text");

// tube and joint-limit excess of the measured state a pack left in p; reads p and the error count (ss may be NULL), writes the tube row only
__global__ void __launch_bounds__(64) bmpc_stream_tube_kernel(int N, int S, int B, const double *p, const double *ss, double *tube) {
    const int b = blockIdx.x;
    bmpcs::stream_tube(N, S, p + (long long)b * (141 + 91 * S), ss ? ss + (long long)b * bmpcs::ss_len(N) : nullptr, tube + (long long)b * bmpcs::TUBE_LEN, threadIdx.x, 64);
}
hipError_t bmpc_stream_tube_launch(int N, int S, int B, const double *p, const double *ss, double *tube, hipStream_t st) {
    hipLaunchKernelGGL(bmpc_stream_tube_kernel, dim3(B), dim3(64), 0, st, N, S, B, p, ss, tube);
    return hipGetLastError();
}

hipError_t bmpc_rollout_audit_launch(bool zlds, bool resto, const void *kargs, const SArgs *s, const RArgs *r, int grid, hipStream_t st) {
    bmpc_rollout_run<true, true, false>(zlds, resto, kargs, *s, *r, grid, st);
    return hipGetLastError();
}
