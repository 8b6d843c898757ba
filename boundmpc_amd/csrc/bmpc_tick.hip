// bmpc_tick.hip -- gfx950 fused closed-loop tick kernels (one wave per stream) of the batched BoundMPC OCP solver: {pack, solve, post} of a
// stream in ONE launch.  A translation unit of its own since round 5: the kernel exists with and without the restoration phase in the solver
// (RESTO), for both placements of the iterate (ZLDS) -- four instantiations of the whole wave program.  The launch function is called from the
// C ABI in bmpc_hip.hip; the kernel text (bmpc_tick_kernel.inl) is shared with the team version in bmpc_team.hip.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "bmpc_gpu_common.h"
#include "bmpc_wave.inl"
#include "bmpc_stream.inl"

typedef KArgsT<bmpc::Opts> KArgs;

#include "bmpc_tick_kernel.inl"

hipError_t bmpc_tick_launch(bool zlds, bool resto, const void *kargs, const SArgs *s, int B, hipStream_t st) {
    KArgs a; memcpy(&a, kargs, sizeof(a));
    if (zlds && resto) hipLaunchKernelGGL((bmpc_stream_tick_kernel<true, true>), dim3(B), dim3(64), 0, st, a, *s);
    else if (zlds) hipLaunchKernelGGL((bmpc_stream_tick_kernel<true, false>), dim3(B), dim3(64), 0, st, a, *s);
    else if (resto) hipLaunchKernelGGL((bmpc_stream_tick_kernel<false, true>), dim3(B), dim3(64), 0, st, a, *s);
    else hipLaunchKernelGGL((bmpc_stream_tick_kernel<false, false>), dim3(B), dim3(64), 0, st, a, *s);
    return hipGetLastError();
}
