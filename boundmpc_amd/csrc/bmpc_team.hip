// bmpc_team.hip -- gfx950 TEAM kernels of the batched BoundMPC OCP solver: a workgroup of NW cooperating waves per problem.
//
// For batches that leave SIMDs idle (B <= resident workgroups / NW: the 256 closed-loop streams of BASELINE configs[4], the single
// solver(...) call per tick that is the reference's own use, BoundMPC.py:446-453) one wave per problem keeps 1 of the 4 SIMDs of a CU
// busy.  Here the same wave program (bmpc_wave.inl compiled with BMPC_NW waves, namespace bmpct) runs on a 64 NW-thread workgroup: the
// item-parallel passes of an interior-point iteration run over all 64 NW lanes, independent sequential pieces run side by side on
// different waves, the recursions (adjoint / Riccati / forward sweep) stay on wave 0.  At 512 registers per wave one team owns a CU
// (one wave per SIMD): 256 problems resident.  The launch functions are called from the C ABI in bmpc_hip.hip.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>

#ifndef BMPC_NW
#define BMPC_NW 4
#endif
#define BMPC_NAMESPACE bmpct
#define BMPC_STAMPS 1      // phase stamps: -DBMPC_PROFILE cycle stamps (bmpc_gpu_common.h)
#include "bmpc_gpu_common.h"
#include "bmpc_wave.inl"
#include "bmpc_stream.inl"

typedef KArgsT<bmpct::Opts> KArgs;
static_assert(bmpct::NW == BMPC_NW, "team size");

#define BMPC_SOLVE_KERNEL __global__ void __launch_bounds__(64 * BMPC_NW, 1) bmpc_team_solve_kernel
#include "bmpc_multi_batch.inl"
// one closed-loop tick of a stream in ONE launch by a team: wave 0 packs, the team solves, wave 0 post-processes (bmpc_team_tick_kernel<RESTO>)
#include "bmpc_tick_kernel.inl"

int bmpc_team_blocks_per_cu(int nw) {
    if (nw != BMPC_NW) return 0;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, bmpc_team_solve_kernel, 64 * BMPC_NW, 0) != hipSuccess) return 0;
    return per_cu;
}
int bmpc_team_nmax(int nw) { return nw == BMPC_NW ? bmpct::TEAM_NMAX : 0; }
int bmpc_team_lds_bytes(int nw) { return nw == BMPC_NW ? (int)(bmpct::L_SIZE * sizeof(double)) : 0; }
hipError_t bmpc_team_launch_solve(int nw, const void *kargs, int grid, hipStream_t st) {
    if (nw != BMPC_NW) return hipErrorInvalidValue;
    KArgs a; memcpy(&a, kargs, sizeof(a));
    hipLaunchKernelGGL(bmpc_team_solve_kernel, dim3(grid), dim3(64 * BMPC_NW), 0, st, a);
    return hipGetLastError();
}
hipError_t bmpc_team_launch_tick(int nw, bool resto, const void *kargs, const SArgs *s, int B, hipStream_t st) {
    if (nw != BMPC_NW) return hipErrorInvalidValue;
    KArgs a; memcpy(&a, kargs, sizeof(a));
    if (resto) hipLaunchKernelGGL(bmpc_team_tick_kernel<true>, dim3(B), dim3(64 * BMPC_NW), 0, st, a, *s);
    else hipLaunchKernelGGL(bmpc_team_tick_kernel<false>, dim3(B), dim3(64 * BMPC_NW), 0, st, a, *s);
    return hipGetLastError();
}
