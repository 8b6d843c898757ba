// bmpc_pair.hip -- gfx950 PAIR kernel of the batched BoundMPC OCP solver: two cooperating waves per problem on the one-wave budget.
//
// The one-wave kernel (bmpc_hip.hip) runs one problem per 64-lane wave; the 4-wave teams (bmpc_team.hip) own a whole CU per problem (their
// workspace rows live in its 160 KB of LDS), so only 256 problems are resident.  Here the same wave program (bmpc_wave.inl compiled with
// BMPC_NW = 2 and BMPC_WSG, namespace bmpcp) runs on a 128-thread workgroup that keeps the ONE-WAVE budget per problem -- 40 KB of LDS, the
// workspace in the global slab -- so two pairs share a CU: 512 problems resident.  Roles: wave 0 runs the recursions (adjoint, Riccati,
// forward); wave 1 the references / objective half of every evaluation beside the kinematics and, inside the Riccati sweep, the staging (its
// own register prefetch) and the recursion-independent half of the next stage's node-cost add, the q~ rows and t6; the item-parallel row
// passes run over all 128 lanes.  Same reduction orders as the team text: results equal the one-wave kernel's up to the order of a few sums
// behind discrete decisions (bit-equal on the bench batches; 2 of 8192 problems differ by 1e-12).  Launched from the C ABI in bmpc_hip.hip
// for batches between the resident teams and the resident pairs (256 < B <= 512): 1.18-1.20x the one-wave kernel there.
//
// Built as the answer to "a second wave on every SIMD" (round 6): compiled for TWO waves per SIMD (-DBMPC_PAIR_EU=2: 256 registers per wave,
// four pairs per CU, 1024 problems resident) the same text needs 744 B of scratch per lane and runs 0.58x the one-wave kernel at B = 1024
// (4.68 vs 2.70 ms; profiles/r06_a_pair_occupancy_ab.txt has the A/B and the resource table per wave role): the LDS budget holds (40 896 B),
// the register budget does not -- at 512 registers per wave the pair is 1.2x the one-wave kernel per problem.  The product build is the
// 512-register one (BMPC_PAIR_EU = 1).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>

#define BMPC_NW 2
#define BMPC_WSG 1
#define BMPC_NAMESPACE bmpcp
#define BMPC_STAMPS 2      // phase stamps: -DBMPC_PROFILE cycle stamps and -DBMPC_MARKS markers (bmpc_gpu_common.h)
#include "bmpc_gpu_common.h"
#include "bmpc_wave.inl"

typedef KArgsT<bmpcp::Opts> KArgs;
static_assert(bmpcp::NW == 2, "pair size");

#ifndef BMPC_PAIR_EU
#define BMPC_PAIR_EU 1      // waves per SIMD the kernel is compiled for (2 = the 256-register experiment of the header)
#endif
#define BMPC_SOLVE_KERNEL __global__ void __launch_bounds__(128, BMPC_PAIR_EU) bmpc_pair_solve_kernel
#include "bmpc_multi_batch.inl"

int bmpc_pair_blocks_per_cu(void) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, bmpc_pair_solve_kernel, 128, 0) != hipSuccess) return 0;
    return per_cu;
}
int bmpc_pair_nmax(void) { return bmpcp::TEAM_NMAX; }
int bmpc_pair_lds_bytes(void) { return (int)(bmpcp::L_SIZE * sizeof(double)); }
long long bmpc_pair_scr_stride(int N) { return bmpcp::make_scr(N).size; }
hipError_t bmpc_pair_launch_solve(const void *kargs, int grid, hipStream_t st) {
    KArgs a; memcpy(&a, kargs, sizeof(a));
    hipLaunchKernelGGL(bmpc_pair_solve_kernel, dim3(grid), dim3(128), 0, st, a);
    return hipGetLastError();
}
