// bmpc_gpu_common.h -- what the translation units of libboundmpc_hip.so share: the device math macros the wave program
// (bmpc_wave.inl) is written in, its lane and phase macros (one set per BMPC_NW: one wave, or a workgroup of cooperating waves), the phase
// stamps, the prologue of a one-wave kernel and the entry words (BMPCK_*) of the kernel entries the CPU tests compile whole (bmpc_tick_kernel.inl,
// bmpc_rollout_kernel.inl); bmpc_args.h holds the kernel argument records, the per-problem / per-stream slicing of a batch and the argument rule of the rollout entries.  The kernel entry texts shared between
// units are bmpc_multi_batch.inl (team and pair batch kernel) and bmpc_tick_kernel.inl (one-wave and team fused tick).  bmpc_hip.hip holds the one-wave-per-problem batch kernel, the service kernel (one entry
// over the jobs of bmpc_dual.inl, bmpc_kkt.inl and bmpc_sens.inl, each of which slices its own batch) and the C ABI, bmpc_team.hip the team
// kernels (NW cooperating waves per problem), bmpc_pair.hip the pair kernel, bmpc_resto.hip the restoration kernels, bmpc_tick.hip the
// one-wave fused ticks, bmpc_rollout.hip the rollouts (many ticks per stream in one launch; kernel text bmpc_rollout_kernel.inl), bmpc_rollout_events.hip the rollouts with events,
// bmpc_rollout_audit.hip the rollouts with events and the tube audit, bmpc_rollout_log.hip those with the logging records on top, bmpc_rollout_legs.hip
// those with a queue of re-plan records per stream, bmpc_rollout_tune.hip those with a table of controller settings per stream, bmpc_team_rollout.hip,
// bmpc_team_rollout_legs.hip and bmpc_team_rollout_tune.hip the rollouts on teams (the same kernel text with BMPC_NW waves per stream); all nine launch
// through bmpc_rollout_run (bmpc_rollout_kernel.inl).
#pragma once
#include <hip/hip_runtime.h>

#include "bmpc_args.h"      // the kernel argument records, the wave initialiser and the per-problem slicers (host-clean: the CPU emulators run them too)

#define BMPC_HD __host__ __device__ __forceinline__
#define BMPC_D __device__ __forceinline__
#define BMPC_SINCOS(x, s, c) sincos(x, s, c)
#define BMPC_EXP(x) exp(x)
#define BMPC_LOG(x) log(x)
#define BMPC_SQRT(x) sqrt(x)
#define BMPC_SIN(x) sin(x)
#define BMPC_COS(x) cos(x)
#define BMPC_ATAN2(y, x) atan2(y, x)
#define BMPC_RSQRT(x) rsqrt(x)
#define BMPC_FABS(x) fabs(x)
#define BMPC_FMAX(a, b) fmax(a, b)
#define BMPC_FMIN(a, b) fmin(a, b)
#define BMPC_POW15(x) ((x) * sqrt(x))
#define BMPC_POW(x, y) pow(x, y)
#define LIDX 0
#define BMPC_WAVE_RED 1
#ifndef BMPC_NO_MFMA
#define BMPC_MFMA 1       // Schur update of the Riccati stage on the matrix cores (v_mfma_f64_16x16x4_f64)
#endif
#define BMPC_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#define BMPC_NOW() ((long long)wall_clock64())      // constant 100 MHz counter
#define BMPCS_OPAQUE(x) asm volatile("" : "+v"(x))      // stream functions: keeps a loaded value out of the optimiser's reach (no re-sinking of the load under a branch)

// What a kernel entry names of its launch (bmpc_tick_kernel.inl, bmpc_rollout_kernel.inl): the HIP words; tests/emu/bmpc_emu_host.h has a host build's
#define BMPCK_KERNEL __global__ void __launch_bounds__(64 * BMPC_NW, 1)
#define BMPCK_LDS __shared__
#define BMPCK_LANE threadIdx.x
#define BMPCK_NL 64                 // lanes that run the stream functions (one wave)
#define BMPCK_BLOCK blockIdx.x
#define BMPCK_GRID gridDim.x
#define BMPCK_WAVE (BMPC_NW == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)))      // this wave's index in the workgroup
#define BMPCK_UNIFORM(i) __builtin_amdgcn_readfirstlane(i)      // a wave-uniform decision as a scalar: the barriers behind it sit in uniform control flow
#define BMPCK_SYNC() __syncthreads()      // WORKGROUP barrier for every BMPC_NW (BMPCS_SYNC is a wave fence in a team unit)
#define BMPCK_WAVE_HOOK(W)          // behind BMPC_WAVE_INIT; a host build gives the wave its lane and wave order here
#define BMPCK_LAUNCH(kernel, grid, st, ...) hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * BMPC_NW), 0, st, __VA_ARGS__)      // a host build calls the function

#if BMPC_NW > 1
// ---- a workgroup of BMPC_NW cooperating waves per problem (bmpc_team.hip, bmpc_pair.hip) ----
#define BMPC_LANE_ID (threadIdx.x & 63)
// a phase of ONE wave of the workgroup (lane = 0..63); opaque lane id as in the one-wave build
#define LANES_BEGIN { int lane_ = threadIdx.x & 63; asm volatile("" : "+v"(lane_)); const int lane = lane_; (void)lane;
#define LANES_END } __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
// workgroup barrier: s_waitcnt vmcnt(0) lgkmcnt(0) + s_barrier with workgroup-scope release / acquire.  The waves of a workgroup sit on
// one CU and share its L1, so workspace words one wave stored are visible to the others behind it.
#define TEAM_SYNC() __syncthreads()
// the same for hand-overs that go through LDS only: LDS operations complete (lgkmcnt(0)), the waves meet, but outstanding vector-memory
// loads -- a sweep's register prefetch of a later stage -- are NOT waited for (what the vmcnt(0) of __syncthreads() would do: a full
// round trip to the slab per barrier)
#define TEAM_SYNC_LDS() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
#define WIDE_BEGIN LANES_BEGIN const int wl = W.wv * 64 + lane; (void)wl;
#define WIDE_END LANES_END TEAM_SYNC();
#ifdef BMPC_PAIR_ROLE
// diagnostic compile only (resource table per wave role, tests/kernel_resources.py --pair-roles): the solo regions of the OTHER role are compiled out
#define SOLO_BEGIN(w) if (W.wv == (w) && (w) == BMPC_PAIR_ROLE) {
#else
#define SOLO_BEGIN(w) if (W.wv == (w)) {
#endif
#define SOLO_END }
// the stream functions run on wave 0 of the workgroup (64 cooperating lanes, as in the one-wave build): their phase boundary is a wavefront fence
#define BMPCS_SYNC() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
#else
// ---- one wave per problem (bmpc_hip.hip, bmpc_resto.hip, bmpc_tick.hip); bmpc_wave.inl supplies the one-wave team macros ----
#define LANES_BEGIN { int lane_ = threadIdx.x; asm volatile("" : "+v"(lane_)); const int lane = lane_; (void)lane;   // opaque per phase: stops LICM from hoisting per-lane address arithmetic out of the solver loops (register pressure)
// The workgroup is ONE wave: its LDS and vector-memory instructions execute in program order, so a phase boundary needs no
// s_barrier and no s_waitcnt drain (what __syncthreads() would emit: vmcnt(0) lgkmcnt(0), i.e. a full stall on every
// outstanding prefetch / store).  A wavefront-scope fence keeps the COMPILER from moving memory operations across it.
#define LANES_END } __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
#define BMPCS_SYNC() __syncthreads()
#endif

// Phase stamps of the wave program (BMPC_PROF), in the batch kernels only: a unit opts in by defining BMPC_STAMPS before this header --
// 1: the per-phase cycle stamps of lane 0 of a -DBMPC_PROFILE build (diagnostic library libboundmpc_hip_prof.so, never the product);
// 2: also the textual markers of a -DBMPC_MARKS compile (-S only: static instructions per phase, tests/isa_phase_stats.py).
#if defined(BMPC_PROFILE) && BMPC_STAMPS >= 1
#define BMPC_PROF(W, id) { long long now_ = clock64(); if (threadIdx.x == 0) { ((long long *)((W).L + BMPC_NAMESPACE::L_PROF))[id] += now_ - (W).tprev; } (W).tprev = now_; }
#elif defined(BMPC_MARKS) && BMPC_STAMPS >= 2
#define BMPC_PROF(W, id) asm volatile("s_nop 0 ; BMPCMARK " #id ::: "memory");
#endif

// Prologue of a kernel that runs one wave per workgroup (bmpc_hip.hip: solve and service kernels; bmpc_resto.hip): the wave `W` of this workgroup
// from the argument head {N, S, h, o, scratch, scr_stride} of `a` (BMPC_WAVE_INIT of bmpc_args.h), on the LDS array `lds` and on workspace slab
// blockIdx.x; in a unit that stamps its phases (above) of a -DBMPC_PROFILE build also the zeroed stamp area and the first stamp.
#if defined(BMPC_PROFILE) && BMPC_STAMPS >= 1
#define BMPC_WAVE_STAMP0(W, lds) if (threadIdx.x < 32) ((long long *)((lds) + BMPC_NAMESPACE::L_PROF))[threadIdx.x] = 0; __syncthreads(); W.tprev = clock64()
#else
#define BMPC_WAVE_STAMP0(W, lds) W.tprev = 0
#endif
#define BMPC_ONE_WAVE(W, a, lds) \
    BMPC_WAVE_INIT(W, a, lds, (a).scratch + (long long)blockIdx.x * (a).scr_stride, 0); \
    BMPC_WAVE_STAMP0(W, lds)

// ---- restoration kernel (bmpc_resto.hip): continues the problems a batch kernel left with the internal status 4 ----
hipError_t bmpc_resto_launch(bool zlds, const void *kargs, int grid, hipStream_t st);

// ---- fused closed-loop tick, one wave per stream (bmpc_tick.hip); resto: the instantiation that carries the restoration phase ----
hipError_t bmpc_tick_launch(bool zlds, bool resto, const void *kargs, const SArgs *s, int B, hipStream_t st);

// ---- rollout: many ticks of every stream in one launch, one wave per stream striding over the batch (bmpc_rollout.hip, bmpc_rollout_kernel.inl) ----
hipError_t bmpc_rollout_launch(bool zlds, bool resto, const void *kargs, const SArgs *s, const RArgs *r, int grid, hipStream_t st);
// ---- the same with events behind a tick's post: plant disturbances, one scheduled re-plan per stream (bmpc_rollout_events.hip; bmpc_rollout_kernel.inl, EV) ----
hipError_t bmpc_rollout_events_launch(bool zlds, bool resto, const void *kargs, const SArgs *s, const RArgs *r, int grid, hipStream_t st);
// ---- the same with the audit behind a tick's pack: tube and joint-limit excess of the state the tick starts from (bmpc_rollout_audit.hip; EV and AU) ----
hipError_t bmpc_rollout_audit_launch(bool zlds, bool resto, const void *kargs, const SArgs *s, const RArgs *r, int grid, hipStream_t st);
// ---- the same with the logging records behind a tick's post and the tracking record over their stage 0 (bmpc_rollout_log.hip; EV, AU and LG) ----
hipError_t bmpc_rollout_log_launch(bool zlds, bool resto, const void *kargs, const SArgs *s, const RArgs *r, int grid, hipStream_t st);
// ---- the same with a queue of re-plan records per stream, fired by tick, goal or lost plan (bmpc_rollout_legs.hip; EV, AU, LG and QU) ----
hipError_t bmpc_rollout_legs_launch(bool zlds, bool resto, const void *kargs, const SArgs *s, const RArgs *r, int grid, hipStream_t st);
// ---- the same with a table of controller settings per stream, validated and resolved on the device (bmpc_rollout_tune.hip; EV, AU, LG, QU and TU) ----
hipError_t bmpc_rollout_tune_launch(bool zlds, bool resto, const void *kargs, const SArgs *s, const RArgs *r, int grid, hipStream_t st);
// ---- the same with a table of actuator models per stream between the command and the plant (bmpc_rollout_plant.hip; EV, AU, LG, QU, TU and PL) ----
hipError_t bmpc_rollout_plant_launch(bool zlds, bool resto, const void *kargs, const SArgs *s, const RArgs *r, int grid, hipStream_t st);
// ---- the plant step on its own, one lane per stream of the batch (bmpc_rollout_plant.hip; bmpc_stream_plant.inl) ----
hipError_t bmpc_stream_plant_launch(int N, int B, double h, double *rb, const double *ss, const double *plant, double *state, int *info, double *rec, int tick, hipStream_t st);
// ---- the same with a table of measurement models per stream between the plant and the controller (bmpc_rollout_sensor.hip; everything on and SE) ----
hipError_t bmpc_rollout_sensor_launch(bool zlds, bool resto, const void *kargs, const SArgs *s, const RArgs *r, const NArgs *n, int grid, hipStream_t st);
// ---- the sample and the way back to the truth on their own, one lane per stream of the batch (bmpc_rollout_sensor.hip; bmpc_stream_sensor.inl) ----
hipError_t bmpc_stream_sense_launch(int N, int B, double *rb, const double *ss, const double *sensor, double *state, int *info, double *rec, const double *noise, double *meas,
                                    int tick, hipStream_t st);
hipError_t bmpc_stream_unsense_launch(int N, int B, double h, double *rb, const double *ss, const double *sensor, const double *state, hipStream_t st);
// ---- the same with a table of state observers per stream between the sensor's sample and the pack (bmpc_rollout_observer.hip; everything on, SE and OB) ----
hipError_t bmpc_rollout_observer_launch(bool zlds, bool resto, const void *kargs, const SArgs *s, const RArgs *r, const NArgs *n, const OArgs *o, int grid, hipStream_t st);
// ---- the sample and the estimate on their own, one lane per stream of the batch (bmpc_rollout_observer.hip; bmpc_stream_observer.inl) ----
hipError_t bmpc_stream_observe_launch(int N, int B, double h, double *rb, const double *ss, const double *sensor, double *state, int *info, double *rec, const double *noise,
                                      double *meas, int tick, const double *observer, double *ostate, int *oinfo, double *orec, double *sample, hipStream_t st);
// ---- the measurement on its own, one wave per stream of the batch (bmpc_rollout_audit.hip; bmpc_stream_tube.inl) ----
hipError_t bmpc_stream_tube_launch(int N, int S, int B, const double *p, const double *ss, double *tube, hipStream_t st);

// ---- team kernels (bmpc_team.hip); `kargs` points at a KArgsT<...> record (the layouts are identical across instantiations) ----
// resident workgroups per CU of the team solver kernel with `nw` waves (0: no such instantiation)
int bmpc_team_blocks_per_cu(int nw);
hipError_t bmpc_team_launch_solve(int nw, const void *kargs, int grid, hipStream_t st);
hipError_t bmpc_team_launch_tick(int nw, bool resto, const void *kargs, const SArgs *s, int B, hipStream_t st);
// the rollout on teams (bmpc_team_rollout.hip; bmpc_rollout_kernel.inl with BMPC_NW waves): workgroup w strides over the streams on workspace slab w;
// full: the kernel with the event, audit and log code (it serves all three entries), else the plain one
hipError_t bmpc_team_rollout_launch(int nw, bool resto, bool full, const void *kargs, const SArgs *s, const RArgs *r, int grid, hipStream_t st);
// the same with the queue of re-plan records (bmpc_team_rollout_legs.hip): the fully-featured kernel with QU
hipError_t bmpc_team_rollout_legs_launch(int nw, bool resto, const void *kargs, const SArgs *s, const RArgs *r, int grid, hipStream_t st);
// the same with the table of controller settings per stream (bmpc_team_rollout_tune.hip): the fully-featured kernel with QU and TU
hipError_t bmpc_team_rollout_tune_launch(int nw, bool resto, const void *kargs, const SArgs *s, const RArgs *r, int grid, hipStream_t st);
// the same with the table of actuator models per stream (bmpc_team_rollout_plant.hip): the fully-featured kernel with QU, TU and PL
hipError_t bmpc_team_rollout_plant_launch(int nw, bool resto, const void *kargs, const SArgs *s, const RArgs *r, int grid, hipStream_t st);
// the same with the table of measurement models per stream (bmpc_team_rollout_sensor.hip): the fully-featured kernel with SE
hipError_t bmpc_team_rollout_sensor_launch(int nw, bool resto, const void *kargs, const SArgs *s, const RArgs *r, const NArgs *n, int grid, hipStream_t st);
// the same with the table of state observers per stream (bmpc_team_rollout_observer.hip): the fully-featured kernel with SE and OB
hipError_t bmpc_team_rollout_observer_launch(int nw, bool resto, const void *kargs, const SArgs *s, const RArgs *r, const NArgs *n, const OArgs *o, int grid, hipStream_t st);
int bmpc_team_lds_bytes(int nw);
int bmpc_team_nmax(int nw);      // longest horizon the team kernels take (their LDS holds most of the workspace)

// ---- pair kernel (bmpc_pair.hip): two cooperating waves per problem at two waves per SIMD, one-wave LDS / workspace budget per problem ----
int bmpc_pair_blocks_per_cu(void);      // resident pairs per CU (4 on an MI355X; 0: the launch configuration does not fit)
int bmpc_pair_nmax(void);               // longest horizon the pair kernel takes (the iterate-in-LDS instantiation)
int bmpc_pair_lds_bytes(void);
long long bmpc_pair_scr_stride(int N);  // doubles of workspace per pair (the one-wave layout)
hipError_t bmpc_pair_launch_solve(const void *kargs, int grid, hipStream_t st);
