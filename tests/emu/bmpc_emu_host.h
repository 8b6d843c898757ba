// TEST-ONLY: the g++ host of the wave program (boundmpc_amd/csrc/bmpc_wave.inl), shared by every lane emulator under tests/emu.  In the place of
// bmpc_gpu_common.h: the device math macros on plain doubles and <cmath>, a phase as a loop over the 64 lanes in a caller-chosen order, a wide
// phase of a team (BMPC_NW > 1) as a loop over its waves in a caller-chosen order; then the kernels' own entry records and slicers (bmpc_args.h)
// and the wave program itself; then emu_wave, the wave of one emulated workgroup.  For the kernel entries that are written in the entry words
// (BMPCK_*: bmpc_tick_kernel.inl, bmpc_rollout_kernel.inl) the host side of those words: a launch is a loop over emu_launch.block.  The flop-counting hosts include it with `double` replaced by
// their number type, after math macros of their own (BMPC_EMU_OWN_MATH) and, where a phase boundary does more, a BMPC_EMU_PHASE_END.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#define BMPC_EMU 1
#define BMPC_HD
#define BMPC_D
#ifndef BMPC_EMU_OWN_MATH
#define BMPC_SINCOS(x, s, c) (*(s) = std::sin(x), *(c) = std::cos(x))
#define BMPC_EXP(x) std::exp(x)
#define BMPC_LOG(x) std::log(x)
#define BMPC_SQRT(x) std::sqrt(x)
#define BMPC_SIN(x) std::sin(x)
#define BMPC_COS(x) std::cos(x)
#define BMPC_ATAN2(y, x) std::atan2(y, x)
#define BMPC_RSQRT(x) (1.0 / std::sqrt(x))
#define BMPC_FABS(x) std::fabs(x)
#define BMPC_FMAX(a, b) std::fmax(a, b)
#define BMPC_FMIN(a, b) std::fmin(a, b)
#define BMPC_POW15(x) ((x) * std::sqrt(x))
#define BMPC_POW(x, y) std::pow(x, y)
#endif

#ifndef BMPC_EMU_PHASE_END
#define BMPC_EMU_PHASE_END      // what a host does at the end of every phase beside leaving the lane loop
#endif
#define LANES_BEGIN for (int li_ = 0; li_ < 64; ++li_) { const int lane = W.order[li_]; (void)lane;
#define LANES_END } BMPC_EMU_PHASE_END
#define LIDX lane
#if BMPC_NW > 1
// A wide phase is a loop over the waves of the team times their 64 lanes; a solo region runs with the wave index it names.  The waves of the GPU
// run a wide phase concurrently and meet at the barrier behind it: any order of the waves inside a phase must give the same result.  What this
// cannot see are missing barriers BETWEEN phases (a wave racing ahead): those are argued in the kernel text (TEAM_SYNC comments) and tested on the GPU.
#define LIDXW wl
#define TEAM_SYNC()
#define TEAM_SYNC_LDS()
#define WIDE_BEGIN for (int wi_ = 0; wi_ < BMPC_NW; ++wi_) { W.wv = W.worder[wi_]; LANES_BEGIN const int wl = W.wv * 64 + lane; (void)wl;
#define WIDE_END LANES_END } W.wv = 0;
#define SOLO_BEGIN(w) { W.wv = (w);
#define SOLO_END W.wv = 0; }
#endif

// The entry words of a kernel entry (the GPU's: bmpc_gpu_common.h).  The caller "launches" by setting emu_launch and calling the kernel function once
// per block; a workgroup is one lane for the stream functions (lane 0 of 1, wave 0), the wave program's phases loop over the lanes inside the solve, in
// the orders BMPCK_WAVE_HOOK hands the wave.  No barriers (one lane at a time) and no clock: no time budget, no latency.
struct EmuLaunch { int block = 0, grid = 1, lane_order = 0, wave_order = 0; };
inline thread_local EmuLaunch emu_launch;
#define BMPCK_KERNEL static void
#define BMPCK_LDS static thread_local
#define BMPCK_LANE 0
#define BMPCK_NL 1
#define BMPCK_BLOCK emu_launch.block
#define BMPCK_GRID emu_launch.grid
#define BMPCK_WAVE 0
#define BMPCK_UNIFORM(i) (i)
#define BMPCK_SYNC()
#define BMPCS_SYNC()
#define BMPCK_WAVE_HOOK(W) BMPC_NAMESPACE::emu_order(W, emu_launch.lane_order, emu_launch.wave_order)
#define BMPCK_LAUNCH(kernel, grid, st, ...) kernel(__VA_ARGS__)      // (the caller has set emu_launch)
#define BMPC_NOW() 0LL

#include "../../boundmpc_amd/csrc/bmpc_args.h"
#include "../../boundmpc_amd/csrc/bmpc_wave.inl"

namespace BMPC_NAMESPACE {
// the shape test of every entry, and the launch functions' choice of the instantiation with the iterate in LDS
inline bool emu_shape_ok(int N, int S) { return S <= SMAX && S >= 2 && N >= 1 && N <= NMAX; }
inline bool emu_zlds(int N, int S) { return N <= BMPC_SHORT_NMAX && S <= SMAX_ZLDS; }
// the argument head every kernel argument record starts with
inline KArgsT<Opts> emu_args(int N, int S, int B, double h, const Opts &o) { KArgsT<Opts> a{}; a.N = N; a.S = S; a.B = B; a.h = h; a.o = o; return a; }
// the one place a wave gets its orders: lanes of a phase in `lane_order`, the waves of a team in `wave_order` (0 forward, 1 reverse, 2 scrambled)
inline void emu_order(Wave &W, int lane_order, int wave_order) {
    for (int i = 0; i < 64; i++) W.order[i] = lane_order == 0 ? i : (lane_order == 1 ? 63 - i : (i * 37 + 11) % 64);
    for (int i = 0; i < BMPC_NW; i++) W.worder[i] = wave_order == 0 ? i : (wave_order == 1 ? BMPC_NW - 1 - i : (i * 3 + 1) % BMPC_NW);
}
// The wave of one emulated workgroup from the argument head of `a` (the kernels' initialiser), on `lds` and the workspace `scr`; lanes in
// `lane_order`, the waves of a team in `wave_order`.  poison: LDS and workspace are filled with NaN first -- a
// read of something this problem's program has not written (what a reused slab or LDS holds on the GPU) then shows up in the outputs.
template <class ARGS>
inline Wave emu_wave(const ARGS &a, std::vector<double> &lds, std::vector<double> &scr, int lane_order, int wave_order = 0, bool poison = false) {
    if (poison) { std::fill(lds.begin(), lds.end(), std::nan("")); std::fill(scr.begin(), scr.end(), std::nan("")); }
    BMPC_WAVE_INIT(W, a, lds.data(), scr.data(), 0);
    emu_order(W, lane_order, wave_order);
    return W;
}
}  // namespace BMPC_NAMESPACE
