// TEST-ONLY: the device math macros of the wave program (boundmpc_amd/csrc/bmpc_gpu_common.h) for a g++ build, shared by the lane
// emulators bmpc_emu.cpp and bmpc_emu_team.cpp.  Plain doubles and <cmath>; the flop-counting emulators use number types of their own.
#pragma once
#include <cmath>

#define BMPC_EMU 1
#define BMPC_HD
#define BMPC_D
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
