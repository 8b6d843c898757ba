// TEST-ONLY: CPU build of the stream re-planning (boundmpc_amd/csrc/bmpc_stream_update.inl), the same text the GPU kernel bmpc_stream_update_kernel
// runs, and of the two event functions (bmpc_stream_events.inl: stream_splice, stream_disturb), with one lane.  No wave program in here.  Used by
// tests/test_stream_update.py, tests/test_stream_rollout_events.py, the contract loop of the rollouts (tests/emu/emu_rollout.py) and their GPU twins;
// never built, loaded or fallen back to by the product.
#include <cstdio>

#include "bmpc_emu_host.h"
#include "../../boundmpc_amd/csrc/bmpc_stream.inl"
#include "../../boundmpc_amd/csrc/bmpc_stream_update.inl"
#include "../../boundmpc_amd/csrc/bmpc_stream_events.inl"

extern "C" int bmpc_emu_stream_replan_len(int S, int cap) { return bmpcs::replan_len(S, cap); }
// one stream: rec (re-plan record), path [cap][48], ss, rb (may be null) are updated in place; returns info
extern "C" int bmpc_emu_stream_update(int N, int S, double *rec, double *path, int cap, double *ss, double *rb, int flags) {
    int info = -1;
    bmpcs::stream_update(N, S, rec, path, cap, ss, rb, &info, flags, 0, 1);
    return info;
}
extern "C" int bmpc_emu_stream_disturb_len() { return bmpcs::DIST_LEN; }
// one stream each: the record / the robot record is updated in place
extern "C" void bmpc_emu_stream_splice(double h, int S, int cap, double *rec, const double *rb, int flags) { bmpcs::stream_splice(h, S, cap, rec, rb, flags, 0, 1); }
extern "C" void bmpc_emu_stream_disturb(double *rb, const double *d) { bmpcs::stream_disturb(rb, d, 0, 1); }
// what bmpc_stream_update does with one stream under `flags` (bit 1: the splice first); returns info, or -2 where the C ABI returns BMPC_ERR_ARG
extern "C" int bmpc_emu_stream_update_flags(int N, int S, double h, double *rec, double *path, int cap, double *ss, double *rb, int flags) {
    if (!bmpc_update_flags_ok(flags, rb)) return -2;
    int info = -1;
    if (flags & 2) bmpcs::stream_splice(h, S, cap, rec, rb, flags, 0, 1);
    bmpcs::stream_update(N, S, rec, path, cap, ss, rb, &info, flags & 1, 0, 1);
    return info;
}
