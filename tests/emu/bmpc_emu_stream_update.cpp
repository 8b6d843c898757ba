// TEST-ONLY: CPU build of the stream re-planning (boundmpc_amd/csrc/bmpc_stream_update.inl), the same text the GPU kernel bmpc_stream_update_kernel
// runs, with one lane.  Used by tests/test_stream_update.py and tests/test_gpu_stream_update.py; never built, loaded or fallen back to by the product.
#include <cstdio>

#include "bmpc_emu_host.h"
#include "../../boundmpc_amd/csrc/bmpc_stream.inl"
#include "../../boundmpc_amd/csrc/bmpc_stream_update.inl"

extern "C" int bmpc_emu_stream_replan_len(int S, int cap) { return bmpcs::replan_len(S, cap); }
// one stream: rec (re-plan record), path [cap][48], ss, rb (may be null) are updated in place; returns info
extern "C" int bmpc_emu_stream_update(int N, int S, double *rec, double *path, int cap, double *ss, double *rb, int flags) {
    int info = -1;
    bmpcs::stream_update(N, S, rec, path, cap, ss, rb, &info, flags, 0, 1);
    return info;
}
