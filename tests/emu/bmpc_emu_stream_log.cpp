// TEST-ONLY: CPU build of the stream log (boundmpc_amd/csrc/bmpc_stream_log.inl), the same text the GPU kernel bmpc_stream_log_kernel runs, with one
// lane.  Used by tests/test_stream_log.py and tests/test_gpu_stream_log.py; never built, loaded or fallen back to by the product.
#include <cstdio>

#include "bmpc_emu_host.h"
#include "../../boundmpc_amd/csrc/bmpc_stream.inl"
#include "../../boundmpc_amd/csrc/bmpc_stream_log.inl"

extern "C" int bmpc_emu_stream_log_len(int N) { return bmpcs::log_len(N); }
// one stream: path [cap][48], ss, p, traj as a tick left them -> log [88 N + 4]
extern "C" void bmpc_emu_stream_log(int N, int S, double h, const double *path, int cap, const double *ss, const double *p, const double *traj, double *log) {
    double sh[bmpcs::LSH_LEN];
    bmpcs::stream_log(N, S, h, path, cap, ss, p, traj, log, sh, 0, 1);
}
