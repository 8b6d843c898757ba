// bmpc_tick_kernel.inl -- one closed-loop tick of a stream in ONE launch: {pack, solve, post}, stream b = workgroup b.  Shared by bmpc_tick.hip
// (one wave per stream: bmpc_stream_tick_kernel<ZLDS, RESTO>) and bmpc_team.hip (a team of BMPC_NW waves, iterate in LDS:
// bmpc_team_tick_kernel<RESTO>); wave 0 packs and post-processes, the workgroup solves.  Included after the wave program and the stream
// functions; the unit defines KArgs.  In the entry words of bmpc_gpu_common.h (BMPCK_*): g++ compiles the same text for the CPU tests (tests/emu/bmpc_emu.cpp).
// The three steps of a tick are each "one wave per stream" and strictly sequential per stream, so they need no grid-wide boundary
// between them: as three kernels + the work-queue reset they cost three launch ramps, three drains and ~130 us of launch overhead
// per tick at 1 kHz (profiles/r03_*_stream_trace.txt); here stream b is block b (B <= resident workgroups: no work queue, no reset node),
// the stream functions use the reduction area of the solver's LDS, and the hand-over of p, x0 -> solver -> x, g, status goes through
// global memory in program order.
#if BMPC_NW == 1
template <bool ZLDS, bool RESTO>
BMPCK_KERNEL bmpc_stream_tick_kernel(KArgs a, SArgs s) {
#else
template <bool RESTO>
BMPCK_KERNEL bmpc_team_tick_kernel(KArgs a, SArgs s) {
    constexpr bool ZLDS = true;
#endif
    BMPCK_LDS double lds[BMPC_NAMESPACE::L_SIZE];
    const long long tk0_ = a.budget_ticks ? BMPC_NOW() : 0;
    const int b = BMPCK_BLOCK;
    if (b >= a.B) return;
    const int wv = BMPCK_WAVE;
    BMPC_STRIDES(a);
    double *sh = lds + BMPC_NAMESPACE::L_RED;
    static_assert(bmpcs::SH_LEN <= 6 * 64, "the stream functions' LDS words must fit into the solver's reduction area");
    BMPC_STREAM_SLICES(a, s, b);
    // A stream that has lost its plan (N consecutive ticks without an accepted solution: BoundMPC.step() returns five Nones there and the
    // reference node stops, BoundMPC.py:498-506, bound_mpc_node.py:318) is not ticked any further: its problems are the ones nobody could
    // solve (tests/golden/g13_hard_ticks.npz), each would run to the stall test or the iteration cap, and a tick lasts as long as its slowest stream.
    if (ss[bmpcs::SS_ERRCNT] >= (double)a.N) {
        if (BMPCK_LANE == 0) { a.status[b] = 3; if (a.iters) a.iters[b] = 0; if (a.kkt) a.kkt[b] = 0.0; if (a.latency_us) a.latency_us[b] = 0.0; }
        return;
    }
    if (BMPC_NW == 1 || wv == 0) bmpcs::stream_pack(a.N, a.S, path, s.path_stride / bmpcs::PT_LEN, ss, rb, p, x0, dual, (s.flags & 2) ? a.x + (long long)b * nw : nullptr, sh, BMPCK_LANE, BMPCK_NL, s.lvl_c, s.lvl_lo, s.lvl_hi);
    BMPCK_SYNC();
    BMPC_WAVE_INIT(W, a, lds, a.scratch + (long long)b * a.scr_stride, wv); BMPCK_WAVE_HOOK(W);
    BMPC_TICK_PROBLEM(pr, a, b, p, x0, dual);
    const long long t0_ = a.latency_us ? BMPC_NOW() : 0;
    W.deadline = a.budget_ticks ? tk0_ + a.budget_ticks : 0;
    BMPC_NAMESPACE::wave_solve<ZLDS, true, RESTO>(W, pr);
    BMPCK_SYNC();
    if (a.latency_us && BMPCK_LANE == 0) a.latency_us[b] = (double)(BMPC_NOW() - t0_) * 0.01;
    if (BMPC_NW == 1 || wv == 0) bmpcs::stream_post(a.N, a.S, a.h, path, s.path_stride / bmpcs::PT_LEN, ss, rb, pr.x, pr.g, a.status[b], traj, s.flags, s.rt_tol,
                                                    sh, BMPCK_LANE, BMPCK_NL, s.rt_row_cap);
}
