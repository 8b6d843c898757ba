// bmpc_multi_batch.inl -- the batch kernel of a workgroup of BMPC_NW cooperating waves per problem, shared by bmpc_team.hip (teams) and
// bmpc_pair.hip (pairs).  Persistent workgroups take the problems of the batch off the work queue, one lane draws for the whole workgroup.
// Included after the wave program; the unit defines KArgs and BMPC_SOLVE_KERNEL, the kernel's declarator (launch bounds and name).
BMPC_SOLVE_KERNEL(KArgs a) {
    __shared__ double lds[BMPC_NAMESPACE::L_SIZE];
    BMPC_WAVE_INIT(W, a, lds, a.scratch + (long long)blockIdx.x * a.scr_stride, __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)));
    BMPC_STRIDES(a);
#ifdef BMPC_PROFILE
    BMPC_WAVE_STAMP0(W, lds);
#endif
    for (;;) {
        // one lane takes the next problem off the queue for the workgroup
        if (threadIdx.x == 0) lds[BMPC_NAMESPACE::L_TFLAG + 1] = (double)atomicAdd(a.counter, 1);
        __syncthreads();
        const int b = __builtin_amdgcn_readfirstlane((int)lds[BMPC_NAMESPACE::L_TFLAG + 1]);
        __syncthreads();                 // every wave has read the word before the next round rewrites it
        if ((unsigned)b >= (unsigned)a.B) break;             // every wave of every workgroup reaches this exit: the queue is finite
        BMPC_PROBLEM(pr, a, b);
        const long long t0_ = a.latency_us ? (long long)wall_clock64() : 0;
        BMPC_NAMESPACE::wave_solve_retry<true>(W, pr);      // with the second attempt of a status-2 stateless solve, like the one-wave kernel (one more trip of a loop; nothing when retry_cap == 0)
        __syncthreads();
        if (a.rcount && threadIdx.x == 0 && *pr.status == 4) atomicAdd(a.rcount, 1);      // jammed: the (one-wave) restoration kernel continues it (bmpc_resto.hip)
        if (a.latency_us && threadIdx.x == 0) a.latency_us[b] = (double)((long long)wall_clock64() - t0_) * 0.01;   // constant 100 MHz counter
    }
#ifdef BMPC_PROFILE
    if (threadIdx.x < 32 && a.prof) atomicAdd(a.prof + threadIdx.x, (unsigned long long)((long long *)(lds + BMPC_NAMESPACE::L_PROF))[threadIdx.x]);
#endif
}
