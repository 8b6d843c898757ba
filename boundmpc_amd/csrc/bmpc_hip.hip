// bmpc_hip.hip -- gfx950 kernel + C ABI (include/boundmpc_hip.h) of the batched BoundMPC OCP solver.
// One problem per 64-lane wavefront (one wave per workgroup); persistent workgroups pull problems
// from an atomic work queue so per-problem iteration counts load-balance; per-wave LDS working
// set + per-wave global scratch slab (see bmpc_wave.inl for the algorithm and the lane maps).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <new>

#include "../../include/boundmpc_hip.h"

#define BMPC_STAMPS 2      // phase stamps: -DBMPC_PROFILE cycle stamps and -DBMPC_MARKS markers (bmpc_gpu_common.h)
#include "bmpc_gpu_common.h"
#include "bmpc_wave.inl"
#include "bmpc_stream.inl"
#include "bmpc_stream_log.inl"
#include "bmpc_stream_update.inl"
#include "bmpc_stream_events.inl"
#include "bmpc_dual.inl"
#include "bmpc_kkt.inl"
#include "bmpc_sens.inl"

typedef KArgsT<bmpc::Opts> KArgs;
#ifndef BMPC_TEAM_NW
#define BMPC_TEAM_NW 4      // waves per problem of the team kernels compiled into the library (bmpc_team.hip)
#endif

#ifndef BMPC_WAVES_PER_EU
#define BMPC_WAVES_PER_EU 1
#endif
template <bool ZLDS>
__global__ void __launch_bounds__(64, BMPC_WAVES_PER_EU) bmpc_solve_kernel(KArgs a) {
    __shared__ double lds[bmpc::L_SIZE];
    BMPC_ONE_WAVE(W, a, lds);
    BMPC_STRIDES(a);
    for (;;) {
        int b = 0;
        if (threadIdx.x == 0) b = atomicAdd(a.counter, 1);
        b = __builtin_amdgcn_readfirstlane(b);
        if ((unsigned)b >= (unsigned)a.B) break;      // every wave reaches this exit: the queue is finite (unsigned: a queue word nobody reset ends the wave, it never becomes an address)
        if (a.order) b = __builtin_amdgcn_readfirstlane(a.order[b]);      // longest-expected-first order of a batch larger than the resident waves (queue_order_kernel)
        BMPC_PROBLEM(pr, a, b);
        const long long t0_ = a.latency_us ? (long long)wall_clock64() : 0;
        bmpc::wave_solve_retry<ZLDS>(W, pr);      // (+ the second attempt of a long-horizon solve that ends with status 2)
        __syncthreads();
        if (a.rcount && threadIdx.x == 0 && *pr.status == 4) atomicAdd(a.rcount, 1);      // jammed: the restoration kernel continues it (bmpc_resto.hip)
        if (a.latency_us && threadIdx.x == 0) a.latency_us[b] = (double)((long long)wall_clock64() - t0_) * 0.01;   // constant 100 MHz counter
    }
#ifdef BMPC_PROFILE
    if (threadIdx.x < 32 && a.prof) atomicAdd(a.prof + threadIdx.x, (unsigned long long)((long long *)(lds + bmpc::L_PROF))[threadIdx.x]);
#endif
}

// Work-queue order of a batch that takes several rounds of the resident waves (bmpc_set_queue_order): rank of every problem by DECREASING key
// (ties: by index) -> order[rank] = problem.  B threads, each walks the B keys (B <= a few 10^4: microseconds).  A launch lasts until its last
// wave is done, so problems that are expected to take long should start first; the key is the objective at the start point (evaluation pass).
#define BMPC_QUEUE_ORDER_MAX 65536      // the ranking is O(B^2 / lanes): beyond this many problems a batch keeps its natural order
__global__ void __launch_bounds__(256) queue_order_kernel(int B, const double *key, int *order) {
    __shared__ double tile[256];
    const int i = blockIdx.x * 256 + threadIdx.x, ic = i < B ? i : B - 1;
    const double ki = key[ic] == key[ic] ? key[ic] : INFINITY;      // (a NaN key -- f of a garbage x0 -- counts as the largest: the ranks must stay a permutation)
    int r = 0;
    for (int j0 = 0; j0 < B; j0 += 256) {      // keys staged through LDS a tile at a time: every thread of the block compares against the same 256 keys
        const int jj = j0 + threadIdx.x;
        __syncthreads();
        tile[threadIdx.x] = jj < B ? (key[jj] == key[jj] ? key[jj] : INFINITY) : -INFINITY;
        __syncthreads();
        const int n = B - j0 < 256 ? B - j0 : 256;
        for (int t = 0; t < n; t++) { const double kj = tile[t]; r += (kj > ki || (kj == ki && j0 + t < i)) ? 1 : 0; }
    }
    if (i < B) order[r] = i;
}

// Service kernel: the jobs that cost a problem a few evaluations, not a solve -- the dual state of a warm solve from multipliers (bmpc_dual.inl,
// DualBatch), the KKT certificate of any primal-dual point (bmpc_kkt.inl, KktBatch), the parametric sensitivity of the solution (bmpc_sens.inl,
// SensBatch).  One wave per problem over the handle's resident waves and workspace slabs, striding over the batch (no work queue); a job is the
// batch record of its file, which slices out problem b and runs the wave program on it.
static_assert(bmpc::KKT_LEN == BMPC_KKT_LEN && bmpc::KKT_E == BMPC_KKT_E && bmpc::KKT_DUAL == BMPC_KKT_DUAL && bmpc::KKT_PRIM_EQ == BMPC_KKT_PRIM_EQ
              && bmpc::KKT_PRIM_INEQ == BMPC_KKT_PRIM_INEQ && bmpc::KKT_COMPL == BMPC_KKT_COMPL && bmpc::KKT_LAM_EQ_GAP == BMPC_KKT_LAM_EQ_GAP
              && bmpc::KKT_LAM_INEQ_GAP == BMPC_KKT_LAM_INEQ_GAP && bmpc::KKT_F == BMPC_KKT_F, "record slots of the header and of the wave program");
static_assert(bmpc::SENS_LEN == BMPC_SENS_LEN && bmpc::SENS_STATUS == BMPC_SENS_STATUS && bmpc::SENS_DELTA == BMPC_SENS_DELTA && bmpc::SENS_RHS == BMPC_SENS_RHS
              && bmpc::SENS_DX == BMPC_SENS_DX, "record slots of the header and of the wave program");
static_assert(bmpc::NZ == 44 && bmpc::NG == 43 && bmpc::NE == 36 && bmpc::NI == 57 && bmpc::NU == 8, "the array lengths include/boundmpc_hip.h documents (44 N, 43 N, ...)");
template <bool ZLDS, class JOB>
__global__ void __launch_bounds__(64, BMPC_WAVES_PER_EU) bmpc_service_kernel(ServiceArgsT<bmpc::Opts, JOB> a) {
    __shared__ double lds[bmpc::L_SIZE];
    BMPC_ONE_WAVE(W, a, lds);
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        a.job.template run<ZLDS>(W, b);
        __syncthreads();
    }
}

// (members without an initialiser start at zero / NULL: bmpc_create value-initialises the handle)
struct bmpc_handle {
    int N, S; double h;
    bmpc::Opts o;            // everything the wave program reads: the public options (bmpc_create) and what the setters add (bmpc_set_restoration, _start_rollout,
                             // _barrier_hold, _second_attempt); defaults of horizon N: bmpc_opts_for (bmpc_args.h)
    int dev;                 // device the handle was created on: workspace, work queue, events and streams of the handle live there
    int refs = 1; bool closed;   // one reference for the creator, one per captured graph (their kernels carry the workspace addresses);
                             // bmpc_destroy closes the handle, the memory goes when the last reference does
    // launches of one handle share its workspace and work queue, so they are ordered against each other whatever streams the
    // caller uses: every launch records order_ev, a launch on another stream waits for it first
    hipEvent_t order_ev, bridge_ev; bool order_valid; hipStream_t order_stream;
    double rt_row_cap;       // real-time mode: a position tube row (l^2 - w^2, any stage) above this vetoes the iterate (bmpc_stream_set_rt_position_row_cap); 0 = off
    double rt_viol_tol = 1e-4;      // acceptance threshold of stream_post in real-time mode (flag bit 1); default = the reference's 1e-4
    double rt_budget_us;     // time budget of a fused tick (bmpc_stream_set_time_budget); 0 = none
    hipStream_t own_stream;  // handle_stream: host-buffer calls run here, and graph replays requested on the legacy null stream, bracketed by events (bmpc_graph_launch)
    int grid; long long scr_stride; double *scratch; int scr_waves; int graphs_alive; int *counter; unsigned long long *prof;
    int team_grid;           // resident TEAMS (workgroups of BMPC_TEAM_NW waves, bmpc_team.hip) of the device; 0: no team kernel for this handle (N > 10 or S > 4)
    int pair_grid;           // resident PAIRS (workgroups of 2 waves at two waves per SIMD, bmpc_pair.hip); 0: no pair kernel for this handle (long horizon or S > 4)
    int *aux_int; int aux_cap;      // [2][aux_cap] status / iters of a batch whose caller passed NULL (the restoration kernel reads them)
    double level_c, level_lo, level_hi;      // bmpc_stream_set_level_rule: stream_pack sets the level of a stream's next tick (level_hi <= 0: off)
    int queue_order;         // bmpc_set_queue_order: 1 = a batch beyond the resident waves is solved in the order of decreasing f(x0) (default for long horizons), 0 = natural order
    double *qkey; int *qorder; int q_cap;      // [q_cap] keys and order of the last such batch
    int team_mode;           // bmpc_set_team_waves: 0 automatic (teams when the batch fits into the resident teams), 1 never, BMPC_TEAM_NW whenever possible
    int rollout_waves = 1;   // bmpc_set_rollout_waves: 1 one wave per stream (default), BMPC_TEAM_NW teams whatever the batch, 0 automatic (teams when the batch fits into the resident teams)
    int timing; hipEvent_t *ev; int nev; long long n_timed;   // timing = number of launches whose {start, stop} event pairs are kept (ring)
    double *latency_us;
    char *arena_d, *arena_h; size_t arena_d_cap, arena_h_cap;      // staging arena of the host-buffer calls (host_call): device and pinned host buffer, capacities in bytes
};

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "boundmpc_hip: %s failed: %s\n", #x, hipGetErrorString(e_)); return BMPC_ERR_HIP; } } while (0)

#define TRY(x) do { if (rc == BMPC_OK && (x) != hipSuccess) rc = BMPC_ERR_HIP; } while (0)      // a step of a sequence that runs to its end: skipped once one has failed

// the instantiation of the one-wave kernels for this handle: iterate in LDS (true) or in the workspace (long horizons, 5 or 6 path segments)
static bool handle_zlds(const bmpc_handle *h) { return h->N <= BMPC_SHORT_NMAX && h->S <= bmpc::SMAX_ZLDS; }
// makes the handle's device current for the scope (allocation, free and synchronisation act on the CURRENT device)
struct DevGuard {
    int prev; bool changed;
    explicit DevGuard(int dev) : prev(dev), changed(false) { if (hipGetDevice(&prev) == hipSuccess && prev != dev) changed = hipSetDevice(dev) == hipSuccess; }
    ~DevGuard() { if (changed) hipSetDevice(prev); }
};
// A stream the CALLER is capturing (e.g. a torch CUDA graph around solve_batch / stream_tick) takes neither: waiting there on an event
// recorded outside the capture invalidates the capture, and recording order_ev inside it would turn it into a captured event that later
// direct launches then wait on.  Ordering of such launches against the handle's other work is the caller's (include/boundmpc_hip.h).
static bool caller_is_capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}
static int order_before(bmpc_handle *h, hipStream_t st) {
    if (caller_is_capturing(st)) return BMPC_OK;
    if (h->order_valid && st != h->order_stream) HIPCHK(hipStreamWaitEvent(st, h->order_ev, 0));
    return BMPC_OK;
}
static int order_after(bmpc_handle *h, hipStream_t st) {
    if (caller_is_capturing(st)) return BMPC_OK;
    HIPCHK(hipEventRecord(h->order_ev, st));
    h->order_stream = st; h->order_valid = true;
    return BMPC_OK;
}
// host wait for the last launch of THIS handle (every launch records order_ev): what teardown and workspace growth need -- not a
// device-wide drain, which would stall every other stream and handle of the process
static void wait_for_handle(bmpc_handle *h) {
    if (h->order_valid) hipEventSynchronize(h->order_ev);
}
static void handle_release(bmpc_handle *h) {
    if (--h->refs > 0) return;
    DevGuard dg(h->dev);
    for (int i = 0; i < 2 * h->nev; i++) hipEventDestroy(h->ev[i]);
    delete[] h->ev;
    if (h->order_ev) hipEventDestroy(h->order_ev);
    if (h->bridge_ev) hipEventDestroy(h->bridge_ev);
    if (h->own_stream) hipStreamDestroy(h->own_stream);
    hipFree(h->scratch); hipFree(h->counter); hipFree(h->aux_int); hipFree(h->qkey); hipFree(h->qorder); hipFree(h->prof); hipFree(h->arena_d); if (h->arena_h) hipHostFree(h->arena_h);
    delete h;
}

// The frozen public struct is the leading part of the wave program's option record; copy_public is the one place that converts between the two.
#define SAME_PLACE(f) (offsetof(bmpc_options, f) == offsetof(bmpc::Opts, f))
static_assert(SAME_PLACE(tol) && SAME_PLACE(max_iter) && SAME_PLACE(mu_init) && SAME_PLACE(mu_min_fac) && SAME_PLACE(slack_push) && SAME_PLACE(exact_hessian)
              && SAME_PLACE(verbose) && SAME_PLACE(mu_warm) && SAME_PLACE(stall_window) && SAME_PLACE(bound_margin)
              && sizeof(bmpc_options) == offsetof(bmpc::Opts, restoration), "bmpc_options is the leading part of bmpc::Opts");
#undef SAME_PLACE
static void copy_public(void *dst, const void *src) { memcpy(dst, src, sizeof(bmpc_options)); }
extern "C" int bmpc_default_options_for(int N, bmpc_options *o) {
    if (!o) return BMPC_ERR_ARG;
    bmpc::Opts d; bmpc_opts_for(N, d);
    copy_public(o, &d);
    return BMPC_OK;
}
extern "C" int bmpc_default_options(bmpc_options *o) { return bmpc_default_options_for(BMPC_SHORT_NMAX, o); }
extern "C" const char *bmpc_error_string(int c) {
    switch (c) { case BMPC_OK: return "ok"; case BMPC_ERR_ARG: return "invalid argument"; case BMPC_ERR_HIP: return "HIP runtime error";
                 case BMPC_ERR_NOGPU: return "no HIP device available"; default: return "unknown error"; }
}
extern "C" int bmpc_create(int N, int S, double dt, const bmpc_options *opts, bmpc_handle **out) {
    if (!out || N < 1 || N > bmpc::NMAX || S < 2 || S > bmpc::SMAX || !(dt > 0)) return BMPC_ERR_ARG;
    if (opts && (!(opts->tol > 0) || opts->max_iter < 0 || opts->stall_window < 0 || (opts->stall_window & 1) || !(opts->mu_init > 0) || !(opts->slack_push > 0) || !(opts->bound_margin >= 0) || opts->bound_margin > 0.5)) return BMPC_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return BMPC_ERR_NOGPU;
    bmpc_handle *h = new (std::nothrow) bmpc_handle();
    if (!h) return BMPC_ERR_ARG;
    h->N = N; h->S = S; h->h = dt;
    bmpc_opts_for(N, h->o); h->queue_order = N > BMPC_SHORT_NMAX ? 1 : 0;
    if (opts) copy_public(&h->o, opts);      // (what the public struct does not carry keeps the default of the horizon)
    int dev = 0, per_cu = 0; hipDeviceProp_t prop;
    bool ok = hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess;
    h->dev = dev;
    if (ok) ok = (handle_zlds(h) ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, bmpc_solve_kernel<true>, 64, 0)
                          : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, bmpc_solve_kernel<false>, 64, 0)) == hipSuccess;
    if (ok) {
        if (per_cu < 1) per_cu = 1;
        h->grid = per_cu * prop.multiProcessorCount;
        h->scr_stride = bmpc::make_scr(N).size;
        // teams: a workgroup of BMPC_TEAM_NW waves per problem (bmpc_team.hip; iterate-in-LDS instantiation only)
        h->team_grid = (N <= bmpc_team_nmax(BMPC_TEAM_NW) && S <= bmpc::SMAX_ZLDS) ? bmpc_team_blocks_per_cu(BMPC_TEAM_NW) * prop.multiProcessorCount : 0;
        // pairs: two waves per problem at two waves per SIMD (bmpc_pair.hip); same workspace layout and LDS budget as one wave per problem
        h->pair_grid = (N <= bmpc_pair_nmax() && S <= bmpc::SMAX_ZLDS && bmpc_pair_scr_stride(N) == h->scr_stride) ? bmpc_pair_blocks_per_cu() * prop.multiProcessorCount : 0;
        // the per-wave workspace slabs (148 KB at N=10, 444 KB at N=30) are allocated on the first solve, for min(B, grid) waves, and grow on demand:
        // a single-problem handle (the nlpsol shim of one BoundMPC object) holds one slab, not 1024
        ok = hipMalloc(&h->counter, 4 * sizeof(int)) == hipSuccess      /* work queue, work queue of the restoration kernel, jam count */
          && hipMemset(h->counter, 0, 4 * sizeof(int)) == hipSuccess
          && hipMalloc(&h->prof, 32 * sizeof(unsigned long long)) == hipSuccess
          && hipMemset(h->prof, 0, 32 * sizeof(unsigned long long)) == hipSuccess
          && hipEventCreateWithFlags(&h->order_ev, hipEventDisableTiming) == hipSuccess
          && hipEventCreateWithFlags(&h->bridge_ev, hipEventDisableTiming) == hipSuccess;
    }
    if (!ok) {   // nothing half-built survives a failed create
        fprintf(stderr, "boundmpc_hip: bmpc_create failed: %s\n", hipGetErrorString(hipGetLastError()));
        if (h->order_ev) hipEventDestroy(h->order_ev);
        if (h->bridge_ev) hipEventDestroy(h->bridge_ev);
        hipFree(h->scratch); hipFree(h->counter); hipFree(h->prof); delete h;
        return BMPC_ERR_HIP;
    }
    *out = h;
    return BMPC_OK;
}
extern "C" int bmpc_destroy(bmpc_handle *h) {
    if (!h || h->closed) return BMPC_ERR_ARG;
    {
        DevGuard dg(h->dev);
        wait_for_handle(h);        // launches are asynchronous: nothing of this handle may still be running on its workspace
    }
    // captured graphs carry the addresses of the workspace and of the work queue: while one is alive the memory stays, the handle
    // only stops accepting work (bmpc_graph_launch of such a graph returns BMPC_ERR_ARG); the last bmpc_graph_destroy frees it
    h->closed = true;
    handle_release(h);
    return BMPC_OK;
}
extern "C" int bmpc_num_vars(const bmpc_handle *h) { return h ? h->N * bmpc::NZ : -1; }
extern "C" int bmpc_num_cons(const bmpc_handle *h) { return h ? h->N * bmpc::NG : -1; }
extern "C" int bmpc_num_params(const bmpc_handle *h) { return h ? 141 + 91 * h->S : -1; }

extern "C" int bmpc_get_bounds(const bmpc_handle *h, double *lbx, double *ubx, double *lbg, double *ubg) {
    if (!h) return BMPC_ERR_ARG;
    // casadi_ocp_formulation.py:92-153 (variables) and :272-349 (constraints); limits RobotModel.py:20-43
    const double qd[7] = {165, 115, 165, 115, 165, 115, 170}, dqd[7] = {85, 85, 100, 75, 130, 135, 135};
    const double inf = INFINITY, pi = 3.14159265358979323846;
    for (int k = 0; k < h->N; k++) {
        double *l = lbx ? lbx + k * 44 : nullptr, *u = ubx ? ubx + k * 44 : nullptr;
        for (int i = 0; i < 44; i++) {
            double lo = -inf, hi = inf;
            if (i < 8) { lo = -35.0; hi = 35.0; }
            else if (i < 15) { hi = qd[i - 8] * pi / 180; lo = -hi; }
            else if (i < 22) { hi = dqd[i - 15] * pi / 180; lo = -hi; }
            else if (i == 41) { lo = 0.0; }
            if (l) l[i] = lo; if (u) u[i] = hi;
        }
        for (int i = 0; i < 43; i++) { if (lbg) lbg[k * 43 + i] = i < 36 ? 0.0 : -inf; if (ubg) ubg[k * 43 + i] = 0.0; }
    }
    return BMPC_OK;
}

// Grows handle-owned device buffers that share one capacity (`cap`, committed last: a failed step leaves capacity 0, and the next call starts
// over from whatever is allocated).  Growing frees the old buffers, which no launch may still be using: the handle's last launch is waited for
// first, and captured graphs (which carry the old addresses) forbid growth with `refusal` -- size the first solve / capture for the largest batch.
struct DevBuf { void **ptr; size_t bytes; };
template <int NB>
static int grow_buffers(bmpc_handle *h, int *cap, int want, const DevBuf (&bufs)[NB], const char *refusal) {
    if (want <= *cap) return BMPC_OK;
    DevGuard dg(h->dev);
    if (*bufs[0].ptr) {
        if (h->graphs_alive > 0) { fprintf(stderr, refusal, h->graphs_alive); return BMPC_ERR_ARG; }
        wait_for_handle(h);
    }
    *cap = 0;
    for (const DevBuf &b : bufs) if (*b.ptr) { void *old = *b.ptr; *b.ptr = nullptr; HIPCHK(hipFree(old)); }
    for (const DevBuf &b : bufs) HIPCHK(hipMalloc(b.ptr, b.bytes));
    *cap = want;
    return BMPC_OK;
}
// workspace for `waves` resident waves
static int ensure_scratch(bmpc_handle *h, int waves) {
    return grow_buffers(h, &h->scr_waves, waves, {{(void **)&h->scratch, sizeof(double) * (size_t)h->scr_stride * waves}},
                        "boundmpc_hip: a larger batch needs a larger workspace, but %d captured graph(s) hold the current one\n");
}

// event pair of the next timed launch (ring of h->timing pairs, created on first use)
static int timing_slot(bmpc_handle *h, hipEvent_t **pair) {
    if (h->nev < h->timing) {
        hipEvent_t *ne = new hipEvent_t[2 * h->timing];
        for (int i = 0; i < 2 * h->nev; i++) ne[i] = h->ev[i];
        for (int i = 2 * h->nev; i < 2 * h->timing; i++) HIPCHK(hipEventCreate(&ne[i]));
        delete[] h->ev; h->ev = ne; h->nev = h->timing;
    }
    *pair = h->ev + 2 * (h->n_timed % h->timing);
    return BMPC_OK;
}
// Which kernel solves a batch of B (waves per problem): a team of BMPC_TEAM_NW waves when the batch fits into the resident teams of the device
// (256 on an MI355X: a team owns a CU) or when the caller asked for teams; a pair (2 waves on the one-wave budget: 512 resident, bmpc_pair.hip)
// when it fits into the resident pairs; else one wave per problem.  bmpc_set_team_waves: 1 = always one wave, 2 = pairs whatever the batch,
// BMPC_TEAM_NW = teams whatever the batch.
static int solve_waves(const bmpc_handle *h, int B) {
    if (h->team_mode == 1) return 1;
    if (h->team_mode == 2) return h->pair_grid > 0 ? 2 : 1;
    if (h->team_grid > 0 && (h->team_mode == BMPC_TEAM_NW || B <= h->team_grid)) return BMPC_TEAM_NW;
    return (h->pair_grid > 0 && B <= h->pair_grid) ? 2 : 1;
}
static bool use_team(const bmpc_handle *h, int B) { return solve_waves(h, B) == BMPC_TEAM_NW; }
static int launch_grid(const bmpc_handle *h, int B) { const int w = solve_waves(h, B), g = w == BMPC_TEAM_NW ? h->team_grid : (w == 2 ? h->pair_grid : h->grid); return B < g ? B : g; }
// the restoration kernel (bmpc_resto.hip) runs one wave per problem whatever kernel solved the batch
static int resto_grid(const bmpc_handle *h, int B) { return B < h->grid ? B : h->grid; }
// a stateless batch of B that is handed out longest-expected-first (bmpc_set_queue_order): one wave per problem, several rounds of the resident waves
static bool queue_ordered(const bmpc_handle *h, int B) { return h->queue_order && B <= BMPC_QUEUE_ORDER_MAX && solve_waves(h, B) == 1 && B > h->grid; }
// what a batch of B needs besides the caller's buffers: workspace slabs for the resident waves of both kernels, -- the hand-over to the
// restoration kernel goes through status[] and iters[] -- handle-owned stand-ins for a caller that passes NULL there, and the keys and
// order of a queue-ordered batch.  Never inside a capture.
static int reserve_for_batch(bmpc_handle *h, int B) {
    const int lg = launch_grid(h, B), rg = h->o.restoration ? resto_grid(h, B) : 0;
    int rc = ensure_scratch(h, lg > rg ? lg : rg);
    if (rc == BMPC_OK) rc = grow_buffers(h, &h->aux_cap, B, {{(void **)&h->aux_int, sizeof(int) * 2 * (size_t)B}},
                                         "boundmpc_hip: a larger batch needs larger status buffers, but captured graphs hold the current ones\n");
    if (rc == BMPC_OK && queue_ordered(h, B)) rc = grow_buffers(h, &h->q_cap, B, {{(void **)&h->qkey, sizeof(double) * (size_t)B}, {(void **)&h->qorder, sizeof(int) * (size_t)B}},
                                                                "boundmpc_hip: a larger batch needs larger queue-order buffers, but captured graphs hold the current ones\n");
    return rc;
}
// a 0 / 1 setting of the handle (field: where it lives; not looked at without a handle)
static int set_switch(bmpc_handle *h, int *field, int v) {
    if (!h || v < 0 || v > 1) return BMPC_ERR_ARG;
    *field = v;
    return BMPC_OK;
}
extern "C" int bmpc_set_queue_order(bmpc_handle *h, int mode) { return set_switch(h, h ? &h->queue_order : nullptr, mode); }
extern "C" int bmpc_get_queue_order(const bmpc_handle *h) { return h ? h->queue_order : -1; }
extern "C" int bmpc_set_restoration(bmpc_handle *h, int enabled, int short_steps, int cap) {
    if (!h || short_steps > 1000 || cap > 100000 || cap == 0 || enabled > 2) return BMPC_ERR_ARG;      // (every argument is checked before any is applied)
    if (enabled >= 0) h->o.restoration = enabled;
    if (short_steps >= 0) h->o.resto_short = short_steps;
    if (cap >= 1) h->o.resto_cap = cap;
    return BMPC_OK;
}
extern "C" int bmpc_get_restoration(const bmpc_handle *h, int *enabled, int *short_steps, int *cap) {
    if (!h) return BMPC_ERR_ARG;
    if (enabled) *enabled = h->o.restoration; if (short_steps) *short_steps = h->o.resto_short; if (cap) *cap = h->o.resto_cap;
    return BMPC_OK;
}
extern "C" int bmpc_set_start_rollout(bmpc_handle *h, int enabled) { return set_switch(h, h ? &h->o.start_rollout : nullptr, enabled); }
extern "C" int bmpc_set_barrier_hold(bmpc_handle *h, int enabled) { return set_switch(h, h ? &h->o.hold_mu : nullptr, enabled); }
extern "C" int bmpc_set_second_attempt(bmpc_handle *h, int cap) {
    if (!h || cap < 0 || cap > 100000) return BMPC_ERR_ARG;
    h->o.retry_cap = cap;
    return BMPC_OK;
}
extern "C" int bmpc_get_second_attempt(const bmpc_handle *h) { return h ? h->o.retry_cap : -1; }
extern "C" int bmpc_stream_set_level_rule(bmpc_handle *h, double c, double lo, double hi) {
    if (!h || !(c >= 0.0) || !(lo >= 0.0) || !(hi >= 0.0) || (hi > 0.0 && !(lo > 0.0 && lo <= hi))) return BMPC_ERR_ARG;
    h->level_c = c; h->level_lo = lo; h->level_hi = hi;
    return BMPC_OK;
}
extern "C" int bmpc_get_start_rollout(const bmpc_handle *h) { return h ? h->o.start_rollout : -1; }
extern "C" int bmpc_options_size(void) { return (int)sizeof(bmpc_options); }
#ifndef BMPC_BUILD_HASH_STR
#define BMPC_BUILD_HASH_STR "0000000000000000"
#endif
// hash of the source text and compiler flags this library was built from (boundmpc_amd/build.py source_hash); the marker is also found in the file's bytes
static const char bmpc_build_hash_marker[] = "BMPC_BUILD_HASH=" BMPC_BUILD_HASH_STR;
extern "C" const char *bmpc_build_hash(void) { return bmpc_build_hash_marker + 16; }
extern "C" int bmpc_set_team_waves(bmpc_handle *h, int waves) {
    if (!h || (waves != 0 && waves != 1 && waves != 2 && waves != BMPC_TEAM_NW)) return BMPC_ERR_ARG;
    if (waves == BMPC_TEAM_NW && h->team_grid <= 0) return BMPC_ERR_ARG;      // no team instantiation for this horizon / window
    if (waves == 2 && h->pair_grid <= 0) return BMPC_ERR_ARG;                // no pair instantiation
    h->team_mode = waves;
    return BMPC_OK;
}
// the waves a rollout gives each stream (bmpc_set_team_waves does not apply to rollouts): read at launch time by rollout_launch
extern "C" int bmpc_set_rollout_waves(bmpc_handle *h, int waves) {
    if (!h || (waves != 0 && waves != 1 && waves != BMPC_TEAM_NW)) return BMPC_ERR_ARG;
    if (waves == BMPC_TEAM_NW && h->team_grid <= 0) return BMPC_ERR_ARG;      // no team instantiation for this horizon / window
    h->rollout_waves = waves;
    return BMPC_OK;
}
extern "C" int bmpc_get_rollout_waves(const bmpc_handle *h) { return h ? h->rollout_waves : -1; }
extern "C" int bmpc_team_info(const bmpc_handle *h, int B, int *waves, int *resident_teams, int *lds_bytes) {
    if (!h) return BMPC_ERR_ARG;
    const int w = solve_waves(h, B);
    if (waves) *waves = w;
    if (resident_teams) *resident_teams = w == 2 ? h->pair_grid : h->team_grid;
    if (lds_bytes) *lds_bytes = w == 2 ? bmpc_pair_lds_bytes() : bmpc_team_lds_bytes(BMPC_TEAM_NW);
    return BMPC_OK;
}
// Reset of the work-queue words (queue, restoration queue, jam count) ahead of a batch kernel.  A KERNEL, not hipMemsetAsync: inside a captured graph
// the runtime (ROCm 7.2) does not reliably order a memset node before the kernel node that follows it when the replay comes behind a cross-stream
// event wait -- a replayed pair kernel drew its first problem index from a queue word that had not been reset yet (round 6: wrong results, then a
// memory fault on a negative index; profiles/r06_e_graph_memset_node.txt).  Kernel after kernel is ordered by the queue itself.
__global__ void __launch_bounds__(64) queue_reset_kernel(int *c) { if (threadIdx.x < 3) c[threadIdx.x] = 0; }
static hipError_t reset_queue(bmpc_handle *h, hipStream_t st) {
    hipLaunchKernelGGL(queue_reset_kernel, dim3(1), dim3(64), 0, st, h->counter);
    return hipGetLastError();
}
// the wave program's options from the handle's settings (max_iter > 0: the cap of this launch)
static bmpc::Opts handle_opts(const bmpc_handle *h, int max_iter) {
    bmpc::Opts o = h->o;
    if (max_iter > 0) o.max_iter = max_iter;
    o.verbose = 0;
    return o;
}
// What a solve of B problems reads and writes, in the order of the C ABI (state: NULL = stateless; max_iter: 0 = the handle's; the outputs
// behind x are optional), and what a closed-loop tick adds to it.  The entry points fill them once; everything below passes them on.
struct SolveIO { const double *p, *x0; double *state; int max_iter; double *x, *g, *lam_g, *lam_x, *f; int *iters, *status; double *kkt; };
struct StreamIO { const double *path; int path_entries; double *sstate, *robot, *traj; int flags; };
// kernel arguments from the handle's settings and a solve record; the caller adds what its launch shape changes
static KArgs handle_kargs(const bmpc_handle *h, int B, const SolveIO &s) {
    KArgs a{}; a.N = h->N; a.S = h->S; a.B = B; a.h = h->h; a.o = handle_opts(h, s.max_iter);
    a.latency_us = h->latency_us; a.scratch = h->scratch; a.scr_stride = h->scr_stride; a.counter = h->counter; a.prof = h->prof;
    a.p = s.p; a.x0 = s.x0; a.x = s.x; a.g = s.g; a.lam_g = s.lam_g; a.lam_x = s.lam_x; a.f = s.f; a.kkt = s.kkt; a.iters = s.iters; a.status = s.status; a.state = s.state;
    return a;
}
// enqueues {reset of the work-queue counter, solver kernel} on `st`
static int enqueue_solve(bmpc_handle *h, int B, const SolveIO &s, hipStream_t st, bool timed, bool capturing = false) {
    if (h->closed) return BMPC_ERR_ARG;
    if (!capturing) { const int rc_ = order_before(h, st); if (rc_ != BMPC_OK) return rc_; }
    KArgs a = handle_kargs(h, B, s);
    if (s.state) a.o.retry_cap = 0;
    const int grid = launch_grid(h, B);
    if (grid > h->scr_waves) return BMPC_ERR_ARG;      // callers reserve the workspace first (never inside a stream capture)
    // restoration phase: the batch kernels hand a jammed problem over through status[] / iters[] (handle-owned when the caller wants neither)
    const bool resto = h->o.restoration != 0;
    a.counter2 = h->counter + 1; a.rcount = resto ? h->counter + 2 : nullptr;
    if (resto && (!a.status || !a.iters)) {
        if (B > h->aux_cap) return BMPC_ERR_ARG;
        if (!a.status) a.status = h->aux_int; if (!a.iters) a.iters = h->aux_int + h->aux_cap;
    }
    const int rgrid = resto ? resto_grid(h, B) : 0;
    if (rgrid > h->scr_waves) return BMPC_ERR_ARG;
    const bool zlds = handle_zlds(h);
    hipEvent_t *pair = nullptr;
    if (timed) { int rc = timing_slot(h, &pair); if (rc != BMPC_OK) return rc; HIPCHK(hipEventRecord(pair[0], st)); }
    if (queue_ordered(h, B) && !s.state && B <= h->q_cap) {
        // Longest-expected-first: an evaluation pass (the same kernel with max_iter = 0: f at x0, nothing else written), the ranking, then the solve
        // hands the problems out in that order.  Inside the timed region: it is part of what the batch costs.  A result does not depend on which
        // wave solves it or when (bitwise invariance under permutation of the batch is a test), so the outputs are those of the natural order.
        KArgs e = a; e.o.max_iter = 0; e.o.start_rollout = 0; e.x = nullptr; e.g = nullptr; e.lam_g = nullptr; e.lam_x = nullptr; e.kkt = nullptr; e.iters = nullptr; e.status = nullptr;
        e.f = h->qkey; e.state = nullptr; e.latency_us = nullptr; e.rcount = nullptr; e.order = nullptr;
        HIPCHK(reset_queue(h, st));
        if (zlds) hipLaunchKernelGGL(bmpc_solve_kernel<true>, dim3(grid), dim3(64), 0, st, e);
        else hipLaunchKernelGGL(bmpc_solve_kernel<false>, dim3(grid), dim3(64), 0, st, e);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(queue_order_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, (const double *)h->qkey, h->qorder);
        HIPCHK(hipGetLastError());
        a.order = h->qorder;
    }
    HIPCHK(reset_queue(h, st));
    // long horizons with the FULL restoration phase (mode 1 is not their default): the whole batch runs in the instantiation that holds the phase, so the
    // continuations of the few problems that need it sit in the work queue instead of following the batch on a handful of waves (same results)
    const bool whole_in_resto = h->o.restoration == 1 && !zlds && solve_waves(h, B) == 1;
    if (whole_in_resto) { KArgs f = a; f.rcount = nullptr; HIPCHK(bmpc_resto_launch(zlds, &f, grid, st)); }
    else if (use_team(h, B)) HIPCHK(bmpc_team_launch_solve(BMPC_TEAM_NW, &a, grid, st));      // a workgroup of waves per problem (bmpc_team.hip)
    else if (solve_waves(h, B) == 2) HIPCHK(bmpc_pair_launch_solve(&a, grid, st));           // two waves per problem at two waves per SIMD (bmpc_pair.hip)
    else if (zlds) hipLaunchKernelGGL(bmpc_solve_kernel<true>, dim3(grid), dim3(64), 0, st, a);      // iterate in LDS; else in the workspace (long horizons, S > 4)
    else hipLaunchKernelGGL(bmpc_solve_kernel<false>, dim3(grid), dim3(64), 0, st, a);
    HIPCHK(hipGetLastError());
    if (resto && !whole_in_resto) HIPCHK(bmpc_resto_launch(zlds, &a, rgrid, st));      // continues what the batch kernel left jammed; returns at once when nothing did (bmpc_resto.hip)
    if (timed) { HIPCHK(hipEventRecord(pair[1], st)); h->n_timed++; }
    if (!capturing) return order_after(h, st);
    return BMPC_OK;
}

// The second attempt of a stateless solve (wave_solve_retry) reads x0 again after the first attempt has written x: with retry_cap > 0 an output
// that overlaps the start would hand the second attempt the failed iterate.  (With the cap at 0 in-place solves are fine: x0 is read in full first.)
static bool second_attempt_rereads_x0(const bmpc_handle *h, int B, const double *x0, const double *x) {
    if (h->o.retry_cap <= 0) return false;
    const size_t n = (size_t)B * h->N * bmpc::NZ * sizeof(double);
    const uintptr_t a = (uintptr_t)x, b = (uintptr_t)x0;
    const bool overlap = a < b + n && b < a + n;
    if (overlap) fprintf(stderr, "boundmpc_hip: x overlaps x0 while the second attempt is on (bmpc_set_second_attempt): it reads x0 again after x is written\n");
    return overlap;
}

// a direct solve on the caller's stream: stateless (bmpc_solve_batch) or warm-started from / updating io.state (bmpc_solve_batch_warm)
static int launch_solve(bmpc_handle *h, int B, bool warm, const SolveIO &io, void *hip_stream) {
    if (!h || B < 0 || io.max_iter < 0 || (B > 0 && (!io.p || !io.x0 || !io.x || (warm && !io.state)))) return BMPC_ERR_ARG;
    if (B == 0) return BMPC_OK;
    if (!warm && second_attempt_rereads_x0(h, B, io.x0, io.x)) return BMPC_ERR_ARG;
    { const int rc_ = reserve_for_batch(h, B); if (rc_ != BMPC_OK) return rc_; }
    return enqueue_solve(h, B, io, (hipStream_t)hip_stream, h->timing != 0);
}
extern "C" int bmpc_solve_batch(bmpc_handle *h, int B, const double *p, const double *x0, double *x, double *g, double *lam_g, double *lam_x,
                                double *f, int *iters, int *status, double *kkt, void *hip_stream) {
    return launch_solve(h, B, false, SolveIO{p, x0, nullptr, 0, x, g, lam_g, lam_x, f, iters, status, kkt}, hip_stream);
}

extern "C" int bmpc_state_len(const bmpc_handle *h) { return h ? h->N * bmpc::NI + 2 : -1; }

extern "C" int bmpc_solve_batch_warm(bmpc_handle *h, int B, const double *p, const double *x0, double *state, int max_iter, double *x, double *g,
                                     double *lam_g, double *lam_x, double *f, int *iters, int *status, double *kkt, void *hip_stream) {
    return launch_solve(h, B, true, SolveIO{p, x0, state, max_iter, x, g, lam_g, lam_x, f, iters, status, kkt}, hip_stream);
}

// ---- service launches: dual state from multipliers (bmpc_dual.inl), KKT certificate (bmpc_kkt.inl), parametric sensitivity (bmpc_sens.inl) ----
typedef bmpc::DualBatch DualBatch; typedef bmpc::KktBatch KktBatch; typedef bmpc::SensBatch SensBatch;
// a service kernel runs one wave per problem on the handle's resident waves, whatever kernel solves a batch of this size
static int service_grid(const bmpc_handle *h, int B) { return B < h->grid ? B : h->grid; }
// reserves the workspace and enqueues the service kernel of `job` on the caller's stream, ordered against the handle's other launches like enqueue_solve
template <class JOB>
static int launch_service(bmpc_handle *h, int B, void *hip_stream, const JOB &job) {
    const int grid = service_grid(h, B); hipStream_t st = (hipStream_t)hip_stream;
    { const int rc_ = ensure_scratch(h, grid); if (rc_ != BMPC_OK) return rc_; }
    if (h->closed) return BMPC_ERR_ARG;
    { const int rc_ = order_before(h, st); if (rc_ != BMPC_OK) return rc_; }
    const ServiceArgsT<bmpc::Opts, JOB> a{h->N, h->S, B, h->h, handle_opts(h, 0), h->scratch, h->scr_stride, job};
    if (handle_zlds(h)) hipLaunchKernelGGL((bmpc_service_kernel<true, JOB>), dim3(grid), dim3(64), 0, st, a);
    else hipLaunchKernelGGL((bmpc_service_kernel<false, JOB>), dim3(grid), dim3(64), 0, st, a);
    HIPCHK(hipGetLastError());
    return order_after(h, st);
}
extern "C" int bmpc_state_from_multipliers(bmpc_handle *h, int B, const double *p, const double *x0, const double *lam_g0, const double *lam_x0,
                                           double mu0, double *state, void *hip_stream) {
    if (!h || B < 0 || (B > 0 && (!p || !x0 || !state))) return BMPC_ERR_ARG;
    if (B == 0) return BMPC_OK;
    return launch_service(h, B, hip_stream, DualBatch{p, x0, lam_g0, lam_x0, state, mu0});
}
extern "C" int bmpc_kkt_len(void) { return BMPC_KKT_LEN; }
extern "C" int bmpc_kkt_batch(bmpc_handle *h, int B, const double *p, const double *x, const double *lam_g0, const double *lam_x0, double *cert,
                              double *g, double *lam_g, double *rj, void *hip_stream) {
    if (!h || B < 1 || !p || !x || !cert) return BMPC_ERR_ARG;
    return launch_service(h, B, hip_stream, KktBatch{p, x, lam_g0, lam_x0, cert, g, lam_g, rj});
}
extern "C" int bmpc_sens_len(void) { return BMPC_SENS_LEN; }
extern "C" int bmpc_sens_batch(bmpc_handle *h, int B, const double *p, const double *x, const double *lam_g, const double *lam_x, const double *dp,
                               double mu, double *dx, double *dlam_eq, double *dnu, double *rec, void *hip_stream) {
    if (!h || B < 1 || !p || !x || !dp || !dx) return BMPC_ERR_ARG;
    return launch_service(h, B, hip_stream, SensBatch{p, x, lam_g, lam_x, dp, mu > 0.0 ? mu : h->o.tol * h->o.mu_min_fac, dx, dlam_eq, dnu, rec});
}

// the handle's own non-blocking stream (created on first use): host-buffer calls and graph replays requested on the legacy null stream run there
static int handle_stream(bmpc_handle *h, hipStream_t *out) {
    if (!h->own_stream) { DevGuard dg(h->dev); HIPCHK(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking)); }
    *out = h->own_stream;
    return BMPC_OK;
}

// ---- hipGraph-captured step: {queue reset, solver kernel, restoration kernel} of one (warm-started) solve, instantiated once, replayed per tick ----
struct bmpc_graph { bmpc_handle *h; hipGraph_t graph; hipGraphExec_t exec; };

// captures what enqueue(stream) puts on a capture stream of its own and instantiates it; the graph holds a reference to the handle
template <class ENQUEUE>
static int capture_graph(bmpc_handle *h, bmpc_graph **out, ENQUEUE enqueue) {
    hipStream_t cs;
    HIPCHK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    bmpc_graph *gr = new (std::nothrow) bmpc_graph{h, nullptr, nullptr};
    if (!gr) { hipStreamDestroy(cs); return BMPC_ERR_ARG; }
    int rc = BMPC_OK;
    if (hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal) != hipSuccess) rc = BMPC_ERR_HIP;
    if (rc == BMPC_OK) {
        rc = enqueue(cs);
        hipError_t e = hipStreamEndCapture(cs, &gr->graph);       // always end the capture, also after an enqueue error
        if (rc == BMPC_OK && e != hipSuccess) rc = BMPC_ERR_HIP;
    }
    if (rc == BMPC_OK && hipGraphInstantiate(&gr->exec, gr->graph, nullptr, nullptr, 0) != hipSuccess) rc = BMPC_ERR_HIP;
    hipStreamDestroy(cs);
    if (rc != BMPC_OK) { if (gr->exec) hipGraphExecDestroy(gr->exec); if (gr->graph) hipGraphDestroy(gr->graph); delete gr; return rc; }
    *out = gr; h->graphs_alive++; h->refs++;
    return BMPC_OK;
}

extern "C" int bmpc_graph_create(bmpc_handle *h, int B, const double *p, const double *x0, double *state, int max_iter, double *x, double *g,
                                 double *lam_g, double *lam_x, double *f, int *iters, int *status, double *kkt, bmpc_graph **out) {
    if (!h || !out || B < 1 || max_iter < 0 || !p || !x0 || !x) return BMPC_ERR_ARG;
    if (!state && second_attempt_rereads_x0(h, B, x0, x)) return BMPC_ERR_ARG;
    { const int rc_ = reserve_for_batch(h, B); if (rc_ != BMPC_OK) return rc_; }
    const SolveIO io{p, x0, state, max_iter, x, g, lam_g, lam_x, f, iters, status, kkt};
    return capture_graph(h, out, [&](hipStream_t cs) { return enqueue_solve(h, B, io, cs, false, true); });
}
extern "C" int bmpc_graph_launch(bmpc_graph *gr, void *hip_stream) {
    if (!gr || !gr->h || gr->h->closed) return BMPC_ERR_ARG;
    bmpc_handle *h = gr->h; hipStream_t st = (hipStream_t)hip_stream;
    // A replay requested on the LEGACY NULL STREAM does not run there: on ROCm 7.2 a graph replayed on the null stream, followed by
    // further null-stream launches without a host synchronisation, ended in a GPU memory fault (tests/cabi/graph_nullstream.cpp).
    // It runs on a non-blocking stream of the handle, bracketed by events: after everything the null stream holds so far, and the
    // null stream's later work after it -- the ordering a caller expects from "launch on the null stream".
    const bool bridged = st == nullptr;
    if (bridged) {
        DevGuard dg(h->dev);
        { const int rc_ = handle_stream(h, &st); if (rc_ != BMPC_OK) return rc_; }
        HIPCHK(hipEventRecord(h->bridge_ev, nullptr));
        HIPCHK(hipStreamWaitEvent(st, h->bridge_ev, 0));
    }
    { const int rc_ = order_before(h, st); if (rc_ != BMPC_OK) return rc_; }
    hipEvent_t *pair = nullptr;
    if (h->timing) { int rc = timing_slot(h, &pair); if (rc != BMPC_OK) return rc; HIPCHK(hipEventRecord(pair[0], st)); }
    HIPCHK(hipGraphLaunch(gr->exec, st));
    if (h->timing) { HIPCHK(hipEventRecord(pair[1], st)); h->n_timed++; }
    { const int rc_ = order_after(h, st); if (rc_ != BMPC_OK) return rc_; }
    if (bridged) HIPCHK(hipStreamWaitEvent(nullptr, h->order_ev, 0));
    return BMPC_OK;
}
extern "C" int bmpc_graph_destroy(bmpc_graph *gr) {
    if (!gr) return BMPC_ERR_ARG;
    bmpc_handle *h = gr->h;
    if (h) {
        DevGuard dg(h->dev);
        wait_for_handle(h);            // a replay of this graph may still be in flight (bmpc_graph_launch records the handle's event behind it)
    }
    hipGraphExecDestroy(gr->exec); hipGraphDestroy(gr->graph); delete gr;
    if (h) { if (h->graphs_alive > 0) h->graphs_alive--; handle_release(h); }     // the last reference of a closed handle frees it
    return BMPC_OK;
}

// ---- host-buffer calls ----
// Device and pinned host staging are owned by the handle and grow on demand (no hipMalloc per call: the single-problem solver(...) call of the
// drop-in shim runs every tick).  ONE arena serves every kind of call: a call synchronises its stream before it returns, on error paths too, so
// nothing of an earlier call is in flight when the next one fills or grows it.  The device buffer holds the call's record and, behind it,
// `tail_bytes` that never cross PCIe (the dual state of bmpc_solve_batch_host_dual); the pinned buffer holds the record.
static int arena_reserve(bmpc_handle *h, size_t rec_bytes, size_t tail_bytes) {
    if (rec_bytes + tail_bytes <= h->arena_d_cap && rec_bytes <= h->arena_h_cap) return BMPC_OK;
    DevGuard dg(h->dev);
    wait_for_handle(h);
    if (rec_bytes + tail_bytes > h->arena_d_cap) {
        hipFree(h->arena_d); h->arena_d = nullptr; h->arena_d_cap = 0;
        if (hipMalloc(&h->arena_d, rec_bytes + tail_bytes) != hipSuccess) { h->arena_d = nullptr; return BMPC_ERR_HIP; }
        h->arena_d_cap = rec_bytes + tail_bytes;
    }
    if (rec_bytes > h->arena_h_cap) {
        if (h->arena_h) hipHostFree(h->arena_h);
        h->arena_h = nullptr; h->arena_h_cap = 0;
        if (hipHostMalloc(&h->arena_h, rec_bytes, hipHostMallocDefault) != hipSuccess) { h->arena_h = nullptr; return BMPC_ERR_HIP; }
        h->arena_h_cap = rec_bytes;
    }
    return BMPC_OK;
}
// One field of a host call's staging record: B problems back to back, `bytes` each.  host: the caller's array (NULL: an optional one it left out).
// FIELD_IN is copied into the record (zeros when left out), FIELD_OUT copied back; an input staged in the slot an output lands in names both
// arrays (bmpc_solve_batch_host_dual).  The fields lie in the record in list order, inputs first: everything up to the last input is ONE
// host-to-device copy, everything from the first output on ONE device-to-host copy.
enum { FIELD_IN = 1, FIELD_OUT = 2 };
struct Field { int io; const void *in; void *out; size_t bytes; };
static Field field_in(const void *host, size_t bytes) { return Field{FIELD_IN, host, nullptr, bytes}; }
static Field field_out(void *host, size_t bytes) { return Field{FIELD_OUT, nullptr, host, bytes}; }
// A host-buffer call: the record staged in, launch(dev, tail, stream) -- dev[i]: field i on the device, tail: `tail_bytes` behind the record --
// and the outputs staged back: one copy each way, one stream synchronisation, on the handle's own non-blocking stream (round 5; it was the
// legacy null stream, on which the call serialised against every blocking stream of a torch process).
template <int NF, class LAUNCH>
static int host_call(bmpc_handle *h, int B, const Field (&f)[NF], size_t tail_bytes, LAUNCH launch) {
    if (h->closed) return BMPC_ERR_ARG;
    size_t off[NF + 1], in_end = 0, out_begin = 0; bool have_out = false;
    off[0] = 0;
    for (int i = 0; i < NF; i++) {
        off[i + 1] = off[i] + (size_t)B * f[i].bytes;
        if (f[i].io & FIELD_IN) in_end = off[i + 1];
        if ((f[i].io & FIELD_OUT) && !have_out) { out_begin = off[i]; have_out = true; }
    }
    int rc = arena_reserve(h, off[NF], tail_bytes);
    if (rc != BMPC_OK) return rc;
    hipStream_t hs = nullptr;
    rc = handle_stream(h, &hs);
    if (rc != BMPC_OK) return rc;
    char *d = h->arena_d, *s = h->arena_h;
    void *dev[NF];
    for (int i = 0; i < NF; i++) {
        dev[i] = d + off[i];
        if (!(f[i].io & FIELD_IN)) continue;
        if (f[i].in) memcpy(s + off[i], f[i].in, off[i + 1] - off[i]); else memset(s + off[i], 0, off[i + 1] - off[i]);
    }
    TRY(hipMemcpyAsync(d, s, in_end, hipMemcpyHostToDevice, hs));
    if (rc == BMPC_OK) rc = launch(dev, d + off[NF], hs);
    TRY(hipMemcpyAsync(s + out_begin, d + out_begin, off[NF] - out_begin, hipMemcpyDeviceToHost, hs));
    if (hipStreamSynchronize(hs) != hipSuccess && rc == BMPC_OK) rc = BMPC_ERR_HIP;      // after a failed step too: the next call reuses the arena
    if (rc != BMPC_OK) return rc;
    for (int i = 0; i < NF; i++) if ((f[i].io & FIELD_OUT) && f[i].out) memcpy(f[i].out, s + off[i], off[i + 1] - off[i]);
    return BMPC_OK;
}
#define DEV(i) ((double *)dev[i])
#define DEV_IF(ptr, i) ((ptr) ? DEV(i) : nullptr)

// The record of a solve: [p | x0 | x | lam_x | g | lam_g | f | kkt] doubles, then [iters | status] ints (until round 3: two blocking copies in, a
// device synchronisation and eight blocking copies out, ~190 us around a 1.1 ms single-problem launch).  dual: the call with multipliers --
// lam_x0 / lam_g0 are staged where the outputs lam_x / lam_g will be written (the conversion reads them before the solve behind it overwrites
// them, in stream order), so the inputs are still ONE host-to-device copy (x and g of the record travel along: the solve overwrites them); the
// dual state between conversion and solve is the tail of the device arena.
static int solve_host(bmpc_handle *h, int B, const double *lam_g0, const double *lam_x0, bool dual, const SolveIO &io) {
    if (!h || B < 0 || (B > 0 && (!io.p || !io.x0 || !io.x))) return BMPC_ERR_ARG;
    if (B == 0) return BMPC_OK;
    const size_t np = (141 + 91 * h->S) * sizeof(double), nw = h->N * bmpc::NZ * sizeof(double), ng = h->N * bmpc::NG * sizeof(double);
    const int staged = dual ? FIELD_IN | FIELD_OUT : FIELD_OUT;
    enum { P, X0, X, LAM_X, G, LAM_G, F, KKT, ITERS, STATUS };
    const Field fl[] = {field_in(io.p, np), field_in(io.x0, nw), field_out(io.x, nw), Field{staged, lam_x0, io.lam_x, nw}, field_out(io.g, ng), Field{staged, lam_g0, io.lam_g, ng},
                        field_out(io.f, sizeof(double)), field_out(io.kkt, sizeof(double)), field_out(io.iters, sizeof(int)), field_out(io.status, sizeof(int))};
    return host_call(h, B, fl, dual ? (size_t)B * (h->N * bmpc::NI + 2) * sizeof(double) : 0, [&](void *const *dev, char *tail, hipStream_t hs) {
        const SolveIO d{DEV(P), DEV(X0), dual ? (double *)tail : nullptr, 0, DEV(X), DEV(G), DEV(LAM_G), DEV(LAM_X), DEV(F), (int *)dev[ITERS], (int *)dev[STATUS], DEV(KKT)};
        const int rc = dual ? bmpc_state_from_multipliers(h, B, d.p, d.x0, DEV_IF(lam_g0, LAM_G), DEV_IF(lam_x0, LAM_X), 0.0, d.state, hs) : BMPC_OK;
        return rc != BMPC_OK ? rc : launch_solve(h, B, dual, d, hs);
    });
}
extern "C" int bmpc_solve_batch_host(bmpc_handle *h, int B, const double *p, const double *x0, double *x, double *g, double *lam_g, double *lam_x,
                                     double *f, int *iters, int *status, double *kkt) {
    return solve_host(h, B, nullptr, nullptr, false, SolveIO{p, x0, nullptr, 0, x, g, lam_g, lam_x, f, iters, status, kkt});
}
extern "C" int bmpc_solve_batch_host_dual(bmpc_handle *h, int B, const double *p, const double *x0, const double *lam_g0, const double *lam_x0,
                                          double *x, double *g, double *lam_g, double *lam_x, double *f, int *iters, int *status, double *kkt) {
    return solve_host(h, B, lam_g0, lam_x0, true, SolveIO{p, x0, nullptr, 0, x, g, lam_g, lam_x, f, iters, status, kkt});
}
// the record of a certificate: [p | x | lam_g0 | lam_x0] in, [cert | g | lam_g | rj] out
extern "C" int bmpc_kkt_batch_host(bmpc_handle *h, int B, const double *p, const double *x, const double *lam_g0, const double *lam_x0, double *cert,
                                   double *g, double *lam_g, double *rj) {
    if (!h || B < 1 || !p || !x || !cert) return BMPC_ERR_ARG;
    const size_t np = (141 + 91 * h->S) * sizeof(double), nw = h->N * bmpc::NZ * sizeof(double), ng = h->N * bmpc::NG * sizeof(double);
    enum { P, X, LAM_G0, LAM_X0, CERT, G, LAM_G, RJ };
    const Field fl[] = {field_in(p, np), field_in(x, nw), field_in(lam_g0, ng), field_in(lam_x0, nw),
                        field_out(cert, BMPC_KKT_LEN * sizeof(double)), field_out(g, ng), field_out(lam_g, ng), field_out(rj, h->N * bmpc::NU * sizeof(double))};
    return host_call(h, B, fl, 0, [&](void *const *dev, char *, hipStream_t hs) {
        return bmpc_kkt_batch(h, B, DEV(P), DEV(X), DEV_IF(lam_g0, LAM_G0), DEV_IF(lam_x0, LAM_X0), DEV(CERT), DEV(G), DEV(LAM_G), DEV(RJ), hs);
    });
}
// the record of a sensitivity: [p | x | dp | lam_g | lam_x] in, [dx | dlam_eq | dnu | rec] out
extern "C" int bmpc_sens_batch_host(bmpc_handle *h, int B, const double *p, const double *x, const double *lam_g, const double *lam_x, const double *dp,
                                    double mu, double *dx, double *dlam_eq, double *dnu, double *rec) {
    if (!h || B < 1 || !p || !x || !dp || !dx) return BMPC_ERR_ARG;
    const size_t np = (141 + 91 * h->S) * sizeof(double), nw = h->N * bmpc::NZ * sizeof(double), ng = h->N * bmpc::NG * sizeof(double);
    enum { P, X, DP, LAM_G, LAM_X, DX, DLAM_EQ, DNU, REC };
    const Field fl[] = {field_in(p, np), field_in(x, nw), field_in(dp, np), field_in(lam_g, ng), field_in(lam_x, nw), field_out(dx, nw),
                        field_out(dlam_eq, h->N * bmpc::NE * sizeof(double)), field_out(dnu, h->N * bmpc::NI * sizeof(double)), field_out(rec, BMPC_SENS_LEN * sizeof(double))};
    return host_call(h, B, fl, 0, [&](void *const *dev, char *, hipStream_t hs) {
        return bmpc_sens_batch(h, B, DEV(P), DEV(X), DEV_IF(lam_g, LAM_G), DEV_IF(lam_x, LAM_X), DEV(DP), mu, DEV(DX), DEV_IF(dlam_eq, DLAM_EQ), DEV_IF(dnu, DNU), DEV(REC), hs);
    });
}
#undef DEV
#undef DEV_IF

extern "C" int bmpc_set_latency_buffer(bmpc_handle *h, double *latency_us) { if (!h) return BMPC_ERR_ARG; h->latency_us = latency_us; return BMPC_OK; }
extern "C" int bmpc_set_timing(bmpc_handle *h, int keep) {
    if (!h || keep < 0 || keep > 65536) return BMPC_ERR_ARG;
    h->timing = keep; h->n_timed = 0;
    return BMPC_OK;
}
extern "C" int bmpc_kernel_ms(bmpc_handle *h, int back, float *ms) {
    if (!h || !ms || back < 0 || h->timing <= 0 || back >= h->timing || back >= h->n_timed) return BMPC_ERR_ARG;
    hipEvent_t *pair = h->ev + 2 * ((h->n_timed - 1 - back) % h->timing);
    HIPCHK(hipEventSynchronize(pair[1]));
    HIPCHK(hipEventElapsedTime(ms, pair[0], pair[1]));
    return BMPC_OK;
}
extern "C" int bmpc_last_kernel_ms(bmpc_handle *h, float *ms) { return bmpc_kernel_ms(h, 0, ms); }
// ---- receding-horizon streams: device-side packing / post-processing, one 64-lane wave per stream ----
__global__ void __launch_bounds__(64) bmpc_stream_pack_kernel(int N, int S, int B, const double *path, int path_stride, double *ss, const double *rb,
                                                             double *p, double *x0, double *dual, const double *xlast, double lvl_c, double lvl_lo, double lvl_hi) {
    __shared__ double sh[bmpcs::SH_LEN];
    const int b = blockIdx.x;
    bmpcs::stream_pack(N, S, path + (long long)b * path_stride, path_stride / bmpcs::PT_LEN, ss + (long long)b * bmpcs::ss_len(N), rb + (long long)b * bmpcs::RB_LEN,
                       p + (long long)b * (141 + 91 * S), x0 + (long long)b * 44 * N, dual ? dual + (long long)b * (57 * N + 2) : nullptr,
                       xlast ? xlast + (long long)b * 44 * N : nullptr, sh, threadIdx.x, 64, lvl_c, lvl_lo, lvl_hi);
}
__global__ void __launch_bounds__(64) bmpc_stream_post_kernel(int N, int S, int B, double h, const double *path, int path_stride, double *ss, double *rb,
                                                             const double *x, const double *g, const int *status, double *traj, int flags, double rt_tol, double rt_row_cap) {
    __shared__ double sh[bmpcs::SH_LEN];
    const int b = blockIdx.x;
    bmpcs::stream_post(N, S, h, path + (long long)b * path_stride, path_stride / bmpcs::PT_LEN, ss + (long long)b * bmpcs::ss_len(N), rb + (long long)b * bmpcs::RB_LEN,
                       x + (long long)b * 44 * N, g + (long long)b * 43 * N, status[b], traj + (long long)b * bmpcs::tr_len(N), flags, rt_tol, sh, threadIdx.x, 64, rt_row_cap);
}
// the logging records (ref_data / err_data) of the plan a tick left behind; reads p, traj, the state and the path table, writes the log row only
__global__ void __launch_bounds__(64) bmpc_stream_log_kernel(int N, int S, int B, double h, const double *path, int path_stride, const double *ss, const double *p,
                                                            const double *traj, double *log) {
    __shared__ double sh[bmpcs::LSH_LEN];
    const int b = blockIdx.x;
    bmpcs::stream_log(N, S, h, path + (long long)b * path_stride, path_stride / bmpcs::PT_LEN, ss + (long long)b * bmpcs::ss_len(N), p + (long long)b * (141 + 91 * S),
                      traj + (long long)b * bmpcs::tr_len(N), log + (long long)b * bmpcs::log_len(N), sh, threadIdx.x, 64);
}
// re-planning (ReferencePath.__init__ and the state part of BoundMPC.update()): reads the re-plan records, writes the path table blocks, the state scalars
// update() sets and the goal of the robot records of the streams whose record carries a raised flag
__global__ void __launch_bounds__(64) bmpc_stream_update_kernel(int N, int S, int B, double *replan, double *path, int path_stride, double *ss, double *rb, int *info,
                                                               int flags) {
    const int b = blockIdx.x, cap = path_stride / bmpcs::PT_LEN;
    bmpcs::stream_update(N, S, replan + (long long)b * bmpcs::replan_len(S, cap), path + (long long)b * path_stride, cap, ss + (long long)b * bmpcs::ss_len(N),
                         rb ? rb + (long long)b * bmpcs::RB_LEN : nullptr, info ? info + b : nullptr, flags, threadIdx.x, 64);
}
// the same behind the splice of the measured state into the raised records (flags bit 1; bit 2: the poor-bounds rule): the spliced words stay in the record
__global__ void __launch_bounds__(64) bmpc_stream_update_splice_kernel(int N, int S, int B, double h, double *replan, double *path, int path_stride, double *ss, double *rb,
                                                                      int *info, int flags) {
    const int b = blockIdx.x, cap = path_stride / bmpcs::PT_LEN;
    double *rec = replan + (long long)b * bmpcs::replan_len(S, cap);
    bmpcs::stream_splice(h, S, cap, rec, rb + (long long)b * bmpcs::RB_LEN, flags, threadIdx.x, 64);
    __syncthreads();
    bmpcs::stream_update(N, S, rec, path + (long long)b * path_stride, cap, ss + (long long)b * bmpcs::ss_len(N), rb + (long long)b * bmpcs::RB_LEN, info ? info + b : nullptr,
                         flags & 1, threadIdx.x, 64);
}
// (the tube kernel, bmpc_stream_tube.inl, lives in bmpc_rollout_audit.hip: this unit's device text is not touched by it)
// plant disturbance: one LANE per stream (the work of a stream is one pass over its kinematic chain)
__global__ void __launch_bounds__(64) bmpc_stream_disturb_kernel(int B, double *rb, const double *d) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b < B) bmpcs::stream_disturb(rb + (long long)b * bmpcs::RB_LEN, d + (long long)b * bmpcs::DIST_LEN, 0, 1);
}
// (the plant kernel, bmpc_stream_plant.inl, lives in bmpc_rollout_plant.hip, as the tube kernel lives in bmpc_rollout_audit.hip: this unit's device text is
// not touched by it)
// (the fused one-launch tick kernels of one wave per stream live in bmpc_tick.hip, those of the teams in bmpc_team.hip)
// The argument test of the four stream entry points (max_iter: 0 where the entry point has none; need: the arrays it cannot do without, looked
// at for B > 0 only).  False: BMPC_ERR_ARG.
static bool stream_args_ok(const bmpc_handle *h, int B, int max_iter, int path_entries, std::initializer_list<const void *> need) {
    if (!h || B < 0 || max_iter < 0 || path_entries < h->S + 1 || h->N > bmpcs::STREAM_NMAX) return false;      // (STREAM_NMAX: the solver's own limit)
    if (B > 0) for (const void *q : need) if (!q) return false;
    return true;
}
static bool tick_args_ok(const bmpc_handle *h, int B, const SolveIO &s, const StreamIO &t) {
    return stream_args_ok(h, B, s.max_iter, t.path_entries, {t.path, t.sstate, t.robot, s.p, s.x0, s.x, s.g, s.status, t.traj});
}
// the stream arguments of a fused launch (tick, rollout): the caller's stream record and the handle's real-time settings and level rule, read now
static SArgs stream_sargs(const bmpc_handle *h, const StreamIO &t) {
    SArgs s; s.path = t.path; s.path_stride = t.path_entries * bmpcs::PT_LEN; s.ss = t.sstate; s.rb = t.robot; s.traj = t.traj; s.flags = t.flags;
    s.rt_tol = h->rt_viol_tol; s.rt_row_cap = h->rt_row_cap; s.lvl_c = h->level_c; s.lvl_lo = h->level_lo; s.lvl_hi = h->level_hi;
    return s;
}
// enqueues the fused tick on `st` (direct launch or inside a capture)
static int enqueue_tick(bmpc_handle *h, int B, const SolveIO &io, const StreamIO &t, hipStream_t st, bool capturing) {
    if (h->closed) return BMPC_ERR_ARG;
    if (!capturing) { const int rc_ = order_before(h, st); if (rc_ != BMPC_OK) return rc_; }
    KArgs a = handle_kargs(h, B, io);
    a.o.retry_cap = 0; a.budget_ticks = (long long)(h->rt_budget_us * 100.0);
    if (B > h->scr_waves) return BMPC_ERR_ARG;
    const SArgs s = stream_sargs(h, t);
    const bool timed = !capturing && h->timing != 0;
    hipEvent_t *pair = nullptr;
    if (timed) { int rc = timing_slot(h, &pair); if (rc != BMPC_OK) return rc; HIPCHK(hipEventRecord(pair[0], st)); }
    // The post-processing of a fused tick needs the final solution, so here the restoration phase runs INSIDE the kernel (instantiations with
    // RESTO); a time-budgeted real-time tick never gets as far as a jam (six short steps) and runs the lean instantiation with the phase off.
    const bool resto = h->o.restoration != 0 && a.budget_ticks == 0;
    if (!resto) a.o.restoration = 0;      // (else the handle's MODE, not a flag: 2 = after a numerical breakdown only, as every other launch shape runs it)
    if (use_team(h, B)) HIPCHK(bmpc_team_launch_tick(BMPC_TEAM_NW, resto, &a, &s, B, st));
    else HIPCHK(bmpc_tick_launch(handle_zlds(h), resto, &a, &s, B, st));      // (long horizons, 5 or 6 path segments: iterate in the workspace)
    if (timed) { HIPCHK(hipEventRecord(pair[1], st)); h->n_timed++; }
    if (!capturing) return order_after(h, st);
    return BMPC_OK;
}
static bool tick_fusable(const bmpc_handle *h, int B) { return B <= (use_team(h, B) ? h->team_grid : h->grid); }      // stream b = workgroup b: every stream needs a resident workgroup
// enqueues one closed-loop tick on `st`: fused into one launch when every stream has a resident workgroup, else {pack, solve, post}
static int enqueue_stream_tick(bmpc_handle *h, int B, const SolveIO &io, const StreamIO &t, hipStream_t st, bool capturing) {
    if (tick_fusable(h, B)) return enqueue_tick(h, B, io, t, st, capturing);
    // real-time mode: the warm start continues from the iterate of the previous tick on every launch shape (fused or not)
    int rc = bmpc_stream_pack_rt(h, B, t.path, t.path_entries, t.sstate, t.robot, (double *)io.p, (double *)io.x0, io.state, (t.flags & 2) ? io.x : nullptr, st);
    if (rc == BMPC_OK) rc = enqueue_solve(h, B, io, st, !capturing && h->timing != 0, capturing);
    if (rc == BMPC_OK) rc = bmpc_stream_post(h, B, t.path, t.path_entries, t.sstate, t.robot, io.x, io.g, io.status, t.traj, t.flags, st);
    return rc;
}
// (a tick has no lam_g, lam_x and f: those slots of its solve record stay NULL)
extern "C" int bmpc_stream_tick(bmpc_handle *h, int B, const double *path, int path_entries, double *sstate, double *robot, double *p, double *x0,
                                double *dual_state, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                                void *hip_stream) {
    const SolveIO io{p, x0, dual_state, max_iter, x, g, nullptr, nullptr, nullptr, iters, status, kkt};
    const StreamIO t{path, path_entries, sstate, robot, traj, flags};
    if (!tick_args_ok(h, B, io, t)) return BMPC_ERR_ARG;
    if (B == 0) return BMPC_OK;
    { const int rc_ = reserve_for_batch(h, B); if (rc_ != BMPC_OK) return rc_; }
    return enqueue_stream_tick(h, B, io, t, (hipStream_t)hip_stream, false);
}

// ---- rollout: `ticks` ticks of every stream in one launch (bmpc_rollout.hip), a direct launch on the caller's stream ----
extern "C" int bmpc_stream_rollout_len(void) { return BMPC_ROLL_LEN; }
// The rollout entries: each fills the solve, stream and rollout records from its arguments and names itself (entry: 0 bmpc_stream_rollout, 1 _events,
// 2 _audit, 3 _log, 4 _legs, 5 _tuned, 6 _plant); the argument test and the level of the kernel text that runs -- without the event code (0), with it (1), with the
// event and the audit code (2), with the log code on top of both (3), with the queue of re-plan records on top of all (4), with the table of per-stream
// settings on top of that (5), with the table of per-stream actuator models on top of that (6) -- are bmpc_rollout_level's (bmpc_args.h).
// n: the record of the sensor entry WITH a table (the SE kernels, which serve whatever level the other arguments name), else NULL.
// o: the record of the observer entry WITH a table (the OB kernels: the SE kernels with the estimate between the sample and the pack), else NULL; with n only.
static int rollout_launch(bmpc_handle *h, int B, const SolveIO &io, const StreamIO &t, const RArgs &r, int entry, hipStream_t st, const NArgs *n = nullptr,
                          const OArgs *o = nullptr) {
    if (!tick_args_ok(h, B, io, t)) return BMPC_ERR_ARG;
    const int level = bmpc_rollout_level(entry, r, h->N, t.flags, t.robot);
    if (level == BMPC_ROLLOUT_REFUSED || (n && !bmpc_rollout_sensor_ok(*n)) || (o && !(n && bmpc_rollout_observer_ok(*n, *o)))) return BMPC_ERR_ARG;
    if (h->rt_budget_us > 0.0) return BMPC_ERR_ARG;                   // a rollout is not real time, and budgeted results depend on the clock
    if (h->closed || caller_is_capturing(st)) return BMPC_ERR_ARG;    // (a direct launch: the workspace may grow, and the ordering events are recorded)
    if (B == 0) return BMPC_OK;
    // bmpc_set_rollout_waves, not bmpc_set_team_waves: one wave per stream (the default), or a team per stream -- whatever the batch, or (automatic)
    // when every stream has a resident team; either way workgroup w strides over the streams on workspace slab w
    const bool team = h->team_grid > 0 && (h->rollout_waves == BMPC_TEAM_NW || (h->rollout_waves == 0 && B <= h->team_grid));
    const int grid = team ? (B < h->team_grid ? B : h->team_grid) : service_grid(h, B);
    { int rc_ = reserve_for_batch(h, B); if (rc_ == BMPC_OK) rc_ = ensure_scratch(h, grid); if (rc_ != BMPC_OK) return rc_; }
    { const int rc_ = order_before(h, st); if (rc_ != BMPC_OK) return rc_; }
    KArgs a = handle_kargs(h, B, io);
    a.o.retry_cap = 0; a.budget_ticks = 0;
    const bool resto = h->o.restoration != 0;      // inside the kernel, as in the fused tick: the post needs the final solution
    const SArgs s = stream_sargs(h, t);
    hipEvent_t *pair = nullptr;
    if (h->timing) { int rc = timing_slot(h, &pair); if (rc != BMPC_OK) return rc; HIPCHK(hipEventRecord(pair[0], st)); }
    // (teams at levels 1 and 2 hand the LG text the caller's log_stages UNCHECKED, with log_hist and track NULL: the kernel reads it behind r.log_hist only)
    if (team && o) HIPCHK(bmpc_team_rollout_observer_launch(BMPC_TEAM_NW, resto, &a, &s, &r, n, o, grid, st));
    else if (o) HIPCHK(bmpc_rollout_observer_launch(handle_zlds(h), resto, &a, &s, &r, n, o, grid, st));
    else if (team && n) HIPCHK(bmpc_team_rollout_sensor_launch(BMPC_TEAM_NW, resto, &a, &s, &r, n, grid, st));
    else if (n) HIPCHK(bmpc_rollout_sensor_launch(handle_zlds(h), resto, &a, &s, &r, n, grid, st));
    else if (team && level == 6) HIPCHK(bmpc_team_rollout_plant_launch(BMPC_TEAM_NW, resto, &a, &s, &r, grid, st));
    else if (team && level == 5) HIPCHK(bmpc_team_rollout_tune_launch(BMPC_TEAM_NW, resto, &a, &s, &r, grid, st));
    else if (team && level == 4) HIPCHK(bmpc_team_rollout_legs_launch(BMPC_TEAM_NW, resto, &a, &s, &r, grid, st));
    else if (team) HIPCHK(bmpc_team_rollout_launch(BMPC_TEAM_NW, resto, level != 0, &a, &s, &r, grid, st));      // (one kernel with everything serves every level from 1 to 3)
    else if (level == 6) HIPCHK(bmpc_rollout_plant_launch(handle_zlds(h), resto, &a, &s, &r, grid, st));
    else if (level == 5) HIPCHK(bmpc_rollout_tune_launch(handle_zlds(h), resto, &a, &s, &r, grid, st));
    else if (level == 4) HIPCHK(bmpc_rollout_legs_launch(handle_zlds(h), resto, &a, &s, &r, grid, st));
    else if (level == 3) HIPCHK(bmpc_rollout_log_launch(handle_zlds(h), resto, &a, &s, &r, grid, st));
    else if (level == 2) HIPCHK(bmpc_rollout_audit_launch(handle_zlds(h), resto, &a, &s, &r, grid, st));
    else if (level == 1) HIPCHK(bmpc_rollout_events_launch(handle_zlds(h), resto, &a, &s, &r, grid, st));
    else HIPCHK(bmpc_rollout_launch(handle_zlds(h), resto, &a, &s, &r, grid, st));
    if (h->timing) { HIPCHK(hipEventRecord(pair[1], st)); h->n_timed++; }
    return order_after(h, st);
}
extern "C" int bmpc_stream_rollout(bmpc_handle *h, int B, int ticks, const double *path, int path_entries, double *sstate, double *robot, double *p, double *x0,
                                   double *dual_state, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                                   double goal_tol, double *hist, double *traj_hist, int *ticks_run, void *hip_stream) {
    const SolveIO io{p, x0, dual_state, max_iter, x, g, nullptr, nullptr, nullptr, iters, status, kkt};
    const StreamIO t{path, path_entries, sstate, robot, traj, flags};
    const RArgs r{ticks, goal_tol, hist, traj_hist, ticks_run};
    return rollout_launch(h, B, io, t, r, 0, (hipStream_t)hip_stream);
}
// with events behind every tick's post (bmpc_rollout_events.hip): disturbances of the plant and one scheduled re-plan per stream
// (the table is written by a re-plan: the caller's `path` is not const where a record may be consumed)
extern "C" int bmpc_stream_rollout_events(bmpc_handle *h, int B, int ticks, const double *path, int path_entries, double *sstate, double *robot, double *p, double *x0,
                                          double *dual_state, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                                          double goal_tol, double *hist, double *traj_hist, int *ticks_run, double *replan, const int *replan_tick, int *replan_info,
                                          int update_flags, const double *disturb, void *hip_stream) {
    const SolveIO io{p, x0, dual_state, max_iter, x, g, nullptr, nullptr, nullptr, iters, status, kkt};
    const StreamIO t{path, path_entries, sstate, robot, traj, flags};
    const RArgs r{ticks, goal_tol, hist, traj_hist, ticks_run, replan, replan_tick, replan_info, update_flags, disturb};
    return rollout_launch(h, B, io, t, r, 1, (hipStream_t)hip_stream);
}
// with the audit behind every tick's pack on top (bmpc_rollout_audit.hip); without both of its arrays it IS the entry above
extern "C" int bmpc_stream_rollout_audit(bmpc_handle *h, int B, int ticks, const double *path, int path_entries, double *sstate, double *robot, double *p, double *x0,
                                         double *dual_state, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                                         double goal_tol, double *hist, double *traj_hist, int *ticks_run, double *replan, const int *replan_tick, int *replan_info,
                                         int update_flags, const double *disturb, double *tube_hist, double *audit, double audit_tol, void *hip_stream) {
    const SolveIO io{p, x0, dual_state, max_iter, x, g, nullptr, nullptr, nullptr, iters, status, kkt};
    const StreamIO t{path, path_entries, sstate, robot, traj, flags};
    const RArgs r{ticks, goal_tol, hist, traj_hist, ticks_run, replan, replan_tick, replan_info, update_flags, disturb, tube_hist, audit, audit_tol};
    return rollout_launch(h, B, io, t, r, 2, (hipStream_t)hip_stream);
}
// with the logging records behind every tick's post on top (bmpc_rollout_log.hip); without both of its arrays it IS the entry above
extern "C" int bmpc_stream_track_len(void) { return BMPC_TRACK_LEN; }
extern "C" int bmpc_stream_rollout_log_len(const bmpc_handle *h, int log_stages) { return (h && log_stages >= 1 && log_stages <= h->N) ? bmpcs::LOG_STAGE * log_stages + 4 : -1; }
extern "C" int bmpc_stream_rollout_log(bmpc_handle *h, int B, int ticks, const double *path, int path_entries, double *sstate, double *robot, double *p, double *x0,
                                       double *dual_state, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                                       double goal_tol, double *hist, double *traj_hist, int *ticks_run, double *replan, const int *replan_tick, int *replan_info,
                                       int update_flags, const double *disturb, double *tube_hist, double *audit, double audit_tol, double *log_hist, int log_stages,
                                       double *track, void *hip_stream) {
    const SolveIO io{p, x0, dual_state, max_iter, x, g, nullptr, nullptr, nullptr, iters, status, kkt};
    const StreamIO t{path, path_entries, sstate, robot, traj, flags};
    const RArgs r{ticks, goal_tol, hist, traj_hist, ticks_run, replan, replan_tick, replan_info, update_flags, disturb, tube_hist, audit, audit_tol, log_hist, log_stages, track};
    return rollout_launch(h, B, io, t, r, 3, (hipStream_t)hip_stream);
}
// with a queue of re-plan records per stream in the place of the one scheduled record (bmpc_rollout_legs.hip, bmpc_team_rollout_legs.hip); without
// records it IS the entry above without a re-plan
extern "C" int bmpc_stream_rollout_legs(bmpc_handle *h, int B, int ticks, const double *path, int path_entries, double *sstate, double *robot, double *p, double *x0,
                                        double *dual_state, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                                        double goal_tol, double *hist, double *traj_hist, int *ticks_run, double *replan, int *replan_info, int update_flags,
                                        const double *disturb, double *tube_hist, double *audit, double audit_tol, double *log_hist, int log_stages, double *track,
                                        int legs, const int *leg_tick, const int *leg_on, const double *leg_tol, int *legs_done, int *leg_fired, int *leg_why,
                                        void *hip_stream) {
    const SolveIO io{p, x0, dual_state, max_iter, x, g, nullptr, nullptr, nullptr, iters, status, kkt};
    const StreamIO t{path, path_entries, sstate, robot, traj, flags};
    const RArgs r{ticks, goal_tol, hist, traj_hist, ticks_run, replan, nullptr, replan_info, update_flags, disturb, tube_hist, audit, audit_tol, log_hist, log_stages, track,
                  legs, leg_tick, leg_on, leg_tol, legs_done, leg_fired, leg_why};
    return rollout_launch(h, B, io, t, r, 4, (hipStream_t)hip_stream);
}
// with a table of controller settings per stream on top (bmpc_rollout_tune.hip, bmpc_team_rollout_tune.hip): the rows live on the device and are validated
// there, by the rule of bmpc_args.h; without a table it IS the entry above
extern "C" int bmpc_stream_tune_len(void) { return BMPC_TUNE_LEN; }
extern "C" int bmpc_stream_tune_defaults(const bmpc_handle *h, int max_iter, double *row) {
    if (!h || max_iter < 0 || !row) return BMPC_ERR_ARG;
    // (the settings as a rollout launched now reads them: rollout_launch's handle_kargs and stream_sargs)
    const bmpc::Opts o = handle_opts(h, max_iter);
    const SArgs s = stream_sargs(h, StreamIO{});
    double unset[BMPC_TUNE_LEN];
    for (int k = 0; k < BMPC_TUNE_LEN; k++) unset[k] = __builtin_nan("");
    bmpc_tune_check(unset, o, s, row);
    return BMPC_OK;
}
extern "C" int bmpc_stream_rollout_tuned(bmpc_handle *h, int B, int ticks, const double *path, int path_entries, double *sstate, double *robot, double *p, double *x0,
                                         double *dual_state, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                                         double goal_tol, double *hist, double *traj_hist, int *ticks_run, double *replan, int *replan_info, int update_flags,
                                         const double *disturb, double *tube_hist, double *audit, double audit_tol, double *log_hist, int log_stages, double *track,
                                         int legs, const int *leg_tick, const int *leg_on, const double *leg_tol, int *legs_done, int *leg_fired, int *leg_why,
                                         const double *tune, int *tune_info, double *tune_used, void *hip_stream) {
    const SolveIO io{p, x0, dual_state, max_iter, x, g, nullptr, nullptr, nullptr, iters, status, kkt};
    const StreamIO t{path, path_entries, sstate, robot, traj, flags};
    const RArgs r{ticks, goal_tol, hist, traj_hist, ticks_run, replan, nullptr, replan_info, update_flags, disturb, tube_hist, audit, audit_tol, log_hist, log_stages, track,
                  legs, leg_tick, leg_on, leg_tol, legs_done, leg_fired, leg_why, tune, tune_info, tune_used};
    return rollout_launch(h, B, io, t, r, 5, (hipStream_t)hip_stream);
}
// with a table of actuator models per stream between the command and the plant on top (bmpc_rollout_plant.hip, bmpc_team_rollout_plant.hip): the rows live on
// the device and are validated there, by the rule of bmpc_args.h; without a table it IS the entry above
extern "C" int bmpc_stream_plant_len(void) { return BMPC_PLANT_LEN; }
extern "C" int bmpc_stream_plant_state_len(void) { return BMPC_PLANT_STATE_LEN; }
extern "C" int bmpc_stream_plant_rec_len(void) { return BMPC_PLANT_REC_LEN; }
extern "C" int bmpc_stream_rollout_plant(bmpc_handle *h, int B, int ticks, const double *path, int path_entries, double *sstate, double *robot, double *p, double *x0,
                                         double *dual_state, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                                         double goal_tol, double *hist, double *traj_hist, int *ticks_run, double *replan, int *replan_info, int update_flags,
                                         const double *disturb, double *tube_hist, double *audit, double audit_tol, double *log_hist, int log_stages, double *track,
                                         int legs, const int *leg_tick, const int *leg_on, const double *leg_tol, int *legs_done, int *leg_fired, int *leg_why,
                                         const double *tune, int *tune_info, double *tune_used, const double *plant, double *plant_state, int *plant_info,
                                         double *plant_rec, void *hip_stream) {
    const SolveIO io{p, x0, dual_state, max_iter, x, g, nullptr, nullptr, nullptr, iters, status, kkt};
    const StreamIO t{path, path_entries, sstate, robot, traj, flags};
    const RArgs r{ticks, goal_tol, hist, traj_hist, ticks_run, replan, nullptr, replan_info, update_flags, disturb, tube_hist, audit, audit_tol, log_hist, log_stages, track,
                  legs, leg_tick, leg_on, leg_tol, legs_done, leg_fired, leg_why, tune, tune_info, tune_used, plant, plant_state, plant_info, plant_rec};
    return rollout_launch(h, B, io, t, r, 6, (hipStream_t)hip_stream);
}
// the step on its own, for per-tick loops (no workspace of the handle: may sit inside a capture)
extern "C" int bmpc_stream_plant(bmpc_handle *h, int B, double *robot, const double *sstate, const double *plant, double *plant_state, int *plant_info, double *plant_rec,
                                 int tick, void *hip_stream) {
    if (!h || B < 1 || !robot || !sstate || !plant || !plant_state || h->N > bmpcs::STREAM_NMAX) return BMPC_ERR_ARG;
    HIPCHK(bmpc_stream_plant_launch(h->N, B, h->h, robot, sstate, plant, plant_state, plant_info, plant_rec, tick, (hipStream_t)hip_stream));
    return BMPC_OK;
}
// with a table of measurement models per stream between the plant and the controller on top (bmpc_rollout_sensor.hip, bmpc_team_rollout_sensor.hip): the rows
// live on the device and are validated there, by the rule of bmpc_args.h; without a table it IS the entry above
extern "C" int bmpc_stream_sensor_len(void) { return BMPC_SENSOR_LEN; }
extern "C" int bmpc_stream_sensor_state_len(void) { return BMPC_SENSOR_STATE_LEN; }
extern "C" int bmpc_stream_sensor_rec_len(void) { return BMPC_SENSOR_REC_LEN; }
extern "C" int bmpc_stream_rollout_sensor(bmpc_handle *h, int B, int ticks, const double *path, int path_entries, double *sstate, double *robot, double *p, double *x0,
                                          double *dual_state, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                                          double goal_tol, double *hist, double *traj_hist, int *ticks_run, double *replan, int *replan_info, int update_flags,
                                          const double *disturb, double *tube_hist, double *audit, double audit_tol, double *log_hist, int log_stages, double *track,
                                          int legs, const int *leg_tick, const int *leg_on, const double *leg_tol, int *legs_done, int *leg_fired, int *leg_why,
                                          const double *tune, int *tune_info, double *tune_used, const double *plant, double *plant_state, int *plant_info,
                                          double *plant_rec, const double *sensor, double *sensor_state, int *sensor_info, double *sensor_rec,
                                          const double *sensor_noise, double *meas_hist, void *hip_stream) {
    const SolveIO io{p, x0, dual_state, max_iter, x, g, nullptr, nullptr, nullptr, iters, status, kkt};
    const StreamIO t{path, path_entries, sstate, robot, traj, flags};
    const RArgs r{ticks, goal_tol, hist, traj_hist, ticks_run, replan, nullptr, replan_info, update_flags, disturb, tube_hist, audit, audit_tol, log_hist, log_stages, track,
                  legs, leg_tick, leg_on, leg_tol, legs_done, leg_fired, leg_why, tune, tune_info, tune_used, plant, plant_state, plant_info, plant_rec};
    const NArgs n{sensor, sensor_state, sensor_info, sensor_rec, sensor_noise, meas_hist};
    return rollout_launch(h, B, io, t, r, 6, (hipStream_t)hip_stream, sensor ? &n : nullptr);
}
// the two steps on their own, for per-tick loops (no workspace of the handle: may sit inside a capture)
extern "C" int bmpc_stream_sense(bmpc_handle *h, int B, double *robot, const double *sstate, const double *sensor, double *sensor_state, int *sensor_info, double *sensor_rec,
                                 const double *sensor_noise, double *meas, int tick, void *hip_stream) {
    if (!h || B < 1 || !robot || !sstate || !sensor || !sensor_state || h->N > bmpcs::STREAM_NMAX) return BMPC_ERR_ARG;
    HIPCHK(bmpc_stream_sense_launch(h->N, B, robot, sstate, sensor, sensor_state, sensor_info, sensor_rec, sensor_noise, meas, tick, (hipStream_t)hip_stream));
    return BMPC_OK;
}
extern "C" int bmpc_stream_unsense(bmpc_handle *h, int B, double *robot, const double *sstate, const double *sensor, const double *sensor_state, void *hip_stream) {
    if (!h || B < 1 || !robot || !sstate || !sensor || !sensor_state || h->N > bmpcs::STREAM_NMAX) return BMPC_ERR_ARG;
    HIPCHK(bmpc_stream_unsense_launch(h->N, B, h->h, robot, sstate, sensor, sensor_state, (hipStream_t)hip_stream));
    return BMPC_OK;
}
// with a table of state observers per stream between the sensor's sample and the pack on top (bmpc_rollout_observer.hip, bmpc_team_rollout_observer.hip): the
// rows live on the device and are validated there, by the rule of bmpc_args.h; without a table it IS the entry above
extern "C" int bmpc_stream_observer_len(void) { return BMPC_OBSERVER_LEN; }
extern "C" int bmpc_stream_observer_state_len(void) { return BMPC_OBSERVER_STATE_LEN; }
extern "C" int bmpc_stream_observer_rec_len(void) { return BMPC_OBSERVER_REC_LEN; }
extern "C" int bmpc_stream_rollout_observer(bmpc_handle *h, int B, int ticks, const double *path, int path_entries, double *sstate, double *robot, double *p, double *x0,
                                            double *dual_state, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj, int flags,
                                            double goal_tol, double *hist, double *traj_hist, int *ticks_run, double *replan, int *replan_info, int update_flags,
                                            const double *disturb, double *tube_hist, double *audit, double audit_tol, double *log_hist, int log_stages, double *track,
                                            int legs, const int *leg_tick, const int *leg_on, const double *leg_tol, int *legs_done, int *leg_fired, int *leg_why,
                                            const double *tune, int *tune_info, double *tune_used, const double *plant, double *plant_state, int *plant_info,
                                            double *plant_rec, const double *sensor, double *sensor_state, int *sensor_info, double *sensor_rec,
                                            const double *sensor_noise, double *meas_hist, const double *observer, double *observer_state, int *observer_info,
                                            double *observer_rec, double *sample_hist, void *hip_stream) {
    const SolveIO io{p, x0, dual_state, max_iter, x, g, nullptr, nullptr, nullptr, iters, status, kkt};
    const StreamIO t{path, path_entries, sstate, robot, traj, flags};
    const RArgs r{ticks, goal_tol, hist, traj_hist, ticks_run, replan, nullptr, replan_info, update_flags, disturb, tube_hist, audit, audit_tol, log_hist, log_stages, track,
                  legs, leg_tick, leg_on, leg_tol, legs_done, leg_fired, leg_why, tune, tune_info, tune_used, plant, plant_state, plant_info, plant_rec};
    const NArgs n{sensor, sensor_state, sensor_info, sensor_rec, sensor_noise, meas_hist};
    const OArgs o{observer, observer_state, observer_info, observer_rec, sample_hist};
    if (!bmpc_rollout_observer_ok(n, o)) return BMPC_ERR_ARG;      // (an observer without a sensor table or without its state)
    return rollout_launch(h, B, io, t, r, 6, (hipStream_t)hip_stream, sensor ? &n : nullptr, observer ? &o : nullptr);
}
// the sample and the estimate on their own, for per-tick loops in the place of bmpc_stream_sense (no workspace of the handle: may sit inside a capture)
extern "C" int bmpc_stream_observe(bmpc_handle *h, int B, double *robot, const double *sstate, const double *sensor, double *sensor_state, int *sensor_info, double *sensor_rec,
                                   const double *sensor_noise, double *meas, int tick, const double *observer, double *observer_state, int *observer_info,
                                   double *observer_rec, double *sample, void *hip_stream) {
    if (!h || B < 1 || !robot || !sstate || !sensor || !sensor_state || !observer || !observer_state || h->N > bmpcs::STREAM_NMAX) return BMPC_ERR_ARG;
    HIPCHK(bmpc_stream_observe_launch(h->N, B, h->h, robot, sstate, sensor, sensor_state, sensor_info, sensor_rec, sensor_noise, meas, tick, observer, observer_state,
                                      observer_info, observer_rec, sample, (hipStream_t)hip_stream));
    return BMPC_OK;
}

extern "C" int bmpc_stream_set_rt_feasibility_tol(bmpc_handle *h, double tol) {
    if (!h || !(tol > 0)) return BMPC_ERR_ARG;
    h->rt_viol_tol = tol;      // read at launch / capture time: re-capture a tick graph after changing it
    return BMPC_OK;
}
extern "C" int bmpc_stream_set_rt_position_row_cap(bmpc_handle *h, double cap_m2) {
    if (!h || !(cap_m2 >= 0.0)) return BMPC_ERR_ARG;
    h->rt_row_cap = cap_m2;      // read at launch / capture time: re-capture a tick graph after changing it
    return BMPC_OK;
}
extern "C" int bmpc_stream_set_time_budget(bmpc_handle *h, double microseconds) {
    if (!h || !(microseconds >= 0.0) || microseconds > 1e7) return BMPC_ERR_ARG;
    h->rt_budget_us = microseconds;      // read at launch / capture time: re-capture a tick graph after changing it
    return BMPC_OK;
}
extern "C" int bmpc_stream_lengths(const bmpc_handle *h, int *path_entry, int *state, int *robot, int *traj) {
    if (!h) return BMPC_ERR_ARG;
    if (path_entry) *path_entry = bmpcs::PT_LEN; if (state) *state = bmpcs::ss_len(h->N); if (robot) *robot = bmpcs::RB_LEN; if (traj) *traj = bmpcs::tr_len(h->N);
    return BMPC_OK;
}
extern "C" int bmpc_stream_pack(bmpc_handle *h, int B, const double *path, int path_entries, double *sstate, const double *robot, double *p, double *x0,
                                double *dual_state, void *hip_stream) {
    return bmpc_stream_pack_rt(h, B, path, path_entries, sstate, robot, p, x0, dual_state, nullptr, hip_stream);
}
extern "C" int bmpc_stream_pack_rt(bmpc_handle *h, int B, const double *path, int path_entries, double *sstate, const double *robot, double *p, double *x0,
                                   double *dual_state, const double *xlast, void *hip_stream) {
    if (!stream_args_ok(h, B, 0, path_entries, {path, sstate, robot, p, x0})) return BMPC_ERR_ARG;
    if (B == 0) return BMPC_OK;
    if (h->closed) return BMPC_ERR_ARG;
    hipLaunchKernelGGL(bmpc_stream_pack_kernel, dim3(B), dim3(64), 0, (hipStream_t)hip_stream, h->N, h->S, B, path, path_entries * bmpcs::PT_LEN,
                       sstate, robot, p, x0, dual_state, xlast, h->level_c, h->level_lo, h->level_hi);
    HIPCHK(hipGetLastError());
    return BMPC_OK;
}
extern "C" int bmpc_stream_post(bmpc_handle *h, int B, const double *path, int path_entries, double *sstate, double *robot, const double *x, const double *g,
                                const int *status, double *traj, int flags, void *hip_stream) {
    if (!stream_args_ok(h, B, 0, path_entries, {path, sstate, robot, x, g, status, traj})) return BMPC_ERR_ARG;
    if (B == 0) return BMPC_OK;
    hipLaunchKernelGGL(bmpc_stream_post_kernel, dim3(B), dim3(64), 0, (hipStream_t)hip_stream, h->N, h->S, B, h->h, path,
                       path_entries * bmpcs::PT_LEN, sstate, robot, x, g, status, traj, flags, h->rt_viol_tol, h->rt_row_cap);
    HIPCHK(hipGetLastError());
    return BMPC_OK;
}
extern "C" int bmpc_stream_log_len(const bmpc_handle *h) { return h ? bmpcs::log_len(h->N) : -1; }
// (no workspace of the handle is touched: no ordering event, and the launch may sit inside a capture of the caller's stream)
extern "C" int bmpc_stream_log(bmpc_handle *h, int B, const double *path, int path_entries, const double *sstate, const double *p, const double *traj, double *log,
                               void *hip_stream) {
    if (!stream_args_ok(h, B, 0, path_entries, {path, sstate, p, traj, log})) return BMPC_ERR_ARG;
    if (B == 0) return BMPC_OK;
    hipLaunchKernelGGL(bmpc_stream_log_kernel, dim3(B), dim3(64), 0, (hipStream_t)hip_stream, h->N, h->S, B, h->h, path, path_entries * bmpcs::PT_LEN, sstate, p, traj, log);
    HIPCHK(hipGetLastError());
    return BMPC_OK;
}
extern "C" int bmpc_stream_tube_len(void) { return BMPC_TUBE_LEN; }
// (like the log: no workspace of the handle, no ordering event, and the launch may sit inside a capture of the caller's stream)
extern "C" int bmpc_stream_tube(bmpc_handle *h, int B, const double *p, const double *sstate, double *tube, void *hip_stream) {
    if (!h || B < 1 || !p || !tube || h->N > bmpcs::STREAM_NMAX) return BMPC_ERR_ARG;
    HIPCHK(bmpc_stream_tube_launch(h->N, h->S, B, p, sstate, tube, (hipStream_t)hip_stream));
    return BMPC_OK;
}
extern "C" int bmpc_stream_replan_len(const bmpc_handle *h, int path_entries) { return (h && path_entries >= h->S + 1) ? bmpcs::replan_len(h->S, path_entries) : -1; }
// (like the log: no workspace of the handle, no ordering event, and the launch may sit inside a capture of the caller's stream)
extern "C" int bmpc_stream_update(bmpc_handle *h, int B, double *replan, double *path, int path_entries, double *sstate, double *robot, int *info, int flags,
                                  void *hip_stream) {
    if (B < 1 || !stream_args_ok(h, B, 0, path_entries, {replan, path, sstate}) || !bmpc_update_flags_ok(flags, robot)) return BMPC_ERR_ARG;
    if (flags & 2) hipLaunchKernelGGL(bmpc_stream_update_splice_kernel, dim3(B), dim3(64), 0, (hipStream_t)hip_stream, h->N, h->S, B, h->h, replan, path,
                                      path_entries * bmpcs::PT_LEN, sstate, robot, info, flags);
    else hipLaunchKernelGGL(bmpc_stream_update_kernel, dim3(B), dim3(64), 0, (hipStream_t)hip_stream, h->N, h->S, B, replan, path, path_entries * bmpcs::PT_LEN, sstate, robot,
                            info, flags);
    HIPCHK(hipGetLastError());
    return BMPC_OK;
}
// (no workspace of the handle either: may sit inside a capture)
extern "C" int bmpc_stream_disturb_len(void) { return BMPC_DIST_LEN; }
extern "C" int bmpc_stream_disturb(bmpc_handle *h, int B, double *robot, const double *d, void *hip_stream) {
    if (!h || B < 1 || !robot || !d) return BMPC_ERR_ARG;
    hipLaunchKernelGGL(bmpc_stream_disturb_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)hip_stream, B, robot, d);
    HIPCHK(hipGetLastError());
    return BMPC_OK;
}
// one closed-loop tick {pack, solve (warm-started, max_iter), post} captured into a hipGraph
extern "C" int bmpc_stream_graph_create(bmpc_handle *h, int B, const double *path, int path_entries, double *sstate, double *robot, double *p, double *x0,
                                        double *dual_state, int max_iter, double *x, double *g, int *iters, int *status, double *kkt, double *traj,
                                        int flags, bmpc_graph **out) {
    const SolveIO io{p, x0, dual_state, max_iter, x, g, nullptr, nullptr, nullptr, iters, status, kkt};
    const StreamIO t{path, path_entries, sstate, robot, traj, flags};
    if (!out || B < 1 || !tick_args_ok(h, B, io, t)) return BMPC_ERR_ARG;
    { const int rc_ = reserve_for_batch(h, B); if (rc_ != BMPC_OK) return rc_; }
    return capture_graph(h, out, [&](hipStream_t cs) { return enqueue_stream_tick(h, B, io, t, cs, true); });
}

#ifdef BMPC_PROFILE
// diagnostic build only: accumulated lane-0 cycle counts per phase (16 slots), then reset
extern "C" int bmpc_get_profile(bmpc_handle *h, unsigned long long *out) {
    if (!h || !out) return BMPC_ERR_ARG;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, h->prof, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(h->prof, 0, 32 * sizeof(unsigned long long)));
    return BMPC_OK;
}
#endif
extern "C" int bmpc_launch_info(const bmpc_handle *h, int *grid, int *lds_bytes, long long *scratch_bytes) {
    if (!h) return BMPC_ERR_ARG;
    if (grid) *grid = h->grid; if (lds_bytes) *lds_bytes = (int)(bmpc::L_SIZE * sizeof(double)); if (scratch_bytes) *scratch_bytes = h->scr_stride * 8;
    return BMPC_OK;
}
