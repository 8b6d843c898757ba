"""TEST-ONLY: ctypes bindings of the CPU lane emulators of the wave program (tests/emu/*.cpp) and the one place that builds them: solves, the stream
functions one by one, and the fused tick as its kernel entry text (stream_tick, one wave or a team).  Beside it: emu_rollout.py (the rollout text in
all its variants, bmpc_emu_rollout.cpp per BMPC_NW, and the contract's loop), emu_stream_update.py (re-plan, splice, disturb), emu_stream_log.py, emu_stream_tube.py.  Modes of a solve (poison, in_kernel) are
arguments, nothing is read from the environment.  Not part of the product; see the header of bmpc_emu.cpp."""
import ctypes
import functools
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "boundmpc_amd", "csrc")
# what every emulator is built from beside its own source: the host header, the kernels' entry records and slicers, the wave program
_COMMON = [os.path.join(_HERE, "bmpc_emu_host.h"), os.path.join(_CSRC, "bmpc_args.h"), os.path.join(_CSRC, "bmpc_wave.inl")]
_STREAM = ("bmpc_stream.inl", "bmpc_tick_kernel.inl")      # what bmpc_emu.cpp reads of csrc beside them


class Opts(ctypes.Structure):
    _fields_ = [("tol", ctypes.c_double), ("max_iter", ctypes.c_int), ("mu_init", ctypes.c_double),
                ("mu_min_fac", ctypes.c_double), ("slack_push", ctypes.c_double),
                ("exact_hessian", ctypes.c_int), ("verbose", ctypes.c_int), ("mu_warm", ctypes.c_double), ("stall_window", ctypes.c_int),
                ("bound_margin", ctypes.c_double), ("restoration", ctypes.c_int), ("resto_short", ctypes.c_int), ("resto_cap", ctypes.c_int), ("start_rollout", ctypes.c_int), ("hold_mu", ctypes.c_int), ("retry_cap", ctypes.c_int)]


@functools.lru_cache(maxsize=None)
def _build(lib_name, source, flags=(), deps=()):
    """tests/emu/<lib_name>, loaded: compiled from tests/emu/<source> with `flags` when it is missing or older than the source, the common files
    or one of `deps` (files of csrc).  Cached: the staleness test runs once per process and library."""
    path, src = os.path.join(_HERE, lib_name), os.path.join(_HERE, source)
    if not os.path.exists(path) or any(os.path.getmtime(path) < os.path.getmtime(s) for s in [src] + _COMMON + [os.path.join(_CSRC, d) for d in deps]):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-Wno-unknown-pragmas", "-Wno-enum-compare", *flags, "-o", path, src])
    return ctypes.CDLL(path)


def lib():
    """the one-wave emulator: solves, the stream functions, the library's option rule and the debug entries"""
    L = _build("libbmpc_emu.so", "bmpc_emu.cpp", ("-fopenmp", "-DBMPC_NW=1"), _STREAM)
    assert L.bmpc_emu_opts_size() == ctypes.sizeof(Opts), "tests/emu/emu.py Opts is not the wave program's option record"
    return L


def build():
    """puts the one-wave library in place (for callers that start worker processes next); returns nothing"""
    lib()


def service_lib(kind):
    """kind = "dual" / "kkt" / "sens": the service job of csrc/bmpc_<kind>.inl over the one-wave emulator (tests/emu/bmpc_emu_<kind>.cpp)"""
    return _build(f"libbmpc_emu_{kind}.so", f"bmpc_emu_{kind}.cpp", (), ("bmpc_dual.inl", f"bmpc_{kind}.inl"))


def opts_for(N, opts=None, **kw):
    """`opts`, or the defaults of a handle for this horizon -- the library's own rule (csrc/bmpc_args.h bmpc_opts_for) -- with the fields of `kw` replaced"""
    if opts is not None:
        return opts
    o = Opts()
    lib().bmpc_emu_opts_for(ctypes.c_int(N), ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_opts(**kw):
    """the record of the short horizons"""
    return opts_for(lib().bmpc_emu_short_nmax(), **kw)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _solve(entry, p, x0, N, S, h, opts, lane_order, wave_order, nthreads, state, poison=False, in_kernel=False):
    p = np.ascontiguousarray(np.atleast_2d(p), dtype=np.float64)
    x0 = np.ascontiguousarray(np.atleast_2d(x0), dtype=np.float64)
    B = p.shape[0]
    out = dict(x=np.zeros((B, N * 44)), g=np.zeros((B, N * 43)), lam_g=np.zeros((B, N * 43)), lam_x=np.zeros((B, N * 44)),
               f=np.zeros(B), iters=np.zeros(B, dtype=np.int32), status=np.zeros(B, dtype=np.int32), kkt=np.zeros(B))
    rc = entry(ctypes.c_int(N), ctypes.c_int(S), ctypes.c_double(h), ctypes.byref(opts_for(N, opts)), ctypes.c_int(B), _p(p), _p(x0), _p(state),
               _p(out["x"]), _p(out["g"]), _p(out["lam_g"]), _p(out["lam_x"]), _p(out["f"]), _p(out["iters"]), _p(out["status"]), _p(out["kkt"]),
               ctypes.c_int(lane_order), ctypes.c_int(wave_order), ctypes.c_int(nthreads), ctypes.c_int(int(bool(poison)) | 2 * int(bool(in_kernel))))
    assert rc == 0
    return out


def solve(p, x0, N, S, h, opts=None, lane_order=0, nthreads=0, state=None, poison=False, in_kernel=False):
    """The one-wave program on the CPU, lanes in `lane_order` (0 forward, 1 reverse, 2 scrambled).  poison: LDS and workspace hold NaN before every
    problem.  in_kernel: the solve of a fused tick (its instantiation, the restoration phase inside) on raw (p, x0), which yields only x, g, kkt,
    iters and status: lam_g, lam_x and f stay zero and are no results."""
    return _solve(lib().bmpc_emu_solve, p, x0, N, S, h, opts, lane_order, 0, nthreads, state, poison, in_kernel)


# ---- team variant of the wave program (tests/emu/bmpc_emu.cpp with BMPC_NW cooperating waves per problem) ----
def team_lib(nw=4):
    """nw = 4 / 2: teams (workspace rows in LDS); nw = "pair": the two-wave team with the workspace in the global slab (BMPC_WSG, csrc/bmpc_pair.hip)"""
    pair = nw == "pair"
    L = _build("libbmpc_emu_pair.so" if pair else f"libbmpc_emu_team{nw}.so", "bmpc_emu.cpp", ("-fopenmp",) + (("-DBMPC_NW=2", "-DBMPC_WSG") if pair else (f"-DBMPC_NW={nw}",)), _STREAM)
    assert L.bmpc_emu_team_waves() == (2 if pair else nw)
    return L


def solve_team(p, x0, N, S, h, nw=4, opts=None, lane_order=0, wave_order=0, nthreads=0, state=None, poison=False):
    """The team program (nw waves per problem) on the CPU: wide phases run wave after wave in `wave_order` (0 forward, 1 reverse,
    2 scrambled), lanes in `lane_order`; poison as in solve."""
    return _solve(team_lib(nw).bmpc_emu_team_solve, p, x0, N, S, h, opts, lane_order, wave_order, nthreads, state, poison)


def newton(p, x, t, nu, mu, delta, N, S, h, nw=1, opts=None, lane_order=0, wave_order=0):
    """ONE Newton direction of the wave program at the interior point (x, t, nu) on the barrier level mu with the regularisation delta, through the
    calls of wave_solve's Newton system (bmpc_emu.cpp EMU_NEWTON); nw = 1, 4, 2 or "pair".  Returns (rc, KT [N][8][35], KF [N][8], dZ [44 N]);
    rc 0, or 3 where a stage block is not positive definite (the arrays are zero then)."""
    a = [np.ascontiguousarray(v, dtype=np.float64).ravel() for v in (p, x, t, nu)]
    assert a[0].size == 141 + 91 * S and a[1].size == 44 * N and a[2].size == 57 * N and a[3].size == 57 * N
    kt, kf, dz = np.zeros((N, 8, 35)), np.zeros((N, 8)), np.zeros(44 * N)
    entry = lib().bmpc_emu_newton if nw == 1 else team_lib(nw).bmpc_emu_team_newton
    rc = entry(ctypes.c_int(N), ctypes.c_int(S), ctypes.c_double(h), ctypes.byref(opts if opts is not None else default_opts()), *[_p(v) for v in a],
               ctypes.c_double(mu), ctypes.c_double(delta), _p(kt), _p(kf), _p(dz), ctypes.c_int(lane_order), ctypes.c_int(wave_order))
    assert rc in (0, 3), rc
    return rc, kt, kf, dz


# ---- CPU build of the stream functions (boundmpc_amd/csrc/bmpc_stream.inl) ----
def stream_lengths(N):
    out = (ctypes.c_int * 4)()
    lib().bmpc_emu_stream_lengths(ctypes.c_int(N), out)
    return dict(path_entry=out[0], state=out[1], robot=out[2], traj=out[3])


def stream_pack(N, S, path, ss, rb, dual=None, xlast=None, level_rule=(0.0, 0.0, 0.0)):
    """path [M][48], ss (updated in place), rb -> (p, x0); xlast: the solver's previous iterate (real-time continuation, bmpc_stream_pack_rt)"""
    p = np.zeros(141 + 91 * S); x0 = np.zeros(44 * N)
    assert path.flags.c_contiguous and ss.flags.c_contiguous and rb.flags.c_contiguous
    lib().bmpc_emu_stream_pack(ctypes.c_int(N), ctypes.c_int(S), _p(path), _p(ss), _p(rb), _p(p), _p(x0), _p(dual) if dual is not None else None,
                               _p(np.ascontiguousarray(xlast, dtype=np.float64)) if xlast is not None else None, ctypes.c_double(level_rule[0]), ctypes.c_double(level_rule[1]), ctypes.c_double(level_rule[2]))
    return p, x0


def stream_post(N, S, h, path, ss, rb, x, g, status, simulate=True, rt_tol=1e-4, flags=0, rt_row_cap=0.0):
    """flags: extra bits of the post flags (bit 1 = real-time acceptance rule)"""
    traj = np.zeros(stream_lengths(N)["traj"])
    x = np.ascontiguousarray(x, dtype=np.float64); g = np.ascontiguousarray(g, dtype=np.float64)
    lib().bmpc_emu_stream_post(ctypes.c_int(N), ctypes.c_int(S), ctypes.c_double(h), _p(path), _p(ss), _p(rb), _p(x), _p(g), ctypes.c_int(int(status)),
                               _p(traj), ctypes.c_int(int(simulate) | int(flags)), ctypes.c_double(rt_tol), ctypes.c_double(rt_row_cap))
    return traj


def stream_tick(N, S, h, T, A, max_iter=0, warm_dual=True, accept_capped=False, simulate=True, opts=None, rt_tol=1e-4, rt_row_cap=0.0, level_rule=(0.0, 0.0, 0.0),
                lane_order=0, wave_order=0, nw=1, want_rc=False):
    """ONE fused tick as the kernel entry text runs it (csrc/bmpc_tick_kernel.inl; nw = 1: one wave per stream, else the team's) on the tick arrays `A`
    (tests/emu/emu_rollout.py fresh_arrays; B streams: every array with a leading axis of B, T [B][M][48]), advanced in place.  Returns the entry's
    return code with want_rc (1: the arguments the C ABI refuses; A[k] = None passes NULL), else asserts it 0."""
    T = np.ascontiguousarray(T, dtype=np.float64)
    B = 1 if T.ndim == 2 else T.shape[0]
    assert all(v is None or v.flags.c_contiguous for v in A.values())
    c = ctypes
    entry = lib().bmpc_emu_stream_tick if nw == 1 else team_lib(nw).bmpc_emu_team_stream_tick
    rc = entry(c.c_int(N), c.c_int(S), c.c_double(h), c.byref(opts_for(N, opts)), c.c_int(B), _p(T), c.c_int(T.shape[-2]), _p(A["ss"]), _p(A["rb"]), _p(A["p"]),
               _p(A["x0"]), _p(A["dual"]) if warm_dual else None, c.c_int(int(max_iter)), _p(A["x"]), _p(A["g"]), _p(A["iters"]), _p(A["status"]), _p(A["kkt"]),
               _p(A["traj"]), c.c_int(int(bool(simulate)) | (2 if accept_capped else 0)), c.c_double(rt_tol), c.c_double(rt_row_cap), c.c_double(level_rule[0]),
               c.c_double(level_rule[1]), c.c_double(level_rule[2]), c.c_int(lane_order), c.c_int(wave_order))
    if want_rc:
        return rc
    assert rc == 0


def jacobian_lin_ddot(q, dq, ddq):
    """Second time derivative of the linear rows of the Jacobian (csrc/bmpc_stream.inl) -> [3][7]."""
    a = [np.ascontiguousarray(v, dtype=np.float64) for v in (q, dq, ddq)]
    out = np.zeros((3, 7))
    lib().bmpc_emu_jacobian_lin_ddot(_p(a[0]), _p(a[1]), _p(a[2]), _p(out))
    return out


def fk_motion(q, dq, ddq, u):
    """Pose, v = J dq, a = J ddq + dJ dq and the linear rows of J u + dJ ddq + ddJ dq in one pass over the chain (csrc/bmpc_stream.inl fk_motion)."""
    a = [np.ascontiguousarray(v, dtype=np.float64) for v in (q, dq, ddq, u)]
    out = np.zeros(21)
    lib().bmpc_emu_fk_motion(_p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), _p(out))
    return out[:6], out[6:12], out[12:18], out[18:21]


# ---- flop-counting build of the same kernel text (tests/emu/bmpc_emu_flops.cpp) ----
def count_flops(p, x0, N, S, h, opts=None):
    """fp64 operations the kernel text executes (summed over the lanes of every phase) while solving the batch: dict with iterations,
    converged, flops, special, flops_per_iteration, per_phase (slot id of tests/gpu_profile_phases.py -> flops)."""
    _fl = _build("libbmpc_emu_flops.so", "bmpc_emu_flops.cpp", ("-Wno-format",))
    p = np.ascontiguousarray(np.atleast_2d(p), dtype=np.float64)
    x0 = np.ascontiguousarray(np.atleast_2d(x0), dtype=np.float64)
    out = np.zeros(36, dtype=np.uint64)
    rc = _fl.bmpc_emu_count_flops(ctypes.c_int(N), ctypes.c_int(S), ctypes.c_double(h), ctypes.byref(opts_for(N, opts)), ctypes.c_int(p.shape[0]), _p(p), _p(x0), _p(out))
    assert rc == 0
    its = int(out[0])
    return dict(iterations=its, converged=int(out[1]), flops=int(out[2]), special=int(out[3]), flops_per_iteration=float(out[2]) / max(its, 1),
                per_phase={i: int(out[4 + i]) for i in range(32) if out[4 + i]})


# ---- mask-aware flop count of the same kernel text (tests/emu/bmpc_emu_useful.cpp): executed vs useful operations by data flow ----
def count_useful(p, x0, N, S, h, opts=None):
    """ONE problem: fp64 operations the kernel text executes and, of those, the ones whose result reaches a store (not the dummy word, not a
    clamped duplicate within the phase) or a decision.  dict: iterations, executed, useful, stores, duplicate_stores, dummy_stores,
    per_phase {slot: (executed, useful)}."""
    _ul = _build("libbmpc_emu_useful.so", "bmpc_emu_useful.cpp", ("-Wno-format",))
    p = np.ascontiguousarray(np.asarray(p, dtype=np.float64).ravel()); x0 = np.ascontiguousarray(np.asarray(x0, dtype=np.float64).ravel())
    out = np.zeros(72, dtype=np.uint64)
    rc = _ul.bmpc_emu_count_useful(ctypes.c_int(N), ctypes.c_int(S), ctypes.c_double(h), ctypes.byref(opts_for(N, opts)), _p(p), _p(x0), _p(out))
    assert rc == 0
    return dict(iterations=int(out[0]), converged=int(out[1]), executed=int(out[2]), useful=int(out[3]), stores=int(out[4]), duplicate_stores=int(out[5]),
                dummy_stores=int(out[6]), per_phase={s_: (int(out[8 + 2 * s_]), int(out[9 + 2 * s_])) for s_ in range(32) if out[8 + 2 * s_]})

