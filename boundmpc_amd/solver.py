"""Batched OCP solver handle and the CasADi-`nlpsol`-compatible single-problem shim.

`BatchedOCPSolver` is the torch-facing wrapper of the C ABI (PyTorch-ROCm tensors are used
for device memory and streams only).  `NlpSolverShim` mirrors the call convention of the
object the reference creates at casadi_ocp_formulation.py:389 and calls at
BoundMPC.py:446-456, so that `BoundMPC.step()` reads like the reference's."""
import ctypes

import numpy as np

from . import _lib

NZ, NG = 44, 43
# slots of the KKT certificate record (include/boundmpc_hip.h BMPC_KKT_*), in order
KKT_E, KKT_DUAL, KKT_PRIM_EQ, KKT_PRIM_INEQ, KKT_COMPL, KKT_LAM_EQ_GAP, KKT_LAM_INEQ_GAP, KKT_F = range(8)
KKT_FIELDS = ("E", "dual", "prim_eq", "prim_ineq", "compl", "lam_eq_gap", "lam_ineq_gap", "f")
# slots of the sensitivity record (include/boundmpc_hip.h BMPC_SENS_*), in order
SENS_STATUS, SENS_DELTA, SENS_RHS, SENS_DX = range(4)
SENS_FIELDS = ("status", "delta", "rhs", "dx_max")
# the outputs of a solve in the order of the C ABI: name -> (row length as an attribute of the solver, None: one number per problem; dtype)
SOLVE_OUTPUTS = {"x": ("n_w", "float64"), "g": ("n_g", "float64"), "lam_g": ("n_g", "float64"), "lam_x": ("n_w", "float64"), "f": (None, "float64"),
                 "iters": (None, "int32"), "status": (None, "int32"), "kkt": (None, "float64")}


def _ptr(a):
    """The address of a torch tensor or a numpy array for a ctypes call; None stays None (an optional argument left out)."""
    if a is None:
        return None
    return ctypes.c_void_p(a.data_ptr()) if hasattr(a, "data_ptr") else a.ctypes.data_as(ctypes.c_void_p)


def _stream_ptr(stream, device):
    """`stream`, or torch's current stream on `device`, as the stream argument of a ctypes call"""
    import torch
    return ctypes.c_void_p((stream if stream is not None else torch.cuda.current_stream(device)).cuda_stream)


def _multiplier_or_none(v):
    """None or a scalar 0 (the reference's initial `lam_g0 = 0`) means: no multipliers of that kind."""
    return None if v is None or (np.isscalar(v) and v == 0) else v


def _check_want(want, offered, what):
    bad = [k for k in want if k not in offered]
    if bad:
        raise ValueError(f"want {bad}: a {what} offers {offered}")


def _new(shape, dtype="float64", device=None):
    """An output array: a torch tensor on `device`, or (None) a zeroed numpy array."""
    if device is None:
        return np.zeros(shape, dtype=dtype)
    import torch
    return torch.empty(shape, dtype=getattr(torch, dtype), device=device)


def _directions(dp, B, point):
    """dp [B][n_p] or [B][D][n_p] (torch or numpy) -> D (None: one direction), the arrays of `point` with every row repeated D times (None stays
    None) and dp as [B D][n_p]."""
    if dp.ndim == 2:
        return None, point, dp
    D = dp.shape[1]
    if D < 1:
        raise ValueError("dp has no directions")
    tile = lambda a: None if a is None else (a.repeat_interleave(D, dim=0).contiguous() if hasattr(a, "repeat_interleave") else np.ascontiguousarray(np.repeat(a, D, axis=0)))
    return D, [tile(a) for a in point], dp.reshape(B * D, dp.shape[-1])


def _take_start_rollout_off(solver):
    """For a user of the caller's handle whose starts are the reference's own: start rollout off while it lives.  Returns the setting as found, for
    _give_start_rollout_back in its close() (None: an A/B library from before the option has no such entry point)."""
    was = solver.get_start_rollout() if hasattr(solver._lib, "bmpc_get_start_rollout") else None
    if was is not None:
        solver.set_start_rollout(False)
    return was


def _give_start_rollout_back(solver, was):
    if was is not None and getattr(solver, "_h", None):
        solver.set_start_rollout(was)


def _host_rows(*named):
    """(name, array, row length) ... -> B and the arrays as contiguous float64 [B][row length]; one ValueError names every shape."""
    arrs = [np.ascontiguousarray(np.atleast_2d(a), dtype=np.float64) for _, a, _ in named]
    B = arrs[0].shape[0]
    if any(a.shape != (B, n) for a, (_, _, n) in zip(arrs, named)):
        raise ValueError("shape mismatch: " + " ".join(f"{nm} {a.shape}" for a, (nm, _, _) in zip(arrs, named)))
    return [B] + arrs


class BatchedOCPSolver:
    def __init__(self, N, S, dt, tol=1e-8, max_iter=500, mu_init=None, slack_push=None, exact_hessian=True, mu_warm=1e-2, stall_window=None, bound_margin=0.0,
                 restoration=None, resto_short=None, resto_cap=None, start_rollout=None, mu_min_fac=None, fixed_barrier=None, level_c=0.02):
        self._lib = _lib.load()
        o = _lib.Options()
        self._lib.bmpc_default_options_for(int(N), ctypes.byref(o))      # mu_init 0.1 / slack_push 1e-2 for N <= 11, 3.0 / 0.1 for longer horizons
        if mu_init is None:
            mu_init = o.mu_init
        if slack_push is None:
            slack_push = o.slack_push
        o.tol, o.max_iter, o.mu_init, o.slack_push, o.exact_hessian = tol, int(max_iter), mu_init, slack_push, int(exact_hessian)
        if fixed_barrier is not None:
            # Real-time iteration on ONE barrier level (closed-loop ticks under a time budget, bench_stream.py rtfix-*): mu_init = mu_warm = final level =
            # fixed_barrier.  A tick then spends its few iterations as Newton steps on the barrier problem whose solution the previous tick left nearby,
            # instead of restarting the barrier at mu_warm and re-converging through its levels; `tol` never fires (the complementarity stays at the
            # level): the tick's budget or iteration cap ends it and the caller's acceptance rule decides.  256 closed loops at 1 kHz: 95.7 % of the
            # streams keep a plan at tick p99 0.96 ms with 0.1 (restarted barrier: 76.6 % at p99 1.00 ms; loops solved to 1e-8: 93.0 % at 12.5 ms).
            # fixed_barrier = "auto" (round 6) or a pair (lo, hi): the level sets itself per stream -- the handle HOLDS the level a solve starts on
            # (bmpc_set_barrier_hold) and the device-side pack writes clamp(c (phi_max - phi), lo, hi) into the stream's dual state
            # (bmpc_stream_set_level_rule): hi far from the end of the path, lower near it, where the barrier of phi <= phi_max would stall the stream.
            # "auto" = (0.01, 0.1) with level_c = 0.02: 94.9 % of the 256 benchmark streams keep their plan over 130 ticks (level 0.1: 95.7 %, 0.01: 87.5 %)
            # AND the reference's two experiments reach their goals after 161 / 64 ticks (0.1: stalls 0.21 / 0.37 short; 0.01: 160 / 62; solved to 1e-8: 155 / 59).
            auto = fixed_barrier == "auto" or isinstance(fixed_barrier, (tuple, list))
            lo, hi = (0.01, 0.1) if fixed_barrier == "auto" else ((float(fixed_barrier[0]), float(fixed_barrier[1])) if auto else (float(fixed_barrier),) * 2)
            mu_init, mu_warm = hi, lo
            mu_min_fac = lo / float(tol)
            self._level_rule = (level_c, lo, hi) if auto else None
        o.mu_init = mu_init if fixed_barrier is not None else o.mu_init
        o.mu_warm = mu_warm
        if mu_min_fac is not None:
            o.mu_min_fac = float(mu_min_fac)      # final barrier level = tol * mu_min_fac (default 0.1); mu_init = mu_warm = tol * mu_min_fac: a FIXED barrier level (real-time ticks)
        o.bound_margin = float(bound_margin)      # joint limits tightened inside the solver (real-time modes; 0 = the reference's limits)
        if stall_window is not None:
            o.stall_window = int(stall_window)      # default: 40 for N <= 11, 20 for longer horizons (bmpc_default_options_for)
        self._h = ctypes.c_void_p()
        _lib.check(self._lib.bmpc_create(int(N), int(S), float(dt), ctypes.byref(o), ctypes.byref(self._h)), "bmpc_create")
        if getattr(self, "_level_rule", None):
            _lib.check(self._lib.bmpc_set_barrier_hold(self._h, 1), "bmpc_set_barrier_hold")
            _lib.check(self._lib.bmpc_stream_set_level_rule(self._h, *[float(v) for v in self._level_rule]), "bmpc_stream_set_level_rule")
        # restoration phase (include/boundmpc_hip.h bmpc_set_restoration): None keeps the handle's default (on for N <= 11; 6 short steps; 40 iterations)
        if not (restoration is None and resto_short is None and resto_cap is None):
            self.set_restoration(restoration, resto_short, resto_cap)
        if start_rollout is not None:      # rollout of a cold start that is not a trajectory (bmpc_set_start_rollout; default on)
            self.set_start_rollout(start_rollout)
        self.N, self.S, self.dt = int(N), int(S), float(dt)
        self.n_w, self.n_g, self.n_p = N * NZ, N * NG, 141 + 91 * S
        self.state_len = int(self._lib.bmpc_state_len(self._h))
        import weakref
        self._children = weakref.WeakSet()      # captured graphs (StepGraph, StreamBatch): closed before the handle, see close()
        # the handle's workspace, work queue and occupancy belong to the device that was current at bmpc_create
        try:
            import torch
            self.device_index = torch.cuda.current_device() if torch.cuda.is_available() else None
        except Exception:
            self.device_index = None

    def close(self):
        """Destroys the captured graphs made from this handle first, then the handle (a graph destroyed later would still be safe --
        the C handle is reference-counted by its graphs -- but could no longer launch)."""
        if getattr(self, "_h", None):
            for c in list(getattr(self, "_children", ())):
                try:
                    c.close()
                except Exception:
                    pass
            self._lib.bmpc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- structural constants (casadi_ocp_formulation.py:384-391) ----
    def bounds(self):
        lbx, ubx, lbg, ubg = np.zeros(self.n_w), np.zeros(self.n_w), np.zeros(self.n_g), np.zeros(self.n_g)
        _lib.check(self._lib.bmpc_get_bounds(self._h, _ptr(lbx), _ptr(ubx), _ptr(lbg), _ptr(ubg)), "bmpc_get_bounds")
        return lbx, ubx, lbg, ubg

    def launch_info(self):
        g, l, s = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
        self._lib.bmpc_launch_info(self._h, ctypes.byref(g), ctypes.byref(l), ctypes.byref(s))
        return dict(grid=g.value, lds_bytes=l.value, scratch_bytes=s.value)

    def set_restoration(self, enabled=None, short_steps=None, cap=None):
        """Restoration phase of the solver (include/boundmpc_hip.h bmpc_set_restoration).  enabled: False / 0 never, True / 1 full (jam, stall, numerical
        breakdown; default for N <= 11), 2 after a numerical breakdown only (default for N > 11).  None keeps a value.  Re-capture graphs after changing it."""
        _lib.check(self._lib.bmpc_set_restoration(self._h, -1 if enabled is None else int(enabled), -1 if short_steps is None else int(short_steps),
                                                  -1 if cap is None else int(cap)), "bmpc_set_restoration")

    def set_start_rollout(self, enabled=True):
        """A stateless solve (solve_batch / solve_host without a dual state) whose x0 violates its own integrator chains by more than 0.5 starts from the
        rollout of x0's jerks (include/boundmpc_hip.h bmpc_set_start_rollout; default on; solves with a dual state and the reference's own starts are never touched).  Re-capture graphs after changing it."""
        _lib.check(self._lib.bmpc_set_start_rollout(self._h, int(bool(enabled))), "bmpc_set_start_rollout")

    def get_start_rollout(self):
        return bool(self._lib.bmpc_get_start_rollout(self._h))

    def get_restoration(self):
        e, s_, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.check(self._lib.bmpc_get_restoration(self._h, ctypes.byref(e), ctypes.byref(s_), ctypes.byref(c)), "bmpc_get_restoration")
        return dict(enabled=e.value == 1, mode=e.value, short_steps=s_.value, cap=c.value)

    def set_second_attempt(self, cap):
        """Iterations of the SECOND ATTEMPT of a stateless solve that ends with status 2: once more from x0 on the barrier start of the short horizons
        (mu 0.1, slacks pushed to 1e-2); iterations add up, a second attempt that hits its cap keeps status 2.  Default 100 for N > 11 (on BASELINE
        configs[3] 22 of the 26 status-2 problems are feasible and converge this way), 0 = off for shorter horizons (include/boundmpc_hip.h).  Holds on
        every launch shape (one wave per problem, pairs, teams: set_team_waves) and with every restoration mode.  With cap > 0 the output x of
        bmpc_solve_batch must not overlap x0 (the second attempt reads x0 again): an overlapping call is refused; solve_batch allocates its own x."""
        _lib.check(self._lib.bmpc_set_second_attempt(self._h, int(cap)), "bmpc_set_second_attempt")

    def get_second_attempt(self):
        return int(self._lib.bmpc_get_second_attempt(self._h))

    def set_queue_order(self, mode):
        """Work-queue order of a stateless batch larger than the resident waves: 1 = longest-expected-first by the objective at x0 (default for N > 11),
        0 = natural order (include/boundmpc_hip.h bmpc_set_queue_order).  Results do not depend on it."""
        _lib.check(self._lib.bmpc_set_queue_order(self._h, int(mode)), "bmpc_set_queue_order")

    def get_queue_order(self):
        return int(self._lib.bmpc_get_queue_order(self._h))

    def set_team_waves(self, waves=0):
        """Waves per problem: 0 (default) automatic -- a batch that fits into the resident teams of the device (256 on an MI355X) is solved by
        workgroups of 4 cooperating waves, one that fits into the resident pairs (512) by workgroups of 2, a larger one by one wave per problem;
        1 never teams; 2 pairs whatever the batch (N <= 11, S <= 4); 4 teams whenever the kernel exists (N <= 10, S <= 4).  Re-capture graphs after changing it."""
        _lib.check(self._lib.bmpc_set_team_waves(self._h, int(waves)), "bmpc_set_team_waves")

    def set_rollout_waves(self, waves=1):
        """Waves per stream of StreamBatch.rollout (include/boundmpc_hip.h bmpc_set_rollout_waves; set_team_waves does not apply there): 1 (default)
        one wave per stream; 4 a team of cooperating waves per stream whatever the batch, striding over the resident teams (N <= 10, S <= 4, else
        refused); 0 automatic -- teams when the batch fits into the resident teams, else one wave.  Read at launch time."""
        _lib.check(self._lib.bmpc_set_rollout_waves(self._h, int(waves)), "bmpc_set_rollout_waves")

    @property
    def rollout_waves(self):
        return int(self._lib.bmpc_get_rollout_waves(self._h))

    def team_info(self, B):
        w, r, l = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.check(self._lib.bmpc_team_info(self._h, int(B), ctypes.byref(w), ctypes.byref(r), ctypes.byref(l)), "bmpc_team_info")
        return dict(waves=w.value, resident_teams=r.value, lds_bytes=l.value)

    def tune_defaults(self, max_iter=0):
        """The row of controller settings (stream.TUNE, stream.unpack_tune) a rollout launched now with this max_iter argument reads from the handle:
        what an all-NaN row of StreamBatch.rollout(tune=...) resolves to (bmpc_stream_tune_defaults).  numpy [stream.TUNE["LEN"]], pad words 0."""
        row = np.zeros(int(self._lib.bmpc_stream_tune_len()))
        _lib.check(self._lib.bmpc_stream_tune_defaults(self._h, int(max_iter), _ptr(row)), "bmpc_stream_tune_defaults")
        return row

    def set_rt_position_row_cap(self, cap_m2):
        """Real-time stream ticks: a position tube row (l^2 - w^2 of any stage, m^2) above the cap vetoes the iterate (include/boundmpc_hip.h
        bmpc_stream_set_rt_position_row_cap; 0 = off, the default).  Set it before the tick graph is captured."""
        _lib.check(self._lib.bmpc_stream_set_rt_position_row_cap(self._h, float(cap_m2)), "bmpc_stream_set_rt_position_row_cap")

    def set_rt_feasibility_tol(self, tol):
        """Threshold of the reference's acceptance rule (summed violation of g, BoundMPC.py:462-465) that stream ticks in real-time mode
        apply to an iteration-capped iterate (default 1e-4, the reference's).  Set it before the tick graph is captured."""
        _lib.check(self._lib.bmpc_stream_set_rt_feasibility_tol(self._h, float(tol)), "bmpc_stream_set_rt_feasibility_tol")

    def set_time_budget_us(self, microseconds):
        """Time budget of a fused closed-loop tick (0 = none): no further solver iteration is started once it is used up
        (bmpc_stream_set_time_budget).  Set it before the tick graph is captured."""
        _lib.check(self._lib.bmpc_stream_set_time_budget(self._h, float(microseconds)), "bmpc_stream_set_time_budget")

    def set_timing(self, keep=1):
        """HIP events around the solver kernel on its launch stream; the pairs of the last `keep` launches are kept (0/False = off)."""
        _lib.check(self._lib.bmpc_set_timing(self._h, int(keep)), "bmpc_set_timing")

    def set_latency_buffer(self, buf):
        """buf: float64 GPU tensor [>= B] that receives each solve's in-kernel duration in microseconds, or None."""
        self._lat = buf          # keep it alive while registered
        _lib.check(self._lib.bmpc_set_latency_buffer(self._h, ctypes.c_void_p(buf.data_ptr()) if buf is not None else None), "bmpc_set_latency_buffer")

    def kernel_ms(self, back=0):
        """duration of the launch `back` launches ago (waits for its stop event only)."""
        ms = ctypes.c_float()
        _lib.check(self._lib.bmpc_kernel_ms(self._h, int(back), ctypes.byref(ms)), "bmpc_kernel_ms")
        return ms.value

    def last_kernel_ms(self):
        return self.kernel_ms(0)

    # ---- dual state of a receding-horizon stream (bmpc_solve_batch_warm) ----
    def new_state(self, B, device="cuda"):
        """Zeroed state = cold start on first use."""
        import torch
        return torch.zeros((B, self.state_len), dtype=torch.float64, device=device)

    def shift_state(self, state):
        """Advance the horizon by one stage, as the host does with x0 (BoundMPC.py:372-375): rows of node k+1 -> node k,
        last node duplicated.  In place."""
        nu = state[:, :self.N * 57].view(-1, self.N, 57)
        nu[:, :-1] = nu[:, 1:].clone()
        return state

    def _check_io(self, p, x0, state):
        import torch
        if not (p.is_cuda and x0.is_cuda and p.dtype == torch.float64 and x0.dtype == torch.float64):
            raise ValueError("p and x0 must be float64 tensors on the GPU")
        B = p.shape[0]
        if p.shape != (B, self.n_p) or x0.shape != (B, self.n_w):
            raise ValueError(f"shape mismatch: p {tuple(p.shape)} x0 {tuple(x0.shape)}")
        if not (p.is_contiguous() and x0.is_contiguous()):
            raise ValueError("p and x0 must be contiguous (the kernel reads them asynchronously on the launch stream; a temporary copy "
                             "made here could be recycled by the allocator before the kernel has run)")
        if self.device_index is not None and (p.device.index != self.device_index or x0.device.index != self.device_index):
            raise ValueError(f"p / x0 live on cuda:{p.device.index}, the solver handle was created on cuda:{self.device_index}")
        if state is not None and not (state.is_cuda and state.dtype == torch.float64 and state.is_contiguous()
                                      and state.shape == (B, self.state_len)):
            raise ValueError(f"state must be a contiguous float64 GPU tensor of shape ({B}, {self.state_len})")
        return B

    def _check_multipliers(self, B, lam_g0, lam_x0, dev):
        import torch
        for t, n, nm in ((lam_g0, self.n_g, "lam_g0"), (lam_x0, self.n_w, "lam_x0")):
            if t is None:
                continue
            if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.shape == (B, n)):
                raise ValueError(f"{nm} must be a contiguous float64 GPU tensor of shape ({B}, {n})")
            if t.device != dev:
                raise ValueError(f"{nm} lives on {t.device}, p on {dev}")

    def _host_multipliers(self, B, lam_g, lam_x, names):
        """The numpy multiplier pair of a host call as contiguous float64 [B][n_g] / [B][n_w], or None where there is none."""
        out = []
        for a, n, nm in ((lam_g, self.n_g, names[0]), (lam_x, self.n_w, names[1])):
            a = _multiplier_or_none(a)
            if a is not None:
                a = np.ascontiguousarray(np.atleast_2d(a), dtype=np.float64)
                if a.shape != (B, n):
                    raise ValueError(f"{nm} has shape {a.shape}, expected {(B, n)}")
            out.append(a)
        return out

    def _solve_shape(self, B, name):
        n = SOLVE_OUTPUTS[name][0]
        return (B, getattr(self, n)) if n else (B,)

    def _cert_shapes(self, B):
        return dict(cert=(B, len(KKT_FIELDS)), g=(B, self.n_g), lam_g=(B, self.n_g), rj=(B, 8 * self.N))

    def _sens_outputs(self, R, want_duals, device=None):
        shapes = dict(dx=(R, self.n_w), rec=(R, len(SENS_FIELDS)), dlam_eq=(R, 36 * self.N), dnu=(R, 57 * self.N))
        return {k: _new(shapes[k], device=device) for k in (("dx", "rec", "dlam_eq", "dnu") if want_duals else ("dx", "rec"))}

    def state_from_multipliers(self, p, x0, lam_g0=None, lam_x0=None, mu0=None, out=None, stream=None):
        """Dual state [B, state_len] of a warm solve (solve_batch(state=...)) from multipliers in CasADi's convention -- lam_g0 [B, 43 N],
        lam_x0 [B, 44 N], as a solve returns them; None = zeros -- evaluated at x0 on the GPU (include/boundmpc_hip.h bmpc_state_from_multipliers:
        the map, what is ignored, the barrier level).  mu0 > 0: the barrier level of the state, else the handle's mu_warm.  Asynchronous on `stream`."""
        import torch
        self._check_io(p, x0, out)
        B = p.shape[0]
        self._check_multipliers(B, lam_g0, lam_x0, p.device)
        state = out if out is not None else torch.empty((B, self.state_len), dtype=torch.float64, device=p.device)
        _lib.check(self._lib.bmpc_state_from_multipliers(self._h, B, _ptr(p), _ptr(x0), _ptr(lam_g0), _ptr(lam_x0), float(mu0 or 0.0), _ptr(state),
                                                         _stream_ptr(stream, p.device)), "bmpc_state_from_multipliers")
        self._inflight = (p, x0, lam_g0, lam_x0, state)      # (asynchronous launch: see solve_batch)
        return state

    # ---- KKT certificate of any primal-dual point (bmpc_kkt_batch) ----
    _CERT_WANT = ("g", "lam_g", "rj")

    def certify(self, p, x, lam_g=None, lam_x=None, want=(), out=None, stream=None):
        """The solver's error measure for points it need not have produced: p [B][n_p], x [B][n_w] and multipliers in CasADi's convention
        lam_g [B][n_g] / lam_x [B][n_w] (None or 0: none), all float64 contiguous GPU tensors.  Returns a dict with the fields KKT_FIELDS as [B]
        tensors (views of the record "cert" [B][8]) -- E is what a solve compares with tol -- plus the arrays named in `want`: "g" [B][n_g],
        "lam_g" [B][n_g] (the consistent multipliers: equality rows recomputed, inequality rows re-exported), "rj" [B][8 N].  The point is taken
        as given (no start rollout, no second attempt); the record, the gap slots and the non-finite rules: include/boundmpc_hip.h bmpc_kkt_batch.
        Asynchronous on `stream`; ordered against the handle's solves."""
        import torch
        lam_g, lam_x = _multiplier_or_none(lam_g), _multiplier_or_none(lam_x)
        B = self._check_io(p, x, None)
        self._check_multipliers(B, lam_g, lam_x, p.device)
        _check_want(want, self._CERT_WANT, "certificate")
        o = out if out is not None else {}
        dev = p.device
        shapes = self._cert_shapes(B)
        ptr = {}
        for k in ("cert",) + tuple(want):
            t = o.get(k)
            if t is None:
                t = o[k] = _new(shapes[k], device=dev)
            elif not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shapes[k] and t.device == dev):
                raise ValueError(f"out[{k!r}] must be a contiguous float64 GPU tensor of shape {shapes[k]} on {dev}")
            ptr[k] = t
        _lib.check(self._lib.bmpc_kkt_batch(self._h, B, _ptr(p), _ptr(x), _ptr(lam_g), _ptr(lam_x), _ptr(ptr["cert"]), _ptr(ptr.get("g")), _ptr(ptr.get("lam_g")),
                                            _ptr(ptr.get("rj")), _stream_ptr(stream, dev)), "bmpc_kkt_batch")
        self._inflight_cert = (p, x, lam_g, lam_x, o)      # (asynchronous launch: see solve_batch)
        for i, k in enumerate(KKT_FIELDS):
            o[k] = ptr["cert"][:, i]
        return o

    def certify_host(self, p, x, lam_g=None, lam_x=None, want=()):
        """certify with numpy in / out (bmpc_kkt_batch_host: staged copies, one synchronisation)."""
        B, p, x = _host_rows(("p", p, self.n_p), ("x", x, self.n_w))
        lam = self._host_multipliers(B, lam_g, lam_x, ("lam_g", "lam_x"))
        _check_want(want, self._CERT_WANT, "certificate")
        shapes = self._cert_shapes(B)
        o = {k: _new(shapes[k]) for k in ("cert",) + tuple(want)}
        _lib.check(self._lib.bmpc_kkt_batch_host(self._h, B, _ptr(p), _ptr(x), _ptr(lam[0]), _ptr(lam[1]), _ptr(o["cert"]), _ptr(o.get("g")), _ptr(o.get("lam_g")),
                                                 _ptr(o.get("rj"))), "bmpc_kkt_batch_host")
        for i, k in enumerate(KKT_FIELDS):
            o[k] = o["cert"][:, i]
        return o

    # ---- parametric sensitivity of the solution (bmpc_sens_batch) ----
    def sensitivity(self, p, x, dp, lam_g=None, lam_x=None, mu=None, stream=None, want_duals=False):
        """The tangent of the solution along a direction of the parameter vector: p [B][n_p], x [B][n_w], multipliers in CasADi's convention
        lam_g [B][n_g] / lam_x [B][n_w] (None or 0: zeros) -- usually a solve's outputs -- and dp [B][n_p] or [B][D][n_p] (D directions per problem:
        the point is tiled to B D rows and the results come back as [B][D][...]); float64 contiguous GPU tensors.  mu: the barrier level of the
        system (None: options.tol * options.mu_min_fac, the last level of a solve).  Returns a dict: "dx" [B](, D)[n_w], "rec" [B](, D)[4] (status,
        delta, max |rhs|, max |dx|: SENS_FIELDS) and, with want_duals, "dlam_eq" [..][36 N] and "dnu" [..][57 N].  The system, the record and the
        rules for non-finite input: include/boundmpc_hip.h bmpc_sens_batch.  Asynchronous on `stream`; ordered against the handle's solves."""
        import torch
        lam_g, lam_x = _multiplier_or_none(lam_g), _multiplier_or_none(lam_x)
        B = self._check_io(p, x, None)
        self._check_multipliers(B, lam_g, lam_x, p.device)
        if not (dp.is_cuda and dp.dtype == torch.float64 and dp.is_contiguous() and dp.device == p.device and dp.dim() in (2, 3) and dp.shape[0] == B
                and dp.shape[-1] == self.n_p):
            raise ValueError(f"dp must be a contiguous float64 GPU tensor of shape ({B}, {self.n_p}) or ({B}, D, {self.n_p}) on {p.device}")
        D, (p, x, lam_g, lam_x), dp = _directions(dp, B, (p, x, lam_g, lam_x))
        R = p.shape[0]
        dev = p.device
        o = self._sens_outputs(R, want_duals, dev)
        _lib.check(self._lib.bmpc_sens_batch(self._h, R, _ptr(p), _ptr(x), _ptr(lam_g), _ptr(lam_x), _ptr(dp), float(mu or 0.0), _ptr(o["dx"]), _ptr(o.get("dlam_eq")),
                                             _ptr(o.get("dnu")), _ptr(o["rec"]), _stream_ptr(stream, dev)), "bmpc_sens_batch")
        self._inflight_sens = (p, x, lam_g, lam_x, dp, o)      # (asynchronous launch: see solve_batch)
        if D is not None:
            o = {k: v.reshape(B, D, v.shape[-1]) for k, v in o.items()}
        return o

    def sensitivity_host(self, p, x, dp, lam_g=None, lam_x=None, mu=None, want_duals=False):
        """sensitivity with numpy in / out (bmpc_sens_batch_host: staged copies, one synchronisation)."""
        dp = np.ascontiguousarray(dp, dtype=np.float64)
        dp = dp[None, :] if dp.ndim == 1 else dp
        B, p, x = _host_rows(("p", p, self.n_p), ("x", x, self.n_w))
        if dp.ndim not in (2, 3) or dp.shape[0] != B or dp.shape[-1] != self.n_p:
            raise ValueError(f"shape mismatch: p {p.shape} x {x.shape} dp {dp.shape}")
        lam = self._host_multipliers(B, lam_g, lam_x, ("lam_g", "lam_x"))
        D, (p, x, *lam), dp = _directions(dp, B, (p, x, *lam))
        R = p.shape[0]
        o = self._sens_outputs(R, want_duals)
        _lib.check(self._lib.bmpc_sens_batch_host(self._h, R, _ptr(p), _ptr(x), _ptr(lam[0]), _ptr(lam[1]), _ptr(dp), float(mu or 0.0), _ptr(o["dx"]), _ptr(o.get("dlam_eq")),
                                                  _ptr(o.get("dnu")), _ptr(o["rec"])), "bmpc_sens_batch_host")
        if D is not None:
            o = {k: v.reshape(B, D, v.shape[-1]) for k, v in o.items()}
        return o

    # ---- batched device solve ----
    def solve_batch(self, p, x0, out=None, want=("g", "lam_g", "lam_x", "f", "iters", "status", "kkt"), stream=None, state=None, max_iter=0,
                    lam_g0=None, lam_x0=None):
        """p [B][n_p], x0 [B][n_w]: CUDA(ROCm) float64 contiguous tensors.  Returns dict of tensors.
        Asynchronous on `stream` (default: torch's current stream).  With `state` (see new_state) the solve is warm-started
        from it and updates it in place; `max_iter` > 0 caps the Newton steps of this call (real-time iteration).
        With multipliers lam_g0 [B][n_g] / lam_x0 [B][n_w] (CasADi's convention; either may be None) the solve is warm-started from the dual state
        state_from_multipliers makes of them, returned as out["state"]; multipliers and `state` together are refused."""
        self._check_io(p, x0, state)
        B = p.shape[0]
        o = out if out is not None else {}
        dev = p.device
        if lam_g0 is not None or lam_x0 is not None:
            if state is not None:
                raise ValueError("pass either multipliers (lam_g0 / lam_x0) or a dual state, not both")
            state = o["state"] = self.state_from_multipliers(p, x0, lam_g0, lam_x0, out=o.get("state"), stream=stream)

        given = [k for k in SOLVE_OUTPUTS if k == "x" or k in want]
        for k in given:
            if o.get(k) is None:
                o[k] = _new(self._solve_shape(B, k), SOLVE_OUTPUTS[k][1], dev)
        outs = [_ptr(o[k]) if k in given else None for k in SOLVE_OUTPUTS]
        st = _stream_ptr(stream, dev)
        if state is None and not max_iter:
            _lib.check(self._lib.bmpc_solve_batch(self._h, B, _ptr(p), _ptr(x0), *outs, st), "bmpc_solve_batch")
        else:
            if state is None:
                raise ValueError("max_iter per call needs a state buffer (new_state)")
            _lib.check(self._lib.bmpc_solve_batch_warm(self._h, B, _ptr(p), _ptr(x0), _ptr(state), int(max_iter), *outs, st), "bmpc_solve_batch_warm")
        # The launch is asynchronous: the kernel reads p / x0 / state and writes the outputs on the launch stream after this call has
        # returned.  The handle keeps them alive until its next launch (a caller that passes temporaries or drops the returned dict would
        # otherwise hand their memory back to the allocator while the kernel is still using it).
        self._inflight = (p, x0, state, o, lam_g0, lam_x0)
        return o

    def capture_step(self, p, x0, state=None, max_iter=0, want=("iters", "status", "kkt")):
        """hipGraph-captured step over FIXED buffers: returns a StepGraph whose launch() replays {queue reset, solver kernel};
        the caller refreshes p / x0 / state in place between launches and reads graph.out."""
        return StepGraph(self, p, x0, state, max_iter, want)

    # ---- host-buffer solve (numpy in/out) ----
    def solve_host(self, p, x0, lam_g0=None, lam_x0=None):
        """numpy in / out.  With multipliers lam_g0 [B][n_g] / lam_x0 [B][n_w] (either may be None): converted and warm-solved in the same
        single call (bmpc_solve_batch_host_dual); without: the stateless solve."""
        B, p, x0 = _host_rows(("p", p, self.n_p), ("x0", x0, self.n_w))
        lam = self._host_multipliers(B, lam_g0, lam_x0, ("lam_g0", "lam_x0"))
        out = {k: _new(self._solve_shape(B, k), dt) for k, (_, dt) in SOLVE_OUTPUTS.items()}
        outs = [_ptr(a) for a in out.values()]
        if lam[0] is None and lam[1] is None:
            _lib.check(self._lib.bmpc_solve_batch_host(self._h, B, _ptr(p), _ptr(x0), *outs), "bmpc_solve_batch_host")
        else:
            _lib.check(self._lib.bmpc_solve_batch_host_dual(self._h, B, _ptr(p), _ptr(x0), _ptr(lam[0]), _ptr(lam[1]), *outs), "bmpc_solve_batch_host_dual")
        return out


class StepGraph:
    """One solver step captured into a hipGraph (bmpc_graph_create / _launch / _destroy)."""

    def __init__(self, solver, p, x0, state, max_iter, want):
        B = solver._check_io(p, x0, state)
        if not (p.is_contiguous() and x0.is_contiguous()):
            raise ValueError("capture needs contiguous p and x0 (their addresses are baked into the graph)")
        self._solver, self.p, self.x0, self.state = solver, p, x0, state
        self.out = {k: _new(solver._solve_shape(B, k), SOLVE_OUTPUTS[k][1], p.device) for k in ("x",) + tuple(want)}
        self._g = ctypes.c_void_p()
        _lib.check(solver._lib.bmpc_graph_create(solver._h, B, _ptr(p), _ptr(x0), _ptr(state), int(max_iter), *[_ptr(self.out.get(k)) for k in SOLVE_OUTPUTS],
                                                 ctypes.byref(self._g)), "bmpc_graph_create")
        solver._children.add(self)

    def launch(self, stream=None):
        _lib.check(self._solver._lib.bmpc_graph_launch(self._g, _stream_ptr(stream, self.p.device)), "bmpc_graph_launch")
        return self.out

    def close(self):
        if getattr(self, "_g", None):
            self._solver._lib.bmpc_graph_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_STATUS = {0: "Solve_Succeeded", 1: "Maximum_Iterations_Exceeded", 2: "Infeasible_Problem_Detected", 3: "Error_In_Step_Computation"}


class NlpSolverShim:
    """Stands where `ca.nlpsol('solver','ipopt',prob,opts)` stands in the reference
    (casadi_ocp_formulation.py:389): `sol = solver(x0=, lbx=, ubx=, lbg=, ubg=, p=)` returns a
    dict with 'x','f','g','lam_x','lam_g' (column vectors like CasADi DMs); `stats()` returns
    'iter_count', 'success', 'return_status' (BoundMPC.py:446-474)."""

    def __init__(self, batched: BatchedOCPSolver):
        self._s = batched
        # behind the reference's BoundMPC every x0 is the reference's own (its cold start or a shifted plan, BoundMPC.py:316-375): taken as given, like Ipopt does
        # (a setting of the caller's handle, kept while the shim lives: close() puts the previous value back)
        self._rollout_was = _take_start_rollout_off(batched)
        self._stats = {"iter_count": 0, "success": False, "return_status": "not run"}
        self._lbx, self._ubx, self._lbg, self._ubg = batched.bounds()

    def close(self):
        """Gives the batched solver back as it was found (the start-rollout setting); the handle itself stays the caller's."""
        _give_start_rollout_back(self._s, getattr(self, "_rollout_was", None))
        self._rollout_was = None

    def generate_dependencies(self, *a, **k):   # BoundMPC.py:155-157 -- nothing to generate
        return None

    def __call__(self, x0=None, lbx=None, ubx=None, lbg=None, ubg=None, p=None, lam_x0=None, lam_g0=None):
        # the bound vectors are structural constants of the formulation; refuse silently different ones
        for given, mine, nm in ((lbx, self._lbx, "lbx"), (ubx, self._ubx, "ubx"), (lbg, self._lbg, "lbg"), (ubg, self._ubg, "ubg")):
            if given is not None and not np.array_equal(np.asarray(given, dtype=float).ravel(), mine):
                raise ValueError(f"{nm} differs from the formulation's structural bounds (casadi_ocp_formulation.py:92-153,272-349)")
        # multipliers (CasADi broadcasting: a scalar, or a column / flat vector of the right length); None or all zeros (the reference's initial
        # `self.lam_g0 = 0`) is the stateless call, otherwise a primal-dual warm start (include/boundmpc_hip.h bmpc_state_from_multipliers)
        lg, lx = self._multiplier(lam_g0, self._s.n_g, "lam_g0"), self._multiplier(lam_x0, self._s.n_w, "lam_x0")
        p_, x0_ = np.asarray(p, dtype=float).ravel()[None, :], np.asarray(x0, dtype=float).ravel()[None, :]
        if lg is None and lx is None:
            out = self._s.solve_host(p_, x0_)
        else:
            out = self._s.solve_host(p_, x0_, lam_g0=lg, lam_x0=lx)
        st = int(out["status"][0])
        self._stats = {"iter_count": int(out["iters"][0]), "success": st == 0, "return_status": _STATUS.get(st, f"status_{st}"),
                       "kkt_error": float(out["kkt"][0])}
        col = lambda a: np.asarray(a[0]).reshape(-1, 1)
        sol = {"x": col(out["x"]), "f": float(out["f"][0]), "g": col(out["g"]), "lam_x": col(out["lam_x"]), "lam_g": col(out["lam_g"])}
        self._last = (p_.copy(), sol)
        return sol

    def certificate(self, sol=None):
        """KKT certificate (BatchedOCPSolver.certify_host: dict of the fields KKT_FIELDS, floats) of a CasADi-style result -- a dict with 'x' and,
        where known, 'lam_g' / 'lam_x' (columns, flat vectors or a scalar, like the multiplier arguments of a call) -- for the parameter vector of the
        LAST call.  Default: the last solution.  Any solver's answer to the same problem can be scored: Ipopt's, a candidate warm start."""
        p_, x, lg, lx = self._point_of_last_call(sol, "certificate() needs a previous solver(...) call: it certifies a point for that call's p")
        c = self._s.certify_host(p_, x, lam_g=lg, lam_x=lx)
        return {k: float(c[k][0]) for k in KKT_FIELDS}

    def sensitivity(self, dp, sol=None):
        """Tangent of the solution along dp (flat [n_p] or [D][n_p]) for the parameter vector of the LAST call, at a CasADi-style result `sol`
        (default: the last solution), like certificate().  Returns {'dx': [n_w] or [D][n_w], 'rec': ...} (BatchedOCPSolver.sensitivity_host)."""
        p_, x, lg, lx = self._point_of_last_call(sol, "sensitivity() needs a previous solver(...) call: it differentiates that call's solution with respect to its p")
        dp = np.asarray(dp, dtype=float)
        one = dp.ndim == 1 or (dp.ndim == 2 and dp.shape[1] == 1)
        d3 = dp.reshape(1, 1, -1) if one else dp.reshape(1, dp.shape[0], -1)
        o = self._s.sensitivity_host(p_, x, d3, lam_g=lg, lam_x=lx)
        return {k: (v[0, 0] if one else v[0]) for k, v in o.items()}

    def _point_of_last_call(self, sol, complaint):
        """p of the last call and the point `sol` (None: the last solution) as [1][n] rows: p, x, lam_g, lam_x (None: no multipliers of that kind)"""
        if getattr(self, "_last", None) is None:
            raise RuntimeError(complaint)
        p_, last = self._last
        sol = last if sol is None else sol
        x = np.asarray(sol["x"], dtype=float).ravel()[None, :]
        return p_, x, self._multiplier(sol.get("lam_g"), self._s.n_g, "lam_g"), self._multiplier(sol.get("lam_x"), self._s.n_w, "lam_x")

    @staticmethod
    def _multiplier(v, n, name):
        """[1, n] float64 array of a multiplier argument, or None for None / all zeros."""
        if v is None:
            return None
        a = np.asarray(v, dtype=float)
        if a.size == 1:
            a = np.full(n, float(a.ravel()[0]))
        elif a.ndim > 2 or (a.ndim == 2 and 1 not in a.shape) or a.size != n:
            raise ValueError(f"{name} has shape {a.shape}: expected a scalar or a vector of length {n}")
        a = a.ravel()
        return None if not a.any() else a[None, :]

    def stats(self):
        return dict(self._stats)
