"""Which kernel a batch is dispatched to (enqueue_solve in bmpc_hip.hip: one wave per problem, pairs, teams, the restoration instantiation as the
batch kernel) COMBINED with the rescue mechanisms a handle has switched on (restoration phase, second attempt), against the CPU oracle.  The
dispatch exists only on the GPU; the sets (tests/entry_path_sets.py) are a few dozen short-horizon problems on which those mechanisms decide the
outcome, and tests/test_entry_paths.py checks on the CPU that they do.

Status-4 hand-over from inside a SECOND attempt (a second attempt that jams or breaks down in a batch kernel is continued by the restoration kernel,
which starts its own attempt counter at 0): no test, because no input was found.  Searched on the CPU oracle for a row whose first attempt ends with
status 2 and whose second attempt alone (mu_init 0.1, slack_push 1e-2, start_rollout 1, max_iter 100, restoration off) ends with status 3:
  C' (below); A + Gaussian noise 1.0 (default_rng(11), with and without the uniform draw ahead of it, 64- and 128-row draws);
  workload.make_batch(64, seed=7, N=20) + default_rng(3).normal * 0.3 with start_rollout 0; rows 0:2048 of BASELINE configs[3] (N = 30, tight, seed 2).
Every second attempt of these pools converges, except 2 of configs[3] that run into the cap (status 1): none breaks down, so the path cannot be
reached from them and the code is left as it is."""
import ctypes

import numpy as np
import pytest

from tests import entry_path_sets as eps

pytestmark = pytest.mark.gpu

MARGIN = {"A": 6, "D": 8,      # the project's margins for these inputs: test_the_solver_does_not_depend_on_the_reference_warm_start, the g13b test
          "B": 2,              # the G12 starts (test_far_off_cold_starts_of_other_sizes); emulators vs oracle measured: 0 (tests/test_entry_paths.py)
          "C": 3, "C'": 3}     # emulator-versus-oracle gap measured in tests/test_entry_paths.py (max 1, on one row of C') + 2


def _gpu(name):
    import torch
    P, X, N, S, dt = eps.problem_set(name)
    return torch.tensor(P, device="cuda"), torch.tensor(X, device="cuda")


def _handle(name, mode, cap, waves=0):
    from boundmpc_amd import BatchedOCPSolver
    _, _, N, S, dt = eps.problem_set(name)
    s = BatchedOCPSolver(N, S, dt, start_rollout=False, restoration=mode)
    s.set_team_waves(waves); s.set_second_attempt(cap)
    return s


def _np(o):
    return o["status"].cpu().numpy(), o["iters"].cpu().numpy(), o["x"].cpu().numpy()


def _against_oracle(name, st, it, x, ref, tag):
    N = eps.problem_set(name)[2]
    gap = np.abs(it - ref["iters"])
    print(f"\n{tag}: status {eps.counts(st)} oracle {eps.counts(ref['status'])}; iteration gap max {gap.max()}, sum {it.sum()} oracle {ref['iters'].sum()}")
    assert np.array_equal(st, ref["status"]), (tag, eps.counts(st), eps.counts(ref["status"]))
    if name == "D":      # (the two that fail after three phases may leave at different counts)
        assert (gap[st == 0].max() if (st == 0).any() else 0) <= MARGIN[name] and (gap <= MARGIN[name]).sum() >= 36, (tag, gap)
    else:
        assert gap.max() <= MARGIN[name], (tag, gap)
    ok = st == 0
    if ok.any():
        assert eps.rms_q(x[ok], ref["x"][ok], N).max() < 1e-5, tag


SHAPE_ROWS = [("A", 0), ("A", 1), ("B", 0), ("B", 1), ("B", 2), ("D", 0), ("D", 1)]


@pytest.mark.parametrize("waves", [1, 2, 4, 0])
@pytest.mark.parametrize("name,mode", SHAPE_ROWS)
def test_second_attempt_on_every_launch_shape(name, mode, waves):
    """bmpc_set_second_attempt(100) on short-horizon handles, on one wave per problem, pairs, teams and the automatic choice (teams at these batch
    sizes), with the restoration phase off / full (/ after breakdowns only on B), against the oracle with the same options: statuses equal,
    iterations within the project's margin for the inputs, joint angles of the converged rows to 1e-5 rad RMS.  On A and B (modes 0, 2) a missing
    second attempt is 52 / 5 / 11 rows of status 2 where the oracle says 0.  On D the statuses stay and the status-2 rows must report the sum of both
    attempts.  The same handle with the cap at 0 against the oracle's cap-0 run is the control."""
    s = _handle(name, mode, 100, waves)
    try:
        p, x0 = _gpu(name)
        B = p.shape[0]
        if waves == 0:
            assert s.team_info(B)["waves"] != 1      # the automatic choice at these batch sizes is a multi-wave kernel
        else:
            assert s.team_info(B)["waves"] == waves
        st, it, x = _np(s.solve_batch(p, x0, out={}))
        ref = eps.oracle(name, mode, 100)
        _against_oracle(name, st, it, x, ref, f"{name} mode {mode} waves {waves} cap 100")
        s.set_second_attempt(0)
        st0, it0, x0_ = _np(s.solve_batch(p, x0, out={}))
        ref0 = eps.oracle(name, mode, 0)
        _against_oracle(name, st0, it0, x0_, ref0, f"{name} mode {mode} waves {waves} cap 0")
        if name == "D":
            s2 = st == 2
            assert (it[s2] > it0[s2]).all(), (it[s2], it0[s2])
            assert abs(int(it.sum()) - int(ref["iters"].sum())) <= 38 * 8, (it.sum(), ref["iters"].sum())
        if (name, mode) in eps.CAP_CHANGES_NOTHING:
            assert np.array_equal(st, st0) and np.array_equal(it, it0) and np.array_equal(x, x0_)
    finally:
        s.close()


@pytest.mark.parametrize("name", ["C", "C'"])
def test_restoration_modes_and_second_attempt_with_five_path_segments(name):
    """N = 6, S = 5: the iterate in the workspace (bmpc_solve_kernel<false>), where mode 1 -- the default -- sends the whole batch through
    bmpc_resto_kernel<false> as a fresh solve and mode 2 through bmpc_solve_kernel<false> plus a continuation.  A jam (C: noise 0.3) and a numerical
    breakdown (C': noise 1.0) in modes 0, 1 and 2, each with the second attempt off and at cap 100, against the oracle with the same options.
    Iteration margin 3 = the emulator-versus-oracle gap measured in tests/test_entry_paths.py (0 on C, max 1 on C') + 2.  Where the oracle's mode-1 and
    mode-2 verdicts agree the GPU's agree with each other too."""
    p, x0 = _gpu(name)
    got = {}
    for mode in (0, 1, 2):
        s = _handle(name, mode, 0)
        try:
            assert s.team_info(p.shape[0])["waves"] == 1      # no pair / team instantiation for S > 4
            for cap in (0, 100):
                s.set_second_attempt(cap)
                st, it, x = _np(s.solve_batch(p, x0, out={}))
                _against_oracle(name, st, it, x, eps.oracle(name, mode, cap), f"{name} mode {mode} cap {cap}")
                got[(mode, cap)] = st
        finally:
            s.close()
    for cap in (0, 100):
        agree = eps.oracle(name, 1, cap)["status"] == eps.oracle(name, 2, cap)["status"]
        assert np.array_equal(got[(1, cap)][agree], got[(2, cap)][agree])


def _raw_solve(s, B, p, x0, x, iters=None, status=None):
    """bmpc_solve_batch through the raw ABI (x may alias x0); returns the error code"""
    import torch
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    rc = s._lib.bmpc_solve_batch(s._h, B, ptr(p), ptr(x0), ptr(x), None, None, None, None, ptr(iters), ptr(status), None, None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("waves", [1, 2, 4])
@pytest.mark.parametrize("mode", [0, 1])
def test_in_place_solve_without_second_attempt_is_bit_equal(mode, waves):
    """x == x0 on set A with the second attempt off (the N <= 11 default): a problem's x0 is read in full before its x is written -- by the batch
    kernel and by the restoration kernel that continues a jammed problem from x -- so the in-place solve is the out-of-place solve bit for bit."""
    import torch
    s = _handle("A", mode, 0, waves)
    try:
        p, x0 = _gpu("A")
        B = p.shape[0]
        o = s.solve_batch(p, x0, out={})
        xio = x0.clone(); it = torch.zeros(B, dtype=torch.int32, device="cuda"); st = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        assert _raw_solve(s, B, p, xio, xio, it, st) == 0
        assert torch.equal(xio, o["x"]) and torch.equal(it, o["iters"]) and torch.equal(st, o["status"])
        assert eps.counts(st.cpu().numpy()) == eps.ORACLE_COUNTS[("A", mode)][0]
    finally:
        s.close()


def test_overlapping_x_and_x0_are_refused_while_the_second_attempt_is_on():
    """With cap > 0 the second attempt reads x0 again after x has been written: bmpc_solve_batch returns BMPC_ERR_ARG when the ranges overlap -- x == x0
    or shifted by one row -- launches nothing, and accepts ranges that only touch."""
    import torch
    from boundmpc_amd import _lib
    s = _handle("A", 0, 100)
    try:
        p, x0 = _gpu("A")
        B, nw = x0.shape
        buf = torch.cat([x0, x0]).contiguous()      # [2B][nw]
        before = buf.clone()
        assert _raw_solve(s, B, p, buf[:B], buf[:B]) == 1            # BMPC_ERR_ARG
        assert _raw_solve(s, B, p, buf[:B], buf[1:B + 1]) == 1       # x one row behind x0
        assert _raw_solve(s, B, p, buf[1:B + 1], buf[:B]) == 1       # x one row ahead of x0
        assert torch.equal(buf, before)
        with pytest.raises(RuntimeError):
            _lib.check(_raw_solve(s, B, p, buf[:B], buf[:B]), "bmpc_solve_batch")
        st = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        assert _raw_solve(s, B, p, buf[:B], buf[B:], None, st) == 0  # adjacent, not overlapping
        assert eps.counts(st.cpu().numpy()) == eps.ORACLE_COUNTS[("A", 0)][1] and torch.equal(buf[:B], before[:B])
        s.set_second_attempt(0)                                      # cap 0: in place is allowed again
        assert _raw_solve(s, B, p, buf[:B], buf[:B]) == 0
    finally:
        s.close()


# ---- growth of the handle-owned buffers (workspace, status stand-ins) ----
@pytest.fixture(scope="module")
def growth():
    """300 N = 10 problems, their first 8, and what a fresh default handle makes of each"""
    import torch
    from boundmpc_amd import BatchedOCPSolver, workload
    P, X, _ = workload.make_batch(300, seed=61, N=10)
    p, x0 = torch.tensor(P, device="cuda"), torch.tensor(X, device="cuda")
    p8, x8 = p[:8].contiguous(), x0[:8].contiguous()
    s = BatchedOCPSolver(10, 4, 0.1)
    fresh300 = {k: v.clone() for k, v in s.solve_batch(p, x0, out={}).items()}
    s.close()
    s = BatchedOCPSolver(10, 4, 0.1)
    fresh8 = {k: v.clone() for k, v in s.solve_batch(p8, x8, out={}).items()}
    s.close()
    assert (fresh300["status"] == 0).all()
    return dict(p=p, x0=x0, p8=p8, x8=x8, fresh300=fresh300, fresh8=fresh8)


def _same(a, b):
    import torch
    return all(torch.equal(a[k], b[k]) for k in ("x", "iters", "status", "f", "g", "lam_g", "lam_x"))


def test_growth_without_graphs_keeps_every_result(growth):
    """B = 8 (teams), then B = 300 (the workspace grows and the batch takes the pair kernel), then B = 8 again: the first and third results are
    bit-equal, the second is a fresh handle's."""
    from boundmpc_amd import BatchedOCPSolver
    s = BatchedOCPSolver(10, 4, 0.1)
    try:
        assert s.team_info(8)["waves"] != s.team_info(300)["waves"]
        a = {k: v.clone() for k, v in s.solve_batch(growth["p8"], growth["x8"], out={}).items()}
        b = s.solve_batch(growth["p"], growth["x0"], out={})
        c = s.solve_batch(growth["p8"], growth["x8"], out={})
        assert _same(a, c) and _same(a, growth["fresh8"]) and _same(b, growth["fresh300"])
    finally:
        s.close()


def test_growth_is_refused_cleanly_while_a_graph_is_alive(growth):
    """A step captured at B = 8 holds the workspace: a direct solve of B = 300 returns the error (no launch, no fault), the replay and a direct B = 8
    solve give the bits they gave before, and once the graph is closed B = 300 succeeds with a fresh handle's results."""
    import torch
    from boundmpc_amd import BatchedOCPSolver
    s = BatchedOCPSolver(10, 4, 0.1)
    try:
        want = ("g", "lam_g", "lam_x", "f", "iters", "status", "kkt")
        gr = s.capture_step(growth["p8"], growth["x8"], want=want)
        r0 = {k: v.clone() for k, v in gr.launch().items()}
        d0 = {k: v.clone() for k, v in s.solve_batch(growth["p8"], growth["x8"], out={}).items()}
        torch.cuda.synchronize()
        assert _same(r0, growth["fresh8"]) and _same(d0, growth["fresh8"])
        for _ in range(2):      # (refused every time, not only the first)
            with pytest.raises(RuntimeError):
                s.solve_batch(growth["p"], growth["x0"], out={})
        for v in gr.out.values():
            v.zero_()
        r1 = gr.launch()
        d1 = s.solve_batch(growth["p8"], growth["x8"], out={})
        torch.cuda.synchronize()
        assert _same(r1, r0) and _same(d1, d0)
        gr.close()
        assert _same(s.solve_batch(growth["p"], growth["x0"], out={}), growth["fresh300"])
        assert _same(s.solve_batch(growth["p8"], growth["x8"], out={}), growth["fresh8"])
    finally:
        s.close()


def test_null_status_and_iters_with_the_restoration_phase_on_while_the_stand_ins_grow():
    """The hand-over to the restoration kernel goes through status[] / iters[]; a caller that passes NULL gets handle-owned stand-ins, which grow
    with the batch: B = 8, then B = 40 of set D's rows (38, the first two repeated) -- x is bit-equal to a call that passes the buffers."""
    import torch
    from boundmpc_amd import BatchedOCPSolver
    P, X, N, S, dt = eps.problem_set("D")
    idx = np.arange(40) % 38
    p, x0 = torch.tensor(P[idx], device="cuda"), torch.tensor(X[idx], device="cuda")
    s = BatchedOCPSolver(N, S, dt, start_rollout=False)      # restoration at its default: the full phase
    ref = BatchedOCPSolver(N, S, dt, start_rollout=False)
    try:
        assert s.get_restoration()["mode"] == 1
        for B in (8, 40):
            pb, xb = p[:B].contiguous(), x0[:B].contiguous()
            o = ref.solve_batch(pb, xb, out={})
            x = torch.full((B, N * 44), float("nan"), dtype=torch.float64, device="cuda")
            assert _raw_solve(s, B, pb, xb, x) == 0
            assert torch.equal(x, o["x"])
            assert (o["status"] == 2).sum().item() >= B // 2      # (most of these went through the restoration kernel: the stand-ins carried the hand-over)
        r = eps.oracle("D", 1, 0)
        assert np.array_equal(o["status"].cpu().numpy(), r["status"][idx])
    finally:
        s.close(); ref.close()


def _settings_of(lib, h, N):
    """everything the ABI has a getter for, as a dict keyed like the option record (plus queue_order)"""
    from boundmpc_amd import _lib
    o, e, s_, c = _lib.Options(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.bmpc_default_options_for(N, ctypes.byref(o)) == 0 and lib.bmpc_get_restoration(h, ctypes.byref(e), ctypes.byref(s_), ctypes.byref(c)) == 0
    got = {f: getattr(o, f) for f, _ in _lib.Options._fields_}
    got.update(restoration=e.value, resto_short=s_.value, resto_cap=c.value, retry_cap=lib.bmpc_get_second_attempt(h),
               start_rollout=lib.bmpc_get_start_rollout(h), queue_order=lib.bmpc_get_queue_order(h))
    return got


@pytest.mark.parametrize("N,queue_order", [(11, 0), (12, 1)])
def test_a_handle_created_without_options_runs_the_horizon_rule(N, queue_order):
    """bmpc_create(opts = NULL) on both sides of the horizon cliff: what the getters of the ABI give back is the record of bmpc_opts_for
    (csrc/bmpc_args.h), read through the emulator, plus the queue order of that horizon.  Handle creation only, no solve."""
    from boundmpc_amd import _lib
    from tests.emu import emu
    lib, h = _lib.load(), ctypes.c_void_p()
    assert lib.bmpc_create(N, 4, 0.1, None, ctypes.byref(h)) == 0
    try:
        got, want = _settings_of(lib, h, N), emu.opts_for(N)
        assert got.pop("queue_order") == queue_order
        assert got == {f: getattr(want, f) for f in got}, (got, {f: getattr(want, f) for f in got})
    finally:
        lib.bmpc_destroy(h)


def test_explicit_options_replace_the_public_fields_only():
    """bmpc_create with a caller's bmpc_options at N = 12: what the public struct does not carry keeps the long horizon's defaults (restoration
    after a breakdown only, second attempt of 100 iterations, queue order on), and the public fields are the caller's.  The ABI has no getter for
    a handle's public fields (bmpc_default_options_for is a function of N alone), so one of them is read off one problem: with max_iter = 2
    the solve of a cold start ends after exactly 2 iterations as status 1."""
    import torch
    from boundmpc_amd import _lib, workload
    from tests.emu import emu
    lib, h = _lib.load(), ctypes.c_void_p()
    mine = _lib.Options(1e-8, 2, 0.5, 0.1, 0.05, 1, 1, 1e-2, 12, 0.0)
    assert lib.bmpc_create(12, 4, 0.1, ctypes.byref(mine), ctypes.byref(h)) == 0
    try:
        got, rule = _settings_of(lib, h, 12), emu.opts_for(12)
        for f in ("restoration", "resto_short", "resto_cap", "retry_cap", "start_rollout"):
            assert got[f] == getattr(rule, f), f
        assert got["restoration"] == 2 and got["resto_cap"] == 40 and got["retry_cap"] == 100 and got["queue_order"] == 1
        P, X, _ = workload.make_batch(1, seed=0, N=12, workers=1)
        p, x0 = torch.tensor(P, device="cuda"), torch.tensor(X, device="cuda")
        x, it, st = torch.empty_like(x0), torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())
        assert lib.bmpc_solve_batch(h, 1, ptr(p), ptr(x0), ptr(x), None, None, None, None, ptr(it), ptr(st), None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        torch.cuda.synchronize()
        assert int(it[0]) == 2 and int(st[0]) == 1, (int(it[0]), int(st[0]))
    finally:
        lib.bmpc_destroy(h)
