"""GPU: the rollout (bmpc_stream_rollout of the C ABI, StreamBatch.rollout) -- many closed-loop ticks of every stream in one launch -- against its exact
checker, T direct launches of the one-wave fused tick on a twin batch (bit for bit on every tick array, `hist` and `traj_hist` against the per-tick
reads), against the g++ build of the same kernel text, over more streams than resident workgroups (the stride), with the stop rules (lost plan, goal),
ordered against a graph replay on another stream of the same handle, and the argument errors of the entry point."""
import numpy as np
import pytest

from tests.rollout_contract import ARRAYS, assert_equal as _assert_equal, batch as _batch, close as _close, per_tick as _per_tick, small_streams as _small_streams, snapshot as _snapshot

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["converged", "held"])
def test_rollout_equals_direct_one_wave_ticks_bit_for_bit(mode):
    """B = 3 distinct streams at (2, 2), tick 0 solved out, then T = 6: rollout(T) on one batch, T tick() calls on one wave per stream on its twin.
    converged: to tolerance with the dual state carried; held: the held-barrier real-time mode, five iterations a tick, the real-time acceptance rule."""
    import torch
    N, S, T = 2, 2, 6
    mpcs, recs = _small_streams(N, S)
    held = mode == "held"
    kw = dict(max_iter=5, warm_dual=True, accept_capped=True) if held else dict(max_iter=0, warm_dual=True)
    a, b = _batch(N, S, mpcs, recs, one_wave=True, held=held), _batch(N, S, mpcs, recs, one_wave=True, held=held)      # (one wave: tick 0 of the twins)
    for _, sb in (a, b):
        sb.tick(max_iter=100, warm_dual=True)
    rows, trajs, snaps = _per_tick(a[1], T, **kw)
    out = b[1].rollout(T, want_traj=True, **kw)
    torch.cuda.synchronize()
    got = _snapshot(b[1])
    _assert_equal(snaps[-1], got, mode)
    assert out["ticks_run"].cpu().numpy().tolist() == [T] * 3
    hist = out["hist"].cpu().numpy()
    assert hist.shape == (T, 3, 52) and np.array_equal(hist, rows) and np.array_equal(out["traj_hist"].cpu().numpy(), trajs)
    assert (np.diff(hist[:, :, 43], axis=0) > 0).all() and (hist[:, :, 45] > 0).all()      # every stream moves, every tick iterates
    assert not np.array_equal(got["state"][0], got["state"][1]) and not np.array_equal(got["state"][1], got["state"][2])
    if held:
        assert (hist[:, :, 45] <= 5).all() and (hist[:, :, 46] == 1).any()
    else:
        assert (hist[:, :, 46] == 0).all()
    _close(a, b)


def test_rollout_on_the_gpu_equals_the_cpu_build_of_the_same_text():
    """(2, 2), T = 3 from the cold start, converged with the dual state: the device arrays against tests/emu's g++ build of csrc/bmpc_rollout_kernel.inl
    on the same inputs, 1e-11 (the tolerance of the log and update tests; device libm and contraction against the host's)."""
    import torch
    from tests.emu import emu, emu_rollout as er
    N, S, T = 2, 2, 3
    mpcs, recs = _small_streams(N, S)
    g = _batch(N, S, mpcs, recs)
    out = g[1].rollout(T, warm_dual=True, want_traj=True)
    torch.cuda.synchronize()
    got, hist, th = _snapshot(g[1]), out["hist"].cpu().numpy(), out["traj_hist"].cpu().numpy()
    assert out["ticks_run"].cpu().numpy().tolist() == [T] * 3
    worst = 0.0
    for b in range(3):
        _, rec, Tb, ss = er.small_stream(N, S, which=b)
        A = er.fresh_arrays(N, S, ss, rec)
        r = er.rollout(N, S, 0.1, Tb, A, T, warm_dual=True, opts=emu.opts_for(N, start_rollout=0))
        assert r["ticks_run"] == T
        pairs = [(got["state"][b], A["ss"]), (got["robot"][b], A["rb"]), (got["p"][b], A["p"]), (got["x0"][b], A["x0"]), (got["x"][b], A["x"]), (got["g"][b], A["g"]),
                 (got["traj"][b], A["traj"]), (hist[:, b], r["hist"]), (th[:, b], r["traj_hist"])]
        for i, (x, y) in enumerate(pairs):
            if i == 7:      # (kkt: the residual at the solution is round-off itself; iterations may differ by one where the test sits on the tolerance)
                x, y = np.delete(x, [45, 47], axis=1), np.delete(y, [45, 47], axis=1)
            worst = max(worst, float(np.abs(x - y).max()))
    print(f"largest deviation GPU - CPU build over state, robot, p, x0, x, g, traj, hist, traj_hist: {worst:.3e}")
    assert worst <= 1e-11
    _close(g)


def test_the_stride_serves_more_streams_than_resident_workgroups():
    """The arrays of a 3-stream batch tiled to B = grid + 2 rows, the entry point called on them with T = 2: every replica of stream i bit-equal to
    the 3-stream run."""
    import torch
    from boundmpc_amd.solver import _ptr
    N, S, T = 2, 2, 2
    mpcs, recs = _small_streams(N, S)
    small, big = _batch(N, S, mpcs, recs), _batch(N, S, mpcs, recs)
    want = small[1].rollout(T, warm_dual=True, want_traj=True)
    solver, sb = big
    B = solver.launch_info()["grid"] + 2
    idx = torch.arange(B, device=sb.path.device) % 3
    t = {k: getattr(sb, k)[idx].contiguous() for k in ARRAYS + ("path",)}
    hist = torch.empty((T, B, 52), dtype=torch.float64, device=sb.path.device)
    th = torch.empty((T, B, sb.tr_len), dtype=torch.float64, device=sb.path.device)
    run = torch.zeros((B,), dtype=torch.int32, device=sb.path.device)
    rc = solver._lib.bmpc_stream_rollout(solver._h, B, T, _ptr(t["path"]), sb.entries, _ptr(t["state"]), _ptr(t["robot"]), _ptr(t["p"]), _ptr(t["x0"]), _ptr(t["dual"]), 0,
                                         _ptr(t["x"]), _ptr(t["g"]), _ptr(t["iters"]), _ptr(t["status"]), _ptr(t["kkt"]), _ptr(t["traj"]), 1, 0.0, _ptr(hist), _ptr(th),
                                         _ptr(run), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert (run == T).all()
    for k in ARRAYS:
        assert torch.equal(t[k], getattr(small[1], k)[idx]), k
    assert torch.equal(hist, want["hist"][:, idx]) and torch.equal(th, want["traj_hist"][:, idx])
    _close(small, big)


def test_streams_that_lose_their_plan_stop():
    """(10, 4): tick 0 solved out, then two iterations a tick without the real-time rule, T = 13 > N + 1; beside the workload stream one that is lost on
    entry.  ticks_run is what the per-tick error counts imply, the rows behind the stop are NaN, status 3 / iters 0 / kkt 0 are written, and every
    array equals the per-tick twin's (which goes on skipping the streams)."""
    import torch
    from boundmpc_amd import stream as bstream
    N, S, T = 10, 4, 13
    mpcs, recs = _small_streams(N, S, n=2)
    a, b = _batch(N, S, mpcs, recs, one_wave=True), _batch(N, S, mpcs, recs, one_wave=True)
    for _, sb in (a, b):
        sb.tick(max_iter=100, warm_dual=True)
        sb.state[1, bstream.SS["ERRCNT"]] = float(N)
    rows, trajs, snaps = _per_tick(a[1], T, max_iter=2, warm_dual=True)
    out = b[1].rollout(T, max_iter=2, warm_dual=True, want_traj=True)
    torch.cuda.synchronize()
    got, hist, run = _snapshot(b[1]), out["hist"].cpu().numpy(), out["ticks_run"].cpu().numpy()
    ec = rows[:, 0, 44]
    implied = int(np.argmax(ec >= N)) + 1
    assert (ec >= N).any() and 1 <= implied < T and run.tolist() == [implied, 0]
    _assert_equal(snaps[-1], got, "lost plan")
    assert np.array_equal(hist, rows, equal_nan=True) and np.array_equal(out["traj_hist"].cpu().numpy(), trajs, equal_nan=True)
    assert np.isfinite(hist[:implied, 0]).all() and np.isnan(hist[implied:, 0]).all() and np.isnan(hist[:, 1]).all()
    assert got["status"].tolist() == [3, 3] and got["iters"].tolist() == [0, 0] and got["kkt"].tolist() == [0.0, 0.0]
    _close(a, b)


def test_streams_stop_at_their_goals():
    """(2, 2): goal_tol from the per-tick twin's own phi trace (stream 0 reaches it behind tick 1 of T = 4): ticks_run is every stream's first crossing,
    its arrays are the twin's behind that tick, the rows behind it NaN."""
    import torch
    from boundmpc_amd import stream as bstream
    N, S, T = 2, 2, 4
    mpcs, recs = _small_streams(N, S)
    a, b = _batch(N, S, mpcs, recs, one_wave=True), _batch(N, S, mpcs, recs)
    phi_max = a[1].state[:, bstream.SS["PHIMAX"]].cpu().numpy()
    rows, trajs, snaps = _per_tick(a[1], T, warm_dual=True)
    gap = phi_max[None, :] - rows[:, :, 43]
    goal_tol = float(gap[1, 0])
    crossed = gap <= goal_tol
    first = np.where(crossed.any(axis=0), crossed.argmax(axis=0) + 1, T)
    assert first[0] == 2 and (first >= 1).all()
    out = b[1].rollout(T, warm_dual=True, goal_tol=goal_tol, want_traj=True)
    torch.cuda.synchronize()
    got, hist, th = _snapshot(b[1]), out["hist"].cpu().numpy(), out["traj_hist"].cpu().numpy()
    assert out["ticks_run"].cpu().numpy().tolist() == first.tolist()
    for s in range(3):
        f = int(first[s])
        _assert_equal(snaps[f - 1], got, f"stream {s} stopped behind tick {f - 1}", rows=s)
        assert np.array_equal(hist[:f, s], rows[:f, s]) and np.array_equal(th[:f, s], trajs[:f, s]) and np.isnan(hist[f:, s]).all() and np.isnan(th[f:, s]).all()
    _close(a, b)


def test_goal_count_on_the_second_reference_experiment():
    """Experiment 2 of the reference, converged ticks, goal_tol = 0.01: ticks_run is the first crossing of a goal_tol = 0 rollout's phi history, and the
    stream stands within 0.01 of the end of its path."""
    import torch
    from boundmpc_amd import stream as bstream
    from tests.closed_loop import reference_experiment_streams
    mpcs, recs, _ = reference_experiment_streams()
    T = 90
    a, b = _batch(10, 4, mpcs[1:], recs[1:]), _batch(10, 4, mpcs[1:], recs[1:])
    phi_max = float(a[1].state[0, bstream.SS["PHIMAX"]])
    free = a[1].rollout(T, warm_dual=True)
    stop = b[1].rollout(T, warm_dual=True, goal_tol=0.01)
    torch.cuda.synchronize()
    gap = phi_max - free["hist"][:, 0, 43].cpu().numpy()
    assert free["ticks_run"].cpu().numpy().tolist() == [T] and (gap <= 0.01).any()
    first = int(np.argmax(gap <= 0.01)) + 1
    assert 1 < first < T and stop["ticks_run"].cpu().numpy().tolist() == [first]
    assert phi_max - float(b[1].state[0, bstream.SS["PHI"]]) <= 0.01
    assert torch.equal(stop["hist"][:first], free["hist"][:first]) and torch.isnan(stop["hist"][first:]).all()
    _close(a, b)


def test_a_graph_replay_behind_a_rollout_on_another_stream_is_ordered():
    """A tick-graph replay enqueued on a second stream directly behind a rollout of the same handle runs after it: the arrays equal those of the twin
    that synchronises between the two."""
    import torch
    N, S = 2, 2
    mpcs, recs = _small_streams(N, S)
    a, b = _batch(N, S, mpcs, recs), _batch(N, S, mpcs, recs)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _, sb in (a, b):
        sb.tick_graph(warm_dual=True, stream=s1)      # tick 0, and the graph is in place
    torch.cuda.synchronize()
    a[1].rollout(5, warm_dual=True, stream=s1); torch.cuda.synchronize(); a[1].tick_graph(warm_dual=True, stream=s2)
    b[1].rollout(5, warm_dual=True, stream=s1); b[1].tick_graph(warm_dual=True, stream=s2)
    torch.cuda.synchronize()
    _assert_equal(_snapshot(a[1]), _snapshot(b[1]), "rollout, then a replay on another stream")
    _close(a, b)


def test_argument_errors_launch_nothing_and_the_side_outputs():
    """BMPC_ERR_ARG: ticks < 1, simulate clear, a negative or non-finite goal_tol, a time budget on the handle, a missing tick array; the ValueError of
    tick() for a cap without the dual state.  Then: hist, traj_hist and ticks_run may be NULL, the latency buffer receives the sum of the solves."""
    import torch
    from boundmpc_amd import stream as bstream
    from boundmpc_amd._lib import BoundMPCHipError
    from boundmpc_amd.solver import _ptr
    N, S = 2, 2
    mpcs, recs = _small_streams(N, S)
    solver, sb = _batch(N, S, mpcs, recs)
    assert solver._lib.bmpc_stream_rollout_len() == bstream.rollout_len() == 52
    before = _snapshot(sb)
    for kw in (dict(ticks=0), dict(ticks=-3), dict(ticks=2, goal_tol=-1e-3), dict(ticks=2, goal_tol=float("nan")), dict(ticks=2, goal_tol=float("inf"))):
        with pytest.raises(BoundMPCHipError, match="invalid argument"):
            sb.rollout(warm_dual=True, **kw)
    solver.set_time_budget_us(500.0)
    with pytest.raises(BoundMPCHipError, match="invalid argument"):
        sb.rollout(2, warm_dual=True)
    solver.set_time_budget_us(0)
    with pytest.raises(ValueError, match="iteration cap needs the dual state"):
        sb.rollout(2, max_iter=5)
    args = [3, 2, _ptr(sb.path), sb.entries, _ptr(sb.state), _ptr(sb.robot), _ptr(sb.p), _ptr(sb.x0), _ptr(sb.dual), 0, _ptr(sb.x), _ptr(sb.g), _ptr(sb.iters), _ptr(sb.status),
            _ptr(sb.kkt), _ptr(sb.traj), 1, 0.0, None, None, None, None]
    assert solver._lib.bmpc_stream_rollout(solver._h, *args[:16], 0, *args[17:]) == 1      # simulate clear
    assert solver._lib.bmpc_stream_rollout(solver._h, *args[:16], 2, *args[17:]) == 1
    for i in (2, 4, 5, 6, 7, 10, 11, 13, 15):                                               # path, sstate, robot, p, x0, x, g, status, traj
        assert solver._lib.bmpc_stream_rollout(solver._h, *[None if j == i else v for j, v in enumerate(args)]) == 1, i
    assert solver._lib.bmpc_stream_rollout(None, *args) == 1
    torch.cuda.synchronize()
    _assert_equal(before, _snapshot(sb), "nothing was launched")
    lat = torch.zeros(3, dtype=torch.float64, device=sb.path.device)
    solver.set_latency_buffer(lat); solver.set_timing(1)
    assert solver._lib.bmpc_stream_rollout(solver._h, *args) == 0                            # without hist, traj_hist, ticks_run; dual state given
    torch.cuda.synchronize()
    ms = solver.last_kernel_ms()
    solver.set_latency_buffer(None); solver.set_timing(0)
    lat = lat.cpu().numpy()
    assert (lat > 0).all() and lat.max() <= 1e3 * ms + 1.0 and (sb.iters.cpu().numpy() > 0).all()
    _close((solver, sb))
