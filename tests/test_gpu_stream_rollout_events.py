"""GPU: events inside a rollout (bmpc_stream_rollout_events, bmpc_stream_disturb and the splice of bmpc_stream_update; StreamBatch.rollout(replan=...,
disturb=...), .disturb, .update_device(splice=True)): without events the rollout's own bits; with events the bits of the per-tick loop {one-wave fused
tick, bmpc_stream_disturb, bmpc_stream_update(splice) of the records due} on a twin batch; the g++ build of the same kernel text; the stride over more
streams than resident workgroups; the splice alone against its numpy mirror; the argument errors.  (2, 2), B = 3 streams, T = 6 unless said otherwise."""
import numpy as np
import pytest

from tests.rollout_contract import ARRAYS, assert_equal as _assert_equal, batch as _batch, close as _close, contract_loop, records as _records, small_streams as _small_streams, snapshot as _snapshot

pytestmark = pytest.mark.gpu
N, S, T = 2, 2, 6
ATOL = 1e-11                     # tests/test_stream_rollout_events.py's bound of the splice (measured there: profiles/stream_splice.txt)


def _raw_events(solver, t, B, ticks, flags, goal_tol, hist, th, run, replan, tick_of, info, uflags, dist, entries, max_iter=0):
    """bmpc_stream_rollout_events on the tensors of `t` (ARRAYS + path); any of the outputs and events may be None"""
    from boundmpc_amd.solver import _ptr
    return solver._lib.bmpc_stream_rollout_events(solver._h, B, ticks, _ptr(t["path"]), entries, _ptr(t["state"]), _ptr(t["robot"]), _ptr(t["p"]), _ptr(t["x0"]), _ptr(t["dual"]),
                                                  max_iter, _ptr(t["x"]), _ptr(t["g"]), _ptr(t["iters"]), _ptr(t["status"]), _ptr(t["kkt"]), _ptr(t["traj"]), flags, goal_tol,
                                                  _ptr(hist), _ptr(th), _ptr(run), _ptr(replan), _ptr(tick_of), _ptr(info), uflags, _ptr(dist), None)


def _tensors(sb):
    return {k: getattr(sb, k) for k in ARRAYS + ("path",)}


def test_the_events_entry_without_events_equals_the_rollout():
    """every event pointer NULL, and a disturbance array of zeros: the bits of bmpc_stream_rollout on a twin"""
    import torch
    mpcs, recs = _small_streams(N, S)
    a, b, c = (_batch(N, S, mpcs, recs) for _ in range(3))
    want = a[1].rollout(T, warm_dual=True, want_traj=True)
    dev = b[1].path.device
    hist, th = torch.empty((T, 3, 52), dtype=torch.float64, device=dev), torch.empty((T, 3, b[1].tr_len), dtype=torch.float64, device=dev)
    run, info = torch.zeros(3, dtype=torch.int32, device=dev), torch.full((3,), 7, dtype=torch.int32, device=dev)
    assert _raw_events(b[0], _tensors(b[1]), 3, T, 1, 0.0, hist, th, run, None, None, info, 3, None, b[1].entries) == 0
    zero = c[1].rollout(T, warm_dual=True, want_traj=True, disturb=np.zeros((T, 3, 21)))
    torch.cuda.synchronize()
    _assert_equal(_snapshot(a[1]), _snapshot(b[1]), "no event pointer")
    _assert_equal(_snapshot(a[1]), _snapshot(c[1]), "zero disturbances")
    assert torch.equal(hist, want["hist"]) and torch.equal(th, want["traj_hist"]) and torch.equal(run, want["ticks_run"]) and info.tolist() == [-1] * 3
    assert torch.equal(zero["hist"], want["hist"]) and torch.equal(zero["traj_hist"], want["traj_hist"]) and zero["replan_info"].tolist() == [-1] * 3
    assert torch.equal(a[1].path, b[1].path) and torch.equal(a[1].path, c[1].path)
    _close(a, b, c)


@pytest.mark.parametrize("mode", ["converged", "held"])
def test_events_equal_the_per_tick_loop_bit_for_bit(mode):
    """Tick 0 solved out, then T = 6 with re-plans (splice) behind tick 2 of stream 0 and the last tick of stream 2, none for stream 1, disturbances on
    ticks 1 and 4: the rollout with events on one batch, the loop of one-wave ticks + bmpc_stream_disturb + bmpc_stream_update(splice) on its twin."""
    import torch
    from tests.emu import emu_rollout as ee
    mpcs, recs = _small_streams(N, S)
    held = mode == "held"
    kw = dict(max_iter=5, warm_dual=True, accept_capped=True) if held else dict(max_iter=0, warm_dual=True)
    a, b = _batch(N, S, mpcs, recs, one_wave=True, held=held), _batch(N, S, mpcs, recs, one_wave=True, held=held)
    for _, sb in (a, b):
        sb.tick(max_iter=100, warm_dual=True)
    records, tick_of, dist = _records(mpcs, recs, a[1].entries), np.array([2, -1, T - 1]), ee.disturbances(T, 3, on=(1, 4))
    loop = contract_loop(a[1], T, records, tick_of, dist, **kw)
    rows, trajs, run, info = loop["hist"], loop["traj_hist"], loop["ticks_run"], loop["replan_info"]
    out = b[1].rollout(T, want_traj=True, replan=records, replan_tick=tick_of, disturb=dist, **kw)
    torch.cuda.synchronize()
    _assert_equal(_snapshot(a[1]), _snapshot(b[1]), mode)
    assert torch.equal(a[1].path, b[1].path) and torch.equal(a[1].replan, b[1].replan)
    hist = out["hist"].cpu().numpy()
    assert np.array_equal(hist, rows, equal_nan=True) and np.array_equal(out["traj_hist"].cpu().numpy(), trajs, equal_nan=True)
    assert out["ticks_run"].tolist() == run.tolist() and out["replan_info"].tolist() == info.tolist()
    if not held:      # (the inputs are good: tests/test_stream_rollout_events.py)
        assert run.tolist() == [T] * 3 and info.tolist() == [0, -1, 0] and (hist[:, :, 46] == 0).all() and (hist[:, :, 50] == 1).all()
        assert b[1].replan[:, 0].tolist() == [0.0, 1.0, 0.0] and not torch.equal(b[1].path[0], torch.as_tensor(_snapshot_path(mpcs, b[1])[0], device=b[1].path.device))
    assert run[0] >= 3 and info[0] == 0 and info[1] == -1
    _close(a, b)


def _snapshot_path(mpcs, sb):
    from boundmpc_amd import stream as bstream
    return np.stack([bstream.path_table(m.ref_path, sb.entries)[0] for m in mpcs])


def test_events_on_the_gpu_equal_the_cpu_build_of_the_same_text():
    """From the cold start, converged with the dual state, the same events: the device arrays against tests/emu's g++ build of the kernel text, 1e-11
    with the two exclusions (iterations, kkt) of test_rollout_on_the_gpu_equals_the_cpu_build_of_the_same_text."""
    import torch
    from tests.emu import emu, emu_rollout as ee
    mpcs, recs = _small_streams(N, S)
    g = _batch(N, S, mpcs, recs)
    records, tick_of, dist = _records(mpcs, recs, g[1].entries), np.array([2, -1, T - 1]), ee.disturbances(T, 3, on=(1, 4))
    out = g[1].rollout(T, warm_dual=True, want_traj=True, replan=records, replan_tick=tick_of, disturb=dist)
    torch.cuda.synchronize()
    got, hist, th = _snapshot(g[1]), out["hist"].cpu().numpy(), out["traj_hist"].cpu().numpy()
    _, A, Tab, R = ee.small_batch(N, S)
    assert np.array_equal(R, records)
    r = ee.rollout(N, S, 0.1, Tab, A, T, entry=1, replan=R, replan_tick=tick_of, disturb=dist, opts=emu.opts_for(N, start_rollout=0))
    assert out["ticks_run"].tolist() == r["ticks_run"].tolist() == [T] * 3 and out["replan_info"].tolist() == r["replan_info"].tolist() == [0, -1, 0]
    pairs = [(got["state"], A["ss"]), (got["robot"], A["rb"]), (got["p"], A["p"]), (got["x0"], A["x0"]), (got["x"], A["x"]), (got["g"], A["g"]), (got["traj"], A["traj"]),
             (np.delete(hist, [45, 47], axis=2), np.delete(r["hist"], [45, 47], axis=2)), (th, r["traj_hist"]), (g[1].path.cpu().numpy(), Tab), (g[1].replan.cpu().numpy(), R)]
    devs = [float(np.abs(x - y).max()) for x, y in pairs]
    print("largest deviation GPU - CPU build: state, robot, p, x0, x, g, traj, hist, traj_hist, path, replan:", " ".join(f"{d:.3e}" for d in devs))
    assert max(devs) <= 1e-11
    _close(g)


def test_the_stride_serves_events_of_more_streams_than_resident_workgroups():
    """The arrays of the 3-stream batch tiled to B = grid + 2 rows, T = 2, a re-plan behind tick 0 and a disturbance on tick 0: every replica of
    stream i bit-equal to the 3-stream run."""
    import torch
    from tests.emu import emu_rollout as ee
    Ts = 2
    mpcs, recs = _small_streams(N, S)
    small, big = _batch(N, S, mpcs, recs), _batch(N, S, mpcs, recs)
    records, dist = _records(mpcs, recs, small[1].entries), ee.disturbances(Ts, 3, on=(0,))
    want = small[1].rollout(Ts, warm_dual=True, want_traj=True, replan=records, replan_tick=[0, 0, 0], disturb=dist)
    solver, sb = big
    dev = sb.path.device
    B = solver.launch_info()["grid"] + 2
    idx = torch.arange(B, device=dev) % 3
    t = {k: v[idx].contiguous() for k, v in _tensors(sb).items()}
    rep = torch.as_tensor(records, device=dev)[idx].contiguous()
    d = torch.as_tensor(dist, device=dev)[:, idx].contiguous()
    tick_of = torch.zeros(B, dtype=torch.int32, device=dev)
    hist, th = torch.empty((Ts, B, 52), dtype=torch.float64, device=dev), torch.empty((Ts, B, sb.tr_len), dtype=torch.float64, device=dev)
    run, info = torch.zeros(B, dtype=torch.int32, device=dev), torch.full((B,), 7, dtype=torch.int32, device=dev)
    assert _raw_events(solver, t, B, Ts, 1, 0.0, hist, th, run, rep, tick_of, info, 3, d, sb.entries) == 0
    torch.cuda.synchronize()
    assert (run == Ts).all() and (info == 0).all() and (rep[:, 0] == 0.0).all()
    for k in ARRAYS + ("path",):
        assert torch.equal(t[k], getattr(small[1], k)[idx]), k
    assert torch.equal(rep, small[1].replan[idx]) and torch.equal(hist, want["hist"][:, idx]) and torch.equal(th, want["traj_hist"][:, idx])
    assert not torch.equal(small[1].path, big[1].path)      # ... and the re-plan did write the tables
    _close(small, big)


def test_the_splice_of_update_device_equals_the_numpy_mirror():
    """Three ticks in, the plants in motion: update_device(splice=True, poor_bounds=True) leaves in the record buffer what stream.splice_record writes
    (1e-11), and the table and state apply_update gives on the mirror's numbers; a lowered flag is left alone.  Flags 0 / 1 (no splice) are what they
    were: the update text's CPU build on the same inputs (emu_stream_update.stream_update) is the checker, as in tests/test_gpu_stream_update.py."""
    import torch
    from boundmpc_amd import stream as bstream
    from tests.emu import emu_stream_update as eup
    from tests.emu.emu_rollout import args_of_record as _args_of_record
    RP, SS = bstream.RP, bstream.SS
    mpcs, recs = _small_streams(N, S)
    g = _batch(N, S, mpcs, recs)
    solver, sb = g
    sb.tick(max_iter=100, warm_dual=True); sb.tick(warm_dual=True); sb.tick(warm_dual=True)
    sb.disturb(np.random.default_rng(2).normal(size=(3, 21)) * 0.01)      # (accelerations and a velocity with a z component)
    torch.cuda.synchronize()
    records = _records(mpcs, recs, sb.entries)
    records[1, RP["FLAG"]] = 0.0
    rb0, st0, path0 = sb.robot.cpu().numpy().copy(), sb.state.cpu().numpy().copy(), sb.path.cpu().numpy().copy()
    assert np.abs(rb0[:, 7:21]).min(axis=1).max() > 0
    info = sb.update_device(records, splice=True, poor_bounds=True)
    torch.cuda.synchronize()
    rep, st, path, rb = sb.replan.cpu().numpy(), sb.state.cpu().numpy(), sb.path.cpu().numpy(), sb.robot.cpu().numpy()
    assert info.tolist() == [0, 0, 0] and (rep[:, 0] == 0.0).all()
    assert np.array_equal(rep[1], records[1]) and np.array_equal(st[1], st0[1]) and np.array_equal(path[1], path0[1]) and np.array_equal(rb[1], rb0[1])
    worst = 0.0
    for b in (0, 2):
        want = bstream.splice_record(records[b], rb0[b], 0.1, S, poor_bounds=True)
        worst = max(worst, float(np.abs(rep[b, 1:] - want[1:]).max()))
        ss_ref = st0[b].copy()
        T_ref, _ = bstream.apply_update(ss_ref, N, S, *_args_of_record(want, S), entries=sb.entries)
        eup.assert_close(path[b], st[b], T_ref, ss_ref, ATOL, f"stream {b}")
        assert rb[b, 33] == st[b, SS["PHIMAX"]]
    print(f"splice on the device - numpy mirror, record words: {worst:.3e}")
    assert worst <= ATOL
    # flags 0 and 1
    for set_goal in (False, True):
        rb1, st1, path1 = sb.robot.cpu().numpy().copy(), sb.state.cpu().numpy().copy(), sb.path.cpu().numpy().copy()
        recs2 = _records(mpcs, recs, sb.entries, tube=0.5)
        sb.update_device(recs2, set_goal=set_goal)
        torch.cuda.synchronize()
        assert np.array_equal(sb.replan.cpu().numpy()[:, 1:], recs2[:, 1:])      # nothing is spliced
        for b in range(3):
            i_cpu, _, Tc, ssc, rbc = eup.stream_update(N, S, recs2[b], path1[b], st1[b], rb1[b], set_goal=set_goal)
            eup.assert_close(sb.path.cpu().numpy()[b], sb.state.cpu().numpy()[b], Tc, ssc, 1e-11, f"flags {int(set_goal)}, stream {b}")
            np.testing.assert_allclose(sb.robot.cpu().numpy()[b], rbc, atol=1e-11, rtol=0)
    _close(g)


def test_argument_errors_launch_nothing_and_the_replan_info_values():
    """BMPC_ERR_ARG: a record buffer without its ticks, the update flags bmpc_stream_update refuses (on both entries), the rollout's own errors, the
    disturb entry's missing arrays.  replan_info: -1 for a tick outside the launch and for a stream that stops first, 1 for an invalid record."""
    import torch
    from boundmpc_amd import stream as bstream
    from boundmpc_amd._lib import BoundMPCHipError
    from boundmpc_amd.solver import _ptr
    mpcs, recs = _small_streams(N, S)
    solver, sb = _batch(N, S, mpcs, recs)
    dev = sb.path.device
    assert solver._lib.bmpc_stream_disturb_len() == bstream.DIST_LEN == 21
    records = _records(mpcs, recs, sb.entries)
    rep = sb._replan_buffer(records, None)
    tick_of = torch.tensor([1, 1, 1], dtype=torch.int32, device=dev)
    d = torch.zeros((2, 3, 21), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    before, t = _snapshot(sb), _tensors(sb)
    ev = lambda ticks=2, flags=1, goal=0.0, replan=rep, ticks_of=tick_of, uflags=3, dist=d: _raw_events(solver, t, 3, ticks, flags, goal, None, None, None, replan, ticks_of, None, uflags,
                                                                                                         dist, sb.entries)
    for kw in (dict(ticks_of=None), dict(uflags=8), dict(uflags=4), dict(uflags=5), dict(uflags=-1), dict(ticks=0), dict(flags=0), dict(goal=-1.0), dict(goal=float("nan"))):
        assert ev(**kw) == 1, kw
    assert _raw_events(type("NoHandle", (), {"_lib": solver._lib, "_h": None}), t, 3, 2, 1, 0.0, None, None, None, rep, tick_of, None, 3, d, sb.entries) == 1
    for flags in (8, 4, 5, 16):
        assert solver._lib.bmpc_stream_update(solver._h, 3, _ptr(rep), _ptr(sb.path), sb.entries, _ptr(sb.state), _ptr(sb.robot), None, flags, None) == 1, flags
    assert solver._lib.bmpc_stream_update(solver._h, 3, _ptr(rep), _ptr(sb.path), sb.entries, _ptr(sb.state), None, None, 3, None) == 1      # the splice needs the robot records
    for args in ((0, _ptr(sb.robot), _ptr(d)), (3, None, _ptr(d)), (3, _ptr(sb.robot), None)):
        assert solver._lib.bmpc_stream_disturb(solver._h, *args, None) == 1
    assert solver._lib.bmpc_stream_disturb(None, 3, _ptr(sb.robot), _ptr(d), None) == 1
    with pytest.raises(ValueError, match="go together"):
        sb.rollout(2, warm_dual=True, replan=records)
    with pytest.raises(ValueError, match="poor_bounds"):
        sb.update_device(records, poor_bounds=True)
    with pytest.raises(BoundMPCHipError, match="invalid argument"):
        sb.rollout(0, warm_dual=True, disturb=np.zeros((0, 3, 21)))
    torch.cuda.synchronize()
    _assert_equal(before, _snapshot(sb), "nothing was launched")
    assert np.array_equal(sb.replan.cpu().numpy(), records)
    # replan_info: stream 0 scheduled behind the launch's last tick + 1, stream 1 lost on entry, stream 2 an invalid record (n = 1)
    sb.tick(max_iter=100, warm_dual=True)
    sb.state[1, bstream.SS["ERRCNT"]] = float(N)
    records[2, bstream.RP["N"]] = 1.0
    path0 = sb.path.cpu().numpy().copy()
    out = sb.rollout(3, warm_dual=True, replan=records, replan_tick=[3, 0, 1])
    torch.cuda.synchronize()
    assert out["replan_info"].tolist() == [-1, -1, 1] and out["ticks_run"].tolist() == [3, 0, 3] and sb.replan[:, 0].tolist() == [1.0, 1.0, 0.0]
    assert np.array_equal(sb.path.cpu().numpy(), path0) and np.array_equal(sb.replan.cpu().numpy()[:, 1:], records[:, 1:])
    assert ev(uflags=2, replan=None, ticks_of=None, dist=None) == 0      # the splice bit without records: allowed and ignored
    torch.cuda.synchronize()
    _close((solver, sb))
