"""GPU: the rollout on TEAMS (bmpc_set_rollout_waves, StreamBatch.rollout(waves=); the kernels of csrc/bmpc_team_rollout.hip: csrc/bmpc_rollout_kernel.inl
with four cooperating waves per stream) -- against its exact checker, T direct launches of the fused TEAM tick on a twin batch (bit for bit: the tick
body is the team tick's); against the one-wave rollout as the team ticks agree with the one-wave ticks; over more streams than resident teams (the
stride); the fully-featured kernel against the loop {team tick, tube, log, disturb, update} on a twin; the stop rules; the setter; and the ordering
against a graph replay on another stream.  (10, 4) handles unless said otherwise, the 16 small streams of tests/emu/emu_rollout.py (workload streams
at rest in their start configurations).
The held-mode comparison against one wave relies on streams where the two programs agree: on the CPU builds of the one-wave and the team tick text
(tests/emu, held settings, tick 0 and 12 ticks) the 16 small streams differ by at most 7.3e-13 in the robot and trajectory records, every tick
accepted under the real-time rule -- five orders below the bounds used here."""
import numpy as np
import pytest

from tests.rollout_contract import ARRAYS, assert_equal as _assert_equal, assert_track, cut, push, batch as _batch, close as _close, contract_loop, per_tick as _per_tick, records as _records, small_streams as _small_streams, snapshot as _snapshot

pytestmark = pytest.mark.gpu
N, S = 10, 4
NW = 4
HELD_KW = dict(max_iter=5, warm_dual=True, accept_capped=True)
CONV_KW = dict(max_iter=0, warm_dual=True)


def _team_batch(mpcs, recs, held=False, n=N, s=S):
    """a batch whose ticks run on teams (the twin of a team rollout)"""
    solver, sb = _batch(n, s, mpcs, recs, held=held)
    solver.set_team_waves(NW)
    return solver, sb


@pytest.mark.parametrize("mode", ["converged", "held"])
def test_team_rollout_equals_team_ticks_bit_for_bit_and_one_wave_rollout_closely(mode):
    """B = 16, tick 0 solved out on teams, then 12 ticks: rollout(12, waves=4) on one batch, 12 tick(fused=True) calls on teams on its twin -- all eleven
    tick arrays and the history rows bit-equal.  held: also rollout(12, waves=1) on a third twin -- robot records within 1e-7, trajectory records within
    1e-6 (the figures of tests/test_gpu_team.py test_team_tick_equals_one_wave_tick_in_closed_loop)."""
    import torch
    T, B = 12, 16
    mpcs, recs = _small_streams(N, S, n=B)
    held = mode == "held"
    kw = HELD_KW if held else CONV_KW
    a, b = _team_batch(mpcs, recs, held), _team_batch(mpcs, recs, held)
    assert a[0].team_info(B)["waves"] == NW and b[0].rollout_waves == 1
    for _, sb in (a, b):
        sb.tick(max_iter=100, warm_dual=True)
    rows, trajs, snaps = _per_tick(a[1], T, fused=True, **kw)
    out = b[1].rollout(T, want_traj=True, waves=NW, **kw)
    torch.cuda.synchronize()
    got = _snapshot(b[1])
    _assert_equal(snaps[-1], got, f"{mode}: team rollout against team ticks")
    hist = out["hist"].cpu().numpy()
    assert out["ticks_run"].cpu().numpy().tolist() == [T] * B and hist.shape == (T, B, 52)
    assert np.array_equal(hist, rows) and np.array_equal(out["traj_hist"].cpu().numpy(), trajs)
    assert (np.diff(hist[:, :, 43], axis=0) > 0).all() and (hist[:, :, 45] > 0).all()      # every stream moves, every tick iterates
    assert b[0].rollout_waves == 1                                                         # the former setting is back
    if held:
        assert (hist[:, :, 45] <= 5).all() and (hist[:, :, 46] == 1).any()
        c = _team_batch(mpcs, recs, held)
        c[1].tick(max_iter=100, warm_dual=True)
        one = c[1].rollout(T, want_traj=True, waves=1, **kw)
        torch.cuda.synchronize()
        w = _snapshot(c[1])
        print(f"held, team rollout against one-wave rollout: robot {np.abs(got['robot'] - w['robot']).max():.3e}, traj {np.abs(got['traj'] - w['traj']).max():.3e}")
        assert np.array_equal(got["status"], w["status"]) and one["ticks_run"].cpu().numpy().tolist() == [T] * B
        np.testing.assert_allclose(got["robot"], w["robot"], atol=1e-7)
        np.testing.assert_allclose(got["traj"], w["traj"], atol=1e-6)
        _close(c)
    else:
        assert (hist[:, :, 46] == 0).all()
    _close(a, b)


def test_the_stride_serves_more_streams_than_resident_teams():
    """The arrays of the 16-stream batch tiled to B = resident teams + 2 rows, the entry point called on them with waves = 4 and T = 3: every replica
    bit-equal to its original, and the first 16 streams equal a B = 16 team rollout's."""
    import torch
    from boundmpc_amd.solver import _ptr
    T = 3
    mpcs, recs = _small_streams(N, S, n=16)
    small, big = _batch(N, S, mpcs, recs), _batch(N, S, mpcs, recs)
    want = small[1].rollout(T, warm_dual=True, want_traj=True, waves=NW)
    solver, sb = big
    B = solver.team_info(1)["resident_teams"] + 2
    assert B > 16 + 2
    idx = torch.arange(B, device=sb.path.device) % 16
    t = {k: getattr(sb, k)[idx].contiguous() for k in ARRAYS + ("path",)}
    hist = torch.empty((T, B, 52), dtype=torch.float64, device=sb.path.device)
    th = torch.empty((T, B, sb.tr_len), dtype=torch.float64, device=sb.path.device)
    run = torch.zeros((B,), dtype=torch.int32, device=sb.path.device)
    solver.set_rollout_waves(NW)
    rc = solver._lib.bmpc_stream_rollout(solver._h, B, T, _ptr(t["path"]), sb.entries, _ptr(t["state"]), _ptr(t["robot"]), _ptr(t["p"]), _ptr(t["x0"]), _ptr(t["dual"]), 0,
                                         _ptr(t["x"]), _ptr(t["g"]), _ptr(t["iters"]), _ptr(t["status"]), _ptr(t["kkt"]), _ptr(t["traj"]), 1, 0.0, _ptr(hist), _ptr(th),
                                         _ptr(run), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert (run == T).all()
    for k in ARRAYS:
        assert torch.equal(t[k], getattr(small[1], k)[idx]), k      # (rows 0..15 are the originals themselves)
    assert torch.equal(hist, want["hist"][:, idx]) and torch.equal(th, want["traj_hist"][:, idx])
    _close(small, big)


def test_the_full_kernel_equals_the_team_loop_and_the_plain_kernel():
    """B = 3, T = 6, a disturbance behind tick 2 of stream 1, a re-plan with splice behind tick 3 of stream 2, audit, tube rows, log rows of two stages
    and the tracking record, waves = 4: the arrays, hist, tube_hist and log_hist of the loop {team tick(), tube(), log(), disturb(),
    update_device(splice=True)} on a twin, bit for bit; audit and track against numpy over the GPU's own rows (integer slots exactly, the others
    within 1e-11); with no event raised the plain team rollout, bit for bit."""
    import torch
    from boundmpc_amd import stream as bstream
    from tests.emu import emu_stream_tube as et
    T, B, TOL = 6, 3, 1e-6
    tick_of = np.array([-1, -1, 3])
    d = push(T, B)
    mpcs, recs = _small_streams(N, S, n=B)
    a, b, c, e = (_team_batch(mpcs, recs) for _ in range(4))
    for _, sb in (a, b, c, e):
        sb.tick(max_iter=100, warm_dual=True)
    records = _records(mpcs, recs, a[1].entries)
    table0 = a[1].path.clone()
    loop = contract_loop(a[1], T, records, tick_of, d, want_tube=True, want_log=True, **CONV_KW)      # (the twin ticks on teams)
    rows, tubes, logs = loop["hist"], loop["tube_hist"], cut(loop["log_hist"], N, 2)
    full = b[1].rollout(T, replan=records, replan_tick=tick_of, disturb=d, audit=True, want_tube=True, audit_tol=TOL, want_log=True, log_stages=2, track=True, waves=NW, **CONV_KW)
    torch.cuda.synchronize()
    _assert_equal(_snapshot(a[1]), _snapshot(b[1]), "team loop against the full team rollout")
    assert torch.equal(a[1].path, b[1].path) and torch.equal(a[1].replan, b[1].replan) and not torch.equal(table0[2], b[1].path[2]) and torch.equal(table0[:2], b[1].path[:2])
    assert full["ticks_run"].tolist() == [T] * B and full["replan_info"].tolist() == [-1, -1, 0]
    hist, th, lh = full["hist"].cpu().numpy(), full["tube_hist"].cpu().numpy(), full["log_hist"].cpu().numpy()
    assert np.array_equal(hist, rows, equal_nan=True) and np.array_equal(th, tubes, equal_nan=True) and np.array_equal(lh, logs, equal_nan=True)
    np.testing.assert_allclose(full["audit"].cpu().numpy(), et.audit_of_batch(th, TOL), rtol=0.0, atol=1e-11)
    trk, want = full["track"].cpu().numpy(), bstream.track_of_rows(lh, hist)
    assert_track(trk, want, rtol=0.0, atol=1e-11)
    assert (full["audit"].cpu().numpy()[:, bstream.AUDIT["SAMPLES"]] == T).all() and (trk[[0, 2], bstream.TRACK["SAMPLES"]] == T).all()
    # no event raised: the fully-featured kernel (audit and log arrays given) leaves what the plain team rollout leaves
    plain = c[1].rollout(T, waves=NW, **CONV_KW)
    quiet = e[1].rollout(T, audit=True, want_log=True, log_stages=2, waves=NW, **CONV_KW)
    torch.cuda.synchronize()
    _assert_equal(_snapshot(c[1]), _snapshot(e[1]), "plain against the quiet full kernel")
    assert torch.equal(plain["hist"], quiet["hist"]) and torch.equal(plain["ticks_run"], quiet["ticks_run"]) and quiet["replan_info"].tolist() == [-1] * B
    _close(a, b, c, e)


def test_streams_that_lose_their_plan_stop():
    """tick 0 solved out, then two iterations a tick without the real-time rule, T = 13 > N + 1, beside the workload stream one that is lost on entry:
    status 3 written once, NaN rows behind the stop, ticks_run what the error counts imply, every array the team-tick twin's"""
    import torch
    from boundmpc_amd import stream as bstream
    T = 13
    mpcs, recs = _small_streams(N, S, n=2)
    a, b = _team_batch(mpcs, recs), _team_batch(mpcs, recs)
    for _, sb in (a, b):
        sb.tick(max_iter=100, warm_dual=True)
        sb.state[1, bstream.SS["ERRCNT"]] = float(N)
    rows, trajs, snaps = _per_tick(a[1], T, max_iter=2, warm_dual=True)
    out = b[1].rollout(T, max_iter=2, warm_dual=True, want_traj=True, waves=NW)
    torch.cuda.synchronize()
    got, hist, run = _snapshot(b[1]), out["hist"].cpu().numpy(), out["ticks_run"].cpu().numpy()
    ec = rows[:, 0, 44]
    implied = int(np.argmax(ec >= N)) + 1
    assert (ec >= N).any() and 1 <= implied < T and run.tolist() == [implied, 0]
    _assert_equal(snaps[-1], got, "lost plan")
    assert np.array_equal(hist, rows, equal_nan=True) and np.array_equal(out["traj_hist"].cpu().numpy(), trajs, equal_nan=True)
    assert np.isfinite(hist[:implied, 0]).all() and np.isnan(hist[implied:, 0]).all() and np.isnan(hist[:, 1]).all()
    assert (hist[:implied, 0, 46] != 3).all()                      # status 3 is the stop's, written once behind the last row
    assert got["status"].tolist() == [3, 3] and got["iters"].tolist() == [0, 0] and got["kkt"].tolist() == [0.0, 0.0]
    _close(a, b)


def test_goal_count_on_the_second_reference_experiment():
    """Experiment 2 of the reference, converged ticks, goal_tol = 0.01: the team rollout stops behind the tick the one-wave rollout stops behind, within
    0.01 of the end of the path, NaN rows behind it."""
    import torch
    from boundmpc_amd import stream as bstream
    from tests.closed_loop import reference_experiment_streams
    mpcs, recs, _ = reference_experiment_streams()
    T = 90
    a, b = _batch(10, 4, mpcs[1:], recs[1:]), _batch(10, 4, mpcs[1:], recs[1:])
    phi_max = float(a[1].state[0, bstream.SS["PHIMAX"]])
    one = a[1].rollout(T, warm_dual=True, goal_tol=0.01, waves=1)
    team = b[1].rollout(T, warm_dual=True, goal_tol=0.01, waves=NW)
    torch.cuda.synchronize()
    first = int(one["ticks_run"][0])
    assert 1 < first < T and team["ticks_run"].cpu().numpy().tolist() == [first]
    assert phi_max - float(b[1].state[0, bstream.SS["PHI"]]) <= 0.01
    assert torch.isfinite(team["hist"][:first]).all() and torch.isnan(team["hist"][first:]).all()
    _close(a, b)


def test_the_setter_and_the_waves_argument():
    """bmpc_set_rollout_waves: values other than 0, 1, 4 refused with the setting intact; 4 refused on a handle without team kernels (N = 16), 0 runs
    there and equals waves = 1 bit for bit; the untouched default equals waves = 1; waves= puts the former setting back, also behind a refusal."""
    import torch
    from boundmpc_amd._lib import BoundMPCHipError
    T = 3
    mpcs, recs = _small_streams(N, S, n=3)
    a, b = _batch(N, S, mpcs, recs), _batch(N, S, mpcs, recs)
    solver = a[0]
    assert solver.rollout_waves == 1 and solver._lib.bmpc_get_rollout_waves(None) == -1 and solver._lib.bmpc_set_rollout_waves(None, 1) == 1
    solver.set_rollout_waves(0)
    for bad in (2, 3, 5, 8, -1, 64):
        with pytest.raises(BoundMPCHipError, match="invalid argument"):
            solver.set_rollout_waves(bad)
        assert solver.rollout_waves == 0
        with pytest.raises(BoundMPCHipError, match="invalid argument"):
            a[1].rollout(T, warm_dual=True, waves=bad)
        assert solver.rollout_waves == 0
    solver.set_rollout_waves(NW); assert solver.rollout_waves == NW
    solver.set_rollout_waves(1)
    # the untouched default against waves = 1; waves= restores
    d = b[1].rollout(T, warm_dual=True, want_traj=True)
    solver.set_rollout_waves(0)
    o = a[1].rollout(T, warm_dual=True, want_traj=True, waves=1)
    assert solver.rollout_waves == 0
    torch.cuda.synchronize()
    _assert_equal(_snapshot(a[1]), _snapshot(b[1]), "default against waves = 1")
    assert torch.equal(d["hist"], o["hist"]) and torch.equal(d["traj_hist"], o["traj_hist"])
    _close(a, b)
    # a handle without team kernels
    m16, r16 = _small_streams(16, S, n=2)
    a, b = _batch(16, S, m16, r16), _batch(16, S, m16, r16)
    with pytest.raises(BoundMPCHipError, match="invalid argument"):
        a[0].set_rollout_waves(NW)
    with pytest.raises(BoundMPCHipError, match="invalid argument"):
        a[1].rollout(2, warm_dual=True, waves=NW)
    assert a[0].rollout_waves == 1
    auto = a[1].rollout(2, warm_dual=True, waves=0)
    one = b[1].rollout(2, warm_dual=True, waves=1)
    torch.cuda.synchronize()
    _assert_equal(_snapshot(a[1]), _snapshot(b[1]), "N = 16: automatic against one wave")
    assert torch.equal(auto["hist"], one["hist"]) and auto["ticks_run"].tolist() == [2, 2]
    _close(a, b)


def test_a_team_graph_replay_behind_a_team_rollout_on_another_stream_is_ordered():
    """A replay of the team tick's graph enqueued on a second stream directly behind a team rollout of the same handle runs after it: the arrays equal
    those of the twin that synchronises between the two."""
    import torch
    mpcs, recs = _small_streams(N, S, n=3)
    a, b = _team_batch(mpcs, recs), _team_batch(mpcs, recs)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _, sb in (a, b):
        sb.tick_graph(warm_dual=True, stream=s1)      # tick 0, and the graph is in place
    torch.cuda.synchronize()
    a[1].rollout(5, warm_dual=True, stream=s1, waves=NW); torch.cuda.synchronize(); a[1].tick_graph(warm_dual=True, stream=s2)
    b[1].rollout(5, warm_dual=True, stream=s1, waves=NW); b[1].tick_graph(warm_dual=True, stream=s2)
    torch.cuda.synchronize()
    _assert_equal(_snapshot(a[1]), _snapshot(b[1]), "team rollout, then a team tick replay on another stream")
    _close(a, b)
