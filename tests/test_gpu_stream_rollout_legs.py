"""GPU: missions inside a rollout (bmpc_stream_rollout_legs, StreamBatch.rollout(legs=..., leg_tick=, leg_on=, leg_tol=); the kernels of
csrc/bmpc_rollout_legs.hip and csrc/bmpc_team_rollout_legs.hip: csrc/bmpc_rollout_kernel.inl with QU) -- against the contract's loop on a twin batch
{fused tick, tube(), log(), disturb(), update_device(splice=True) for the streams whose head record is due; the host reads the three state words per
tick to evaluate the triggers}, bit for bit, converged and in held-barrier mode; legs = 1 against rollout(replan=, replan_tick=); the g++ build of the
same text; teams against the team-tick loop and against one wave; the stride over more streams than resident workgroups; the refusals; the ordering
against a graph replay on another stream.  (2, 2), B = 3 streams of tests/emu/emu_rollout.py, T <= 10."""
import numpy as np
import pytest

from tests.rollout_contract import (ARRAYS, assert_equal as _assert_equal, batch as _batch, close as _close, contract_loop, cut, raw_rollout, records as _records,
                                    small_streams as _small_streams, snapshot as _snapshot)

pytestmark = pytest.mark.gpu
N, S = 2, 2
NW = 4
HELD_KW = dict(max_iter=5, warm_dual=True, accept_capped=True)
CONV_KW = dict(max_iter=0, warm_dual=True)


def _queue(mpcs, recs, entries, K):
    """[B][K][len]: per stream a leg back, a leg back with a detour, a leg back, ..."""
    kinds = [_records(mpcs, recs, entries), _records(mpcs, recs, entries, detour=0.05)]
    return np.ascontiguousarray(np.stack([kinds[k % 2] for k in range(K)], axis=1))


def _mission(B, T):
    """K = 3 records per stream.  Record 0: the goal of the first leg, phi_max - c with c = 2e-4, 5e-4, 9e-4 of the streams' phi traces (1.2e-4, 3.1e-4, 6.4e-4,
    1.1e-3 behind ticks 1..4: the records fire behind ticks 2, 3 and 4).  Record 1: goal or tick 7, whichever first -- its tolerance is taken against the
    FIRST leg's phi_max, 2e-3 short, and the second leg's phi_max is up to 1e-3 shorter.  Record 2: at tick 8 (stream 0), an end-of-queue word (stream
    1), on a lost plan (stream 2: never)."""
    from boundmpc_amd.stream import LEG
    lt = np.array([[-1, 7, 8], [-1, 7, -1], [-1, 7, -1]], dtype=np.int32)[:B]
    lo = np.array([[LEG["AT_GOAL"], LEG["AT_GOAL"], 0], [LEG["AT_GOAL"], LEG["AT_GOAL"], 0], [LEG["AT_GOAL"], LEG["AT_GOAL"], LEG["ON_LOST"]]], dtype=np.int32)[:B]
    c = np.array([[2e-4, 2e-3, 0.0], [5e-4, 2e-3, 0.0], [9e-4, 2e-3, 0.0]])[:B]
    return lt, lo, c


def _assert_mission(out, loop, sb, what):
    for k in ("ticks_run", "legs_done", "leg_fired", "leg_why", "replan_info"):
        assert out[k].cpu().numpy().tolist() == loop[k].tolist(), f"{what}: {k} {out[k].tolist()}, the loop's {loop[k].tolist()}"
    assert np.array_equal(sb.legs.cpu().numpy(), loop["queue"], equal_nan=True), f"{what}: the queue buffer"


def _run_against_the_loop(a, b, T, held, waves=None):
    """tick 0 solved out on both twins; the mission of _mission with disturbances on ticks 1 and 4 as one launch on b, as the loop on a"""
    import torch
    from boundmpc_amd import stream as bstream
    from tests.emu import emu_rollout as ee
    kw = HELD_KW if held else CONV_KW
    for _, sb, _, _ in (a, b):
        sb.tick(max_iter=100, warm_dual=True)
    torch.cuda.synchronize()
    B = a[1].B
    Q = _queue(a[2], a[3], a[1].entries, 3)
    lt, lo, c = _mission(B, T)
    tol = a[1].state[:, bstream.SS["PHIMAX"]].cpu().numpy()[:, None] - c
    dist = ee.disturbances(T, B, on=(1, 4))
    loop = contract_loop(a[1], T, dist=dist, want_tube=True, want_log=True, queue=Q, leg_tick=lt, leg_on=lo, leg_tol=tol, **kw)
    out = b[1].rollout(T, want_traj=True, legs=Q, leg_tick=lt, leg_on=lo, leg_tol=tol, disturb=dist, audit=True, want_tube=True, want_log=True, log_stages=N, track=True,
                       waves=waves, **kw)
    torch.cuda.synchronize()
    what = f"{'held' if held else 'converged'}, waves {waves}"
    _assert_equal(_snapshot(a[1]), _snapshot(b[1]), what)
    assert torch.equal(a[1].path, b[1].path)
    _assert_mission(out, loop, b[1], what)
    for k in ("hist", "traj_hist", "tube_hist"):
        assert np.array_equal(out[k].cpu().numpy(), loop[k], equal_nan=True), f"{what}: {k}"
    assert np.array_equal(out["log_hist"].cpu().numpy(), cut(loop["log_hist"], N, N), equal_nan=True), f"{what}: log_hist"
    print(what, "fired", loop["leg_fired"].tolist(), "why", loop["leg_why"].tolist(), "ticks_run", loop["ticks_run"].tolist())
    return out, loop


def _twins(n, team=False, held=False, B=3):
    mpcs, recs = _small_streams(N, S, n=B)
    made = []
    for _ in range(n):
        solver, sb = _batch(N, S, mpcs, recs, one_wave=not team, held=held)
        if team:
            solver.set_team_waves(NW)
        made.append((solver, sb, mpcs, recs))
    return made


@pytest.mark.parametrize("mode", ["converged", "held"])
def test_a_mission_equals_the_per_tick_loop_bit_for_bit(mode):
    """T = 10: goal-triggered, goal-or-tick and tick-triggered records, an end-of-queue word and an on-lost record that never fires, disturbances on two
    ticks, every output on: one launch on one batch, the loop of one-wave ticks on its twin"""
    T, held = 10, mode == "held"
    a, b = _twins(2, held=held)
    out, loop = _run_against_the_loop(a, b, T, held)
    if not held:      # (the inputs are good, the construction holds: every stream flies its legs at its own ticks, the first two by their goals)
        from boundmpc_amd.stream import LEG
        assert loop["ticks_run"].tolist() == [T] * 3 and loop["legs_done"].tolist() == [3, 2, 2] and loop["leg_fired"][:, 0].tolist() == [2, 3, 4]
        assert (loop["leg_why"][:, 0] == LEG["WHY_GOAL"]).all() and (loop["leg_why"][:, 1] & LEG["WHY_GOAL"]).any() and loop["leg_why"][0, 2] == LEG["WHY_TICK"]
        assert (loop["replan_info"][loop["leg_fired"] >= 0] == 0).all() and (out["hist"].cpu().numpy()[:, :, 46] == 0).all()
    assert loop["legs_done"].min() >= 1 and len(set(loop["leg_fired"][:, 0].tolist())) >= 2
    _close(*[m[:2] for m in (a, b)])


def test_one_tick_triggered_record_equals_the_scheduled_replan():
    """legs = 1, leg_on = 0, leg_tick = replan_tick: every array, the record buffer and every output of rollout(replan=, replan_tick=) with everything on"""
    import torch
    from tests.emu import emu_rollout as ee
    T = 6
    a, b = _twins(2)
    for _, sb, _, _ in (a, b):
        sb.tick(max_iter=100, warm_dual=True)
    records, tick_of, dist = _records(a[2], a[3], a[1].entries), np.array([2, -1, T - 1]), ee.disturbances(T, 3, on=(1, 4))
    on = dict(want_traj=True, disturb=dist, audit=True, want_tube=True, want_log=True, log_stages=N, track=True, **CONV_KW)
    want = a[1].rollout(T, replan=records, replan_tick=tick_of, **on)
    got = b[1].rollout(T, legs=records[:, None], leg_tick=tick_of[:, None], **on)
    torch.cuda.synchronize()
    _assert_equal(_snapshot(a[1]), _snapshot(b[1]), "legs = 1")
    assert torch.equal(a[1].path, b[1].path) and torch.equal(a[1].replan, b[1].legs[:, 0])
    for k in ("hist", "traj_hist", "ticks_run", "tube_hist", "audit", "log_hist", "track"):
        assert torch.equal(want[k], got[k]) or np.array_equal(want[k].cpu().numpy(), got[k].cpu().numpy(), equal_nan=True), k
    assert want["replan_info"].tolist() == got["replan_info"][:, 0].tolist() == [0, -1, 0]
    assert got["legs_done"].tolist() == [1, 0, 1] and got["leg_fired"][:, 0].tolist() == [2, -1, T - 1] and got["leg_why"][:, 0].tolist() == [4, 0, 4]
    _close(a[:2], b[:2])


def test_a_mission_on_the_gpu_equals_the_cpu_build_of_the_same_text():
    """From the cold start, converged with the dual state, T = 8: a goal-triggered record per stream (its tolerance placed in the middle of a gap of the CPU
    build's phi trace), then a tick-triggered one: the device arrays against tests/emu's g++ build of the kernel text, 1e-11 with the two exclusions
    (iterations, kkt) of the siblings."""
    import torch
    from boundmpc_amd.stream import LEG
    from tests.emu import emu, emu_rollout as ee
    T = 8
    (solver, sb, mpcs, recs), = _twins(1)
    _, A, Tab, _ = ee.small_batch(N, S)
    Q = _queue(mpcs, recs, sb.entries, 2)
    o = emu.opts_for(N, start_rollout=0)
    at = [2, 3, 4]
    lt = np.array([[-1, 6]] * 3, dtype=np.int32)
    lo = np.array([[LEG["AT_GOAL"], 0]] * 3, dtype=np.int32)
    tol = np.zeros((3, 2))
    for b in range(3):
        tr = ee.contract_loop(N, S, 0.1, Tab[b].copy(), ee.unstack(A, b), T, opts=o)
        tol[b, 0] = tr["phi_max"][at[b]] - 0.5 * (tr["phi"][at[b] - 1] + tr["phi"][at[b]])
        assert tr["phi"][at[b]] - tr["phi"][at[b] - 1] > 1e-6      # (the gap is far above what separates the two builds)
    out = sb.rollout(T, warm_dual=True, want_traj=True, legs=Q, leg_tick=lt, leg_on=lo, leg_tol=tol)
    torch.cuda.synchronize()
    got, hist, th = _snapshot(sb), out["hist"].cpu().numpy(), out["traj_hist"].cpu().numpy()
    R = Q.copy()
    r = ee.rollout(N, S, 0.1, Tab, A, T, entry=4, replan=R, leg_tick=lt, leg_on=lo, leg_tol=tol, opts=o)
    for k in ("ticks_run", "legs_done", "leg_fired", "leg_why", "replan_info"):
        assert out[k].tolist() == r[k].tolist(), k
    assert r["leg_fired"].tolist() == [[2, 6], [3, 6], [4, 6]] and r["ticks_run"].tolist() == [T] * 3 and (r["hist"][:, :, 46] == 0).all()
    pairs = [(got["state"], A["ss"]), (got["robot"], A["rb"]), (got["p"], A["p"]), (got["x0"], A["x0"]), (got["x"], A["x"]), (got["g"], A["g"]), (got["traj"], A["traj"]),
             (np.delete(hist, [45, 47], axis=2), np.delete(r["hist"], [45, 47], axis=2)), (th, r["traj_hist"]), (sb.path.cpu().numpy(), Tab), (sb.legs.cpu().numpy(), R)]
    devs = [float(np.abs(x - y).max()) for x, y in pairs]
    print("largest deviation GPU - CPU build: state, robot, p, x0, x, g, traj, hist, traj_hist, path, queue:", " ".join(f"{d:.3e}" for d in devs))
    assert max(devs) <= 1e-11
    _close((solver, sb))


@pytest.mark.parametrize("mode", ["converged", "held"])
def test_a_mission_on_teams_equals_the_team_tick_loop_and_one_wave_closely(mode):
    """waves = 4: the same mission against the loop of TEAM ticks on a twin, bit for bit; held: against the one-wave launch on a third twin -- the same
    records on the same ticks, robot records within 1e-7, trajectory records within 1e-6 (the bounds of tests/test_gpu_stream_team_rollout.py)."""
    import torch
    T, held = 10, mode == "held"
    a, b = _twins(2, team=True, held=held)
    out, loop = _run_against_the_loop(a, b, T, held, waves=NW)
    assert b[0].rollout_waves == 1 and loop["legs_done"].min() >= 1
    if held:
        c, d = _twins(2, held=True)
        one, _ = _run_against_the_loop(c, d, T, True, waves=1)
        got, w = _snapshot(b[1]), _snapshot(d[1])
        print(f"held, team mission against one-wave mission: robot {np.abs(got['robot'] - w['robot']).max():.3e}, traj {np.abs(got['traj'] - w['traj']).max():.3e}")
        assert one["leg_fired"].tolist() == out["leg_fired"].tolist() and one["ticks_run"].tolist() == out["ticks_run"].tolist()
        np.testing.assert_allclose(got["robot"], w["robot"], atol=1e-7)
        np.testing.assert_allclose(got["traj"], w["traj"], atol=1e-6)
        _close(c[:2], d[:2])
    _close(a[:2], b[:2])


def _tensors(sb):
    return {k: getattr(sb, k) for k in ARRAYS + ("path",)}


def test_the_stride_serves_missions_of_more_streams_than_resident_workgroups():
    """The arrays of the 3-stream batch tiled to B = grid + 2 rows, T = 4, two records per stream at ticks (0, 2), (1, 1) and by an immediate goal: every
    replica of stream i bit-equal to the 3-stream run, its queue outputs included"""
    import torch
    Ts = 4
    small, big = _twins(2)
    Q = _queue(small[2], small[3], small[1].entries, 2)
    lt, lo, tol = np.array([[0, 2], [1, 1], [-1, 3]], dtype=np.int32), np.array([[0, 0], [0, 0], [1, 0]], dtype=np.int32), np.full((3, 2), 100.0)
    want = small[1].rollout(Ts, warm_dual=True, legs=Q, leg_tick=lt, leg_on=lo, leg_tol=tol)
    solver, sb = big[:2]
    dev = sb.path.device
    B = solver.launch_info()["grid"] + 2
    idx = torch.arange(B, device=dev) % 3
    t = {k: v[idx].contiguous() for k, v in _tensors(sb).items()}
    tile = lambda a, dt: torch.as_tensor(a, device=dev)[idx].to(dt).contiguous()
    q, tlt, tlo, ttol = tile(Q, torch.float64), tile(lt, torch.int32), tile(lo, torch.int32), tile(tol, torch.float64)
    hist, run = torch.empty((Ts, B, 52), dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    done = torch.full((B,), 7, dtype=torch.int32, device=dev)
    fired, why, info = (torch.full((B, 2), 7, dtype=torch.int32, device=dev) for _ in range(3))
    assert raw_rollout(solver, sb, 4, tensors=t, B=B, ticks=Ts, replan=q, leg_tick=tlt, leg_on=tlo, leg_tol=ttol, legs_done=done, leg_fired=fired, leg_why=why, replan_info=info,
                       hist=hist, ticks_run=run)[0] == 0
    torch.cuda.synchronize()
    assert want["leg_fired"].tolist() == [[0, 2], [1, 2], [0, 3]] and want["leg_why"].tolist() == [[4, 4], [4, 4], [1, 4]]
    assert (run == Ts).all() and (done == 2).all() and (info == 0).all() and (q[:, :, 0] == 0.0).all()
    for k in ARRAYS + ("path",):
        assert torch.equal(t[k], getattr(small[1], k)[idx]), k
    assert torch.equal(q, small[1].legs[idx]) and torch.equal(hist, want["hist"][:, idx])
    assert torch.equal(fired, want["leg_fired"][idx]) and torch.equal(why, want["leg_why"][idx])
    _close(small[:2], big[:2])


def test_argument_errors_launch_nothing():
    """BMPC_ERR_ARG: records without leg_tick, leg_on or legs_done, legs < 1 with records, and what the log entry refuses; the errors of the Python layer"""
    import torch
    from boundmpc_amd._lib import BoundMPCHipError
    (solver, sb, mpcs, recs), = _twins(1)
    dev = sb.path.device
    Q = _queue(mpcs, recs, sb.entries, 2)
    q = torch.as_tensor(Q, device=dev)
    lt, lo = torch.ones((3, 2), dtype=torch.int32, device=dev), torch.zeros((3, 2), dtype=torch.int32, device=dev)
    done = torch.full((3,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    before = _snapshot(sb)
    call = lambda **kw: raw_rollout(solver, sb, 4, **{**dict(replan=q, leg_tick=lt, leg_on=lo, legs_done=done), **kw})[0]
    for kw in (dict(leg_tick=None), dict(leg_on=None), dict(legs_done=None), dict(legs=0), dict(legs=-1), dict(update_flags=8), dict(update_flags=4), dict(ticks=0), dict(flags=0),
               dict(goal_tol=-1.0), dict(goal_tol=float("nan")), dict(audit_tol=-1.0), dict(replan=None, audit_tol=float("nan")), dict(handle=None)):
        assert call(**kw) == 1, kw
    with pytest.raises(ValueError, match="does not go with"):
        sb.rollout(2, warm_dual=True, legs=Q, replan=Q[:, 0], replan_tick=[1, 1, 1])
    with pytest.raises(ValueError, match="records of legs"):
        sb.rollout(2, warm_dual=True, leg_tick=[[1, 1]] * 3)
    with pytest.raises(ValueError, match="legs must be"):
        sb.rollout(2, warm_dual=True, legs=Q[:, 0])
    with pytest.raises(ValueError, match="leg_on must be"):
        sb.rollout(2, warm_dual=True, legs=Q, leg_on=[1, 1, 1])
    with pytest.raises(BoundMPCHipError, match="invalid argument"):
        sb.rollout(0, warm_dual=True, legs=Q, leg_tick=[[1, 1]] * 3)
    torch.cuda.synchronize()
    _assert_equal(before, _snapshot(sb), "nothing was launched")
    assert torch.equal(q, torch.as_tensor(Q, device=dev)) and done.tolist() == [7, 7, 7]
    # without records the queue arguments are not looked at: the call runs (as the log entry without a re-plan)
    assert call(replan=None, leg_tick=None, leg_on=None, legs_done=None, legs=-3) == 0
    torch.cuda.synchronize()
    _close((solver, sb))


def test_a_graph_replay_behind_a_mission_on_another_stream_is_ordered():
    """A replay of the tick's graph enqueued on a second stream directly behind a mission of the same handle runs after it: the arrays equal those of the
    twin that synchronises between the two."""
    import torch
    a, b = _twins(2)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _, sb, _, _ in (a, b):
        sb.tick_graph(warm_dual=True, stream=s1)      # tick 0, and the graph is in place
    torch.cuda.synchronize()
    Q = _queue(a[2], a[3], a[1].entries, 2)
    kw = dict(warm_dual=True, legs=Q, leg_tick=[[1, 3]] * 3, stream=s1)
    a[1].rollout(5, **kw); torch.cuda.synchronize(); a[1].tick_graph(warm_dual=True, stream=s2)
    b[1].rollout(5, **kw); b[1].tick_graph(warm_dual=True, stream=s2)
    torch.cuda.synchronize()
    _assert_equal(_snapshot(a[1]), _snapshot(b[1]), "mission, then a tick replay on another stream")
    assert torch.equal(a[1].path, b[1].path) and torch.equal(a[1].legs, b[1].legs)
    _close(a[:2], b[:2])
