"""GPU: plants inside a rollout (bmpc_stream_rollout_plant, bmpc_stream_plant; StreamBatch.rollout(plant=, want_plant_rec=), StreamBatch.plant_step; the
kernels of csrc/bmpc_rollout_plant.hip and csrc/bmpc_team_rollout_plant.hip: csrc/bmpc_rollout_kernel.inl with PL) -- against the contract: the entry
against the loop {tick() on one wave per stream or on teams, plant_step(), tube(), log(), disturb(), update_device(splice=True) of the head records due} on
a twin, converged and held; no table, the table of NaN and the identity table against rollout(tune=); invalid rows; the g++ build of the same text; the
stride over more streams than resident workgroups; the refusals; a graph replay on another stream behind the launch.  (2, 2), B = 4 streams of
tests/emu/emu_rollout.py, T = 6, the tables of tests/test_stream_rollout_plant.py."""
import numpy as np
import pytest

from tests.rollout_contract import (ARRAYS, assert_equal as _assert_equal, batch as _batch, close as _close, contract_loop, cut, raw_rollout, records as _records,
                                    small_streams as _small_streams, snapshot as _snapshot)

pytestmark = pytest.mark.gpu
N, S, T, B = 2, 2, 6, 4
NW = 4
HELD_KW = dict(max_iter=5, warm_dual=True, accept_capped=True)
CONV_KW = dict(max_iter=0, warm_dual=True, accept_capped=True)
ON = dict(want_traj=True, audit=True, want_tube=True, want_log=True, log_stages=N, track=True)
OUT = ("hist", "traj_hist", "tube_hist", "log_hist")      # [ticks][B][..]
PER = ("ticks_run", "audit", "track", "legs_done", "leg_fired", "leg_why", "replan_info")      # [B][..]
NAN = float("nan")
# The entry against the loop: asserted at 1e-11 -- the stand-alone kernel bmpc_stream_plant is another translation unit than the rollout kernels, the
# project's figure and argument for the log -- and bit for bit on top, which is what the first run on an MI355X found on all four launch shapes.
LOOP_ATOL, LOOP_BIT_EQUAL = 1e-11, True


def _queue(mpcs, recs, entries, K=2):
    kinds = [_records(mpcs, recs, entries), _records(mpcs, recs, entries, detour=0.05)]
    return np.ascontiguousarray(np.stack([kinds[k % 2] for k in range(K)], axis=1))


def _events():
    from tests.emu import emu_rollout as ee
    return dict(leg_tick=np.array([[1, 4], [2, 4], [1, 4], [2, 4]], dtype=np.int32), disturb=ee.disturbances(T, B, on=(1, 4)))


def _made(held=False, team=False, n=B):
    mpcs, recs = _small_streams(N, S, n=n)
    solver, sb = _batch(N, S, mpcs, recs, one_wave=not team, held=held)
    if team:
        solver.set_team_waves(NW)
    return solver, sb, mpcs, recs


def _tables(peak):
    """the tables of tests/test_stream_rollout_plant.py from the |first planned jerk| trace [T][B] of the run without a plant"""
    from boundmpc_amd import stream as bstream
    from tests.test_stream_rollout_plant import _sat_between
    bias = np.zeros(7); bias[3] = 0.05
    lin = bstream.plant_table(B, gain=[[0.8] * 7, [NAN] * 7, [NAN] * 7, [NAN] * 7], bias=[[NAN] * 7, bias, [NAN] * 7, [NAN] * 7], lag=[NAN, NAN, 0.5, NAN],
                              delay=[NAN, NAN, NAN, 1.0])
    sat = bstream.plant_table(B, gain=[[NAN] * 7, [0.8] * 7, [NAN] * 7, [NAN] * 7], sat=[_sat_between(peak[:, 0]), 0.8 * _sat_between(peak[:, 1]), NAN, NAN],
                              lag=[NAN, NAN, 0.5, NAN], delay=[NAN, NAN, 1.0, NAN])
    return dict(lin=lin, sat=sat)


def _fixed_table():
    """a table that needs no trace: gain 0.8 / LAG 0.5 with DELAY 1 / a clip at 0.1 rad/s^3 / all NaN"""
    from boundmpc_amd import stream as bstream
    return bstream.plant_table(B, gain=[[0.8] * 7, [NAN] * 7, [NAN] * 7, [NAN] * 7], lag=[NAN, 0.5, NAN, NAN], delay=[NAN, 1.0, NAN, NAN], sat=[NAN, NAN, 0.1, NAN])


def _deviation(x, y):
    x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
    assert x.shape == y.shape and np.array_equal(np.isnan(x), np.isnan(y)), "shapes or NaN slots differ"
    with np.errstate(invalid="ignore"):
        d = np.abs(x - y)
    return float(np.nanmax(np.where(np.isinf(x) & (x == y), 0.0, d), initial=0.0))


def _contract(held, team):
    import torch
    kw = HELD_KW if held else CONV_KW
    what = f"{'held' if held else 'converged'}, {'teams' if team else 'one wave'}"
    waves = NW if team else None
    # the run without a plant: the trace the clip is placed in, and what an ignored table would leave
    solver0, sb0, mpcs, recs = _made(held, team)
    sb0.tick(max_iter=100, warm_dual=True)
    Q, ev = _queue(mpcs, recs, sb0.entries), _events()
    plain = sb0.rollout(T, legs=Q, waves=waves, **ev, **ON, **kw)
    torch.cuda.synchronize()
    p_hist = plain["hist"].cpu().numpy()
    assert plain["ticks_run"].tolist() == [T] * B
    _close((solver0, sb0))
    for which, tab in _tables(np.abs(p_hist[:, :, 36:43]).max(axis=2)).items():
        a, b = _made(held, team), _made(held, team)
        for _, sb, _, _ in (a, b):
            sb.tick(max_iter=100, warm_dual=True)
        loop = contract_loop(a[1], T, dist=ev["disturb"], want_tube=True, want_log=True, queue=Q, leg_tick=ev["leg_tick"], plant=tab, **kw)
        out = b[1].rollout(T, legs=Q, plant=tab, want_plant_rec=True, waves=waves, **ev, **ON, **kw)
        torch.cuda.synchronize()
        got, want = _snapshot(b[1]), _snapshot(a[1])
        assert out["plant_info"].tolist() == [0] * B and out["ticks_run"].tolist() == [T] * B == loop["ticks_run"].tolist()
        for k in ("legs_done", "leg_fired", "replan_info"):
            assert out[k].cpu().numpy().tolist() == loop[k].tolist(), f"{what}, {which}: {k}"
        pairs = {k: (got[k], want[k]) for k in ARRAYS if k not in ("iters", "status")}
        pairs.update({k: (out[k].cpu().numpy(), loop[k]) for k in ("hist", "traj_hist", "tube_hist")})
        pairs.update(log_hist=(out["log_hist"].cpu().numpy(), cut(loop["log_hist"], N, N)), path=(b[1].path.cpu().numpy(), a[1].path.cpu().numpy()),
                     queue=(b[1].legs.cpu().numpy(), loop["queue"]), plant_state=(b[1].plant_state.cpu().numpy(), loop["plant_state"]),
                     plant_rec=(out["plant_rec"].cpu().numpy(), loop["plant_rec"]))
        devs = {k: _deviation(x, y) for k, (x, y) in pairs.items()}
        bits = all(np.array_equal(x, y, equal_nan=True) for x, y in pairs.values())
        print(f"{what}, {which}: largest deviation entry - loop", " ".join(f"{k} {d:.2e}" for k, d in devs.items()), "| bit-equal:", bits)
        print("  plant_rec", out["plant_rec"].cpu().numpy()[:, :6].tolist())
        assert np.array_equal(got["iters"], want["iters"]) and np.array_equal(got["status"], want["status"])
        assert max(devs.values()) <= LOOP_ATOL, devs
        assert bits or not LOOP_BIT_EQUAL, f"{what}, {which}: within {LOOP_ATOL} of the loop but not bit-equal to it"
        # an ignored table cannot pass, nor a step on the wrong side of the rows: every non-identity row changes the history of its stream
        h = out["hist"].cpu().numpy()
        for s_ in range(B):
            assert np.array_equal(h[:, s_], p_hist[:, s_]) == bool(np.isnan(tab[s_]).all()), f"{what}, {which}: row {s_}"
        if which == "sat":
            rec = out["plant_rec"].cpu().numpy()
            assert (0 < rec[:2, 1]).all() and (rec[:2, 1] < rec[:2, 0]).all() and rec[3].tolist() == [T, 0, 0, 0, 0, 0, 0, 0]
        _close(a[:2], b[:2])


# ---- 1. the contract ----
@pytest.mark.parametrize("mode", ["converged", "held"])
def test_a_rollout_with_plants_equals_the_per_tick_loop(mode):
    _contract(mode == "held", False)


@pytest.mark.parametrize("mode", ["converged", "held"])
def test_a_rollout_with_plants_on_teams_equals_the_per_tick_loop_of_team_ticks(mode):
    _contract(mode == "held", True)


def _every_output_on(solver, sb, ticks, Q, ev, plant, state, **kw):
    """bmpc_stream_rollout_plant on the tensors of the batch with every output on, the log rows of all N stages, the real-time rule and leg_on = 0;
    plant: [B][20] array or None, state: a device tensor or None; kw: arguments of raw_rollout -> (rc, dict of what was passed)"""
    lt = ev.get("leg_tick")
    return raw_rollout(solver, sb, 6, outputs=True, **{**dict(ticks=ticks, flags=3, log_stages=N, replan=Q, leg_tick=lt, leg_on=None if lt is None else np.zeros_like(lt),
                                                              disturb=ev.get("disturb"), plant=plant, plant_state=state), **kw})


# ---- 2. no table, the table of NaN, the identity table ----
@pytest.mark.parametrize("waves", [None, NW])
def test_no_table_a_table_of_nan_and_the_identity_table_are_the_sweeps_entry(waves):
    import torch
    from boundmpc_amd import stream as bstream
    from tests.emu import emu_rollout as ee
    made = [_made() for _ in range(4)]
    for _, sb, _, _ in made:
        sb.tick(max_iter=100, warm_dual=True)
    Q, ev, tune = _queue(made[0][2], made[0][3], made[0][1].entries), _events(), ee.table()
    want = made[0][1].rollout(T, legs=Q, tune=tune, want_tune_used=True, waves=waves, **ev, **ON, **CONV_KW)
    nan = made[1][1].rollout(T, legs=Q, tune=tune, want_tune_used=True, plant=np.full((B, 20), NAN), want_plant_rec=True, waves=waves, **ev, **ON, **CONV_KW)
    ident = made[2][1].rollout(T, legs=Q, tune=tune, want_tune_used=True, plant=np.tile(bstream.plant_identity(), (B, 1)), want_plant_rec=True, waves=waves, **ev, **ON, **CONV_KW)
    rc, none = _every_output_on(made[3][0], made[3][1], T, Q, ev, None, None, tune=tune, waves=waves)
    torch.cuda.synchronize()
    assert rc == 0
    for r, sb, what in ((nan, made[1][1], "a table of NaN"), (ident, made[2][1], "the identity table"), (none, made[3][1], "no table")):
        _assert_equal(_snapshot(made[0][1]), _snapshot(sb), what)
        assert torch.equal(made[0][1].path, sb.path)
        for k in OUT + PER + ("tune_info", "tune_used"):
            assert np.array_equal(want[k].cpu().numpy(), r[k].cpu().numpy(), equal_nan=True), f"{what}: {k}"
    assert torch.equal(made[0][1].legs, made[1][1].legs) and torch.equal(made[0][1].legs, made[2][1].legs) and torch.equal(made[0][1].legs, none["replan"])
    for r, sb in ((nan, made[1][1]), (ident, made[2][1])):      # the state holds the commands: the jerk the last post stored
        assert r["plant_info"].tolist() == [0] * B and r["plant_rec"].tolist() == [[T, 0, 0, 0, 0, 0, 0, 0]] * B
        st, last = sb.plant_state.cpu().numpy(), r["hist"][T - 1].cpu().numpy()[:, 36:43]
        assert np.array_equal(st[:, :7], last) and np.array_equal(st[:, 7:14], last) and (st[:, 14:] == 0).all()
    assert none["plant_info"].tolist() == [-7] * B and (none["plant_rec"] == -7.0).all()      # (not looked at)
    _close(*[m[:2] for m in made])


# ---- 3. invalid rows ----
@pytest.mark.parametrize("waves", [None, NW])
def test_invalid_rows_do_not_run_and_their_neighbours_do(waves):
    import torch
    from boundmpc_amd.stream import PLANT, SS
    a, b, lost = _made(), _made(), _made()
    for _, sb, _, _ in (a, b, lost):
        sb.tick(max_iter=100, warm_dual=True)
    Q, ev, tab = _queue(a[2], a[3], a[1].entries), _events(), _fixed_table()
    bad = tab.copy()
    bad[0, PLANT["LAG"]], bad[0, PLANT["GAIN"] + 5] = 0.0, np.inf
    bad[3, PLANT["DELAY"]] = 0.5
    for k in ("x", "g", "kkt"):
        getattr(b[1], k)[[0, 3]] = 7.25
    b[1].iters[[0, 3]] = 77; b[1].status[[0, 3]] = 9
    torch.cuda.synchronize()
    before, path = _snapshot(b[1]), b[1].path.clone()
    good = a[1].rollout(T, legs=Q, plant=tab, want_plant_rec=True, waves=waves, **ev, **ON, **CONV_KW)
    r = b[1].rollout(T, legs=Q, plant=bad, want_plant_rec=True, waves=waves, **ev, **ON, **CONV_KW)
    torch.cuda.synchronize()
    assert r["plant_info"].tolist() == [1 << PLANT["LAG"] | 1 << PLANT["GAIN"] + 5, 0, 0, 1 << PLANT["DELAY"]] and r["ticks_run"].tolist() == [0, T, T, 0]
    got, ok = _snapshot(b[1]), _snapshot(a[1])
    _assert_equal(before, got, "invalid rows keep every bit", rows=[0, 3])
    _assert_equal(ok, got, "the neighbours", rows=[1, 2])
    assert torch.equal(b[1].path[[0, 3]], path[[0, 3]]) and torch.equal(b[1].path[[1, 2]], a[1].path[[1, 2]]) and torch.equal(b[1].legs[[1, 2]], a[1].legs[[1, 2]])
    assert np.array_equal(b[1].legs[[0, 3]].cpu().numpy(), Q[[0, 3]])      # (their records keep their flags)
    st, jerk0 = b[1].plant_state.cpu().numpy(), before["robot"][:, 36:43]
    assert np.array_equal(st[[0, 3], :7], jerk0[[0, 3]]) and np.array_equal(st[[0, 3], 7:14], jerk0[[0, 3]])      # (the state they started from: untouched)
    assert torch.equal(b[1].plant_state[[1, 2]], a[1].plant_state[[1, 2]])
    for k in OUT:
        assert torch.isnan(r[k][:, [0, 3]]).all() and np.array_equal(r[k][:, [1, 2]].cpu().numpy(), good[k][:, [1, 2]].cpu().numpy(), equal_nan=True), k
    for k in PER + ("plant_rec",):
        assert np.array_equal(r[k][[1, 2]].cpu().numpy(), good[k][[1, 2]].cpu().numpy(), equal_nan=True), k
    assert r["legs_done"][[0, 3]].tolist() == [0, 0] and (r["leg_fired"][[0, 3]] == -1).all() and (r["replan_info"][[0, 3]] == -1).all() and (r["leg_why"][[0, 3]] == 0).all()
    assert r["plant_rec"][[0, 3]].tolist() == [[0, 0, -np.inf, -1, -1, 0, 0, 0]] * 2
    # their audit and tracking records: those of a stream lost on entry
    lost[1].state[:, SS["ERRCNT"]] = N
    lo = lost[1].rollout(T, legs=Q, plant=tab, want_plant_rec=True, waves=waves, **ev, **ON, **CONV_KW)
    torch.cuda.synchronize()
    assert lo["ticks_run"].tolist() == [0] * B and lo["plant_rec"].tolist() == [[0, 0, -np.inf, -1, -1, 0, 0, 0]] * B
    for k in ("audit", "track"):
        assert np.array_equal(r[k][[0, 3]].cpu().numpy(), lo[k][[0, 3]].cpu().numpy(), equal_nan=True), k
    # the stand-alone step: the mask, and nothing touched
    rb = b[1].robot.clone()
    info = b[1].plant_step(bad, tick=9)
    torch.cuda.synchronize()
    assert info.tolist() == r["plant_info"].tolist() and torch.equal(b[1].robot[[0, 3]], rb[[0, 3]]) and not torch.equal(b[1].robot[[1, 2]], rb[[1, 2]])
    assert np.array_equal(b[1].plant_state.cpu().numpy()[[0, 3]], st[[0, 3]]) and b[1].plant_rec[[0, 3]].tolist() == [[0, 0, -np.inf, -1, -1, 0, 0, 0]] * 2
    _close(a[:2], b[:2], lost[:2])


# ---- 4. the GPU against the CPU build of the same text ----
def test_a_rollout_with_plants_on_the_gpu_equals_the_cpu_build_of_the_same_text():
    """From the cold start with the dual state, T = 6, a run whose ticks all converge, a two-record queue and disturbances: the device arrays against
    tests/emu's g++ build of the kernel text -- the comparison of the sweeps' and the missions' tests: 1e-11 with its two exclusions (iterations, kkt)."""
    import torch
    from boundmpc_amd import stream as bstream
    from tests.emu import emu, emu_rollout as ee
    solver, sb, mpcs, recs = _made()
    _, A, Tab, _ = ee.small_batch(N, S, B)
    Q, ev, tab = _queue(mpcs, recs, sb.entries), _events(), _fixed_table()
    out = sb.rollout(T, warm_dual=True, accept_capped=True, want_traj=True, legs=Q, plant=tab, want_plant_rec=True, **ev)
    torch.cuda.synchronize()
    got, hist, th = _snapshot(sb), out["hist"].cpu().numpy(), out["traj_hist"].cpu().numpy()
    R, st = Q.copy(), bstream.plant_state_of(A["rb"])
    r = ee.rollout(N, S, 0.1, Tab, A, T, entry=6, plant=tab, plant_state=st, replan=R, leg_on=np.zeros((B, 2)), accept_capped=True, opts=emu.opts_for(N, start_rollout=0), **ev)
    for k in ("ticks_run", "legs_done", "leg_fired", "leg_why", "replan_info", "plant_info"):
        assert out[k].tolist() == r[k].tolist(), k
    assert r["ticks_run"].tolist() == [T] * B and (hist[:, :, 46] == 0).all()
    rec = out["plant_rec"].cpu().numpy()
    assert np.array_equal(rec[:, [0, 1, 3, 4]], r["plant_rec"][:, [0, 1, 3, 4]])
    pairs = [(got["state"], A["ss"]), (got["robot"], A["rb"]), (got["p"], A["p"]), (got["x0"], A["x0"]), (got["x"], A["x"]), (got["g"], A["g"]), (got["traj"], A["traj"]),
             (np.delete(hist, [45, 47], axis=2), np.delete(r["hist"], [45, 47], axis=2)), (th, r["traj_hist"]), (sb.path.cpu().numpy(), Tab), (sb.legs.cpu().numpy(), R),
             (sb.plant_state.cpu().numpy(), st), (rec[:, 2], r["plant_rec"][:, 2]), (np.sqrt(rec[:, 5]), np.sqrt(r["plant_rec"][:, 5]))]
    # (SUMSQ_DU is in squared units and as large as 1e2 here: what compares with the arrays, which are in rad/s^3, is its root, the norm of u - c over the run)
    devs = [float(np.abs(x - y).max()) for x, y in pairs]
    print("largest deviation GPU - CPU build: state, robot, p, x0, x, g, traj, hist, traj_hist, path, queue, plant_state, MAX_DU, sqrt(SUMSQ_DU):", " ".join(f"{d:.3e}" for d in devs))
    assert max(devs) <= 1e-11
    _close((solver, sb))


# ---- 5. the stride ----
def test_the_stride_serves_more_streams_than_resident_workgroups():
    """The arrays of the 4-stream batch tiled to B = grid + 2 rows, the rows cycling through the table, T = 4: every replica of stream i bit-equal to the
    4-stream run, its plant state and record included"""
    import torch
    Ts = 4
    small, big = _made(), _made()
    Q, tab = _queue(small[2], small[3], small[1].entries), _fixed_table()
    ev = dict(leg_tick=np.array([[0, 2], [1, 1], [-1, 3], [2, 3]], dtype=np.int32))
    want = small[1].rollout(Ts, warm_dual=True, accept_capped=True, legs=Q, plant=tab, want_plant_rec=True, **ev)
    solver, sb = big[:2]
    dev = sb.path.device
    Bn = solver.launch_info()["grid"] + 2
    idx = torch.arange(Bn, device=dev) % B
    t = {k: getattr(sb, k)[idx].contiguous() for k in ARRAYS + ("path",)}
    state = torch.zeros((Bn, 16), dtype=torch.float64, device=dev)
    state[:, :7] = state[:, 7:14] = t["robot"][:, 36:43]
    i = idx.cpu().numpy()
    rc, r = _every_output_on(solver, sb, Ts, Q[i], dict(leg_tick=ev["leg_tick"][i]), tab[i], state, tensors=t, B=Bn)
    torch.cuda.synchronize()
    assert rc == 0
    assert (r["ticks_run"] == Ts).all() and (r["plant_info"] == 0).all()
    for k in ARRAYS + ("path",):
        assert torch.equal(t[k], getattr(small[1], k)[idx]), k
    assert torch.equal(r["replan"], small[1].legs[idx]) and torch.equal(r["hist"], want["hist"][:, idx]) and torch.equal(r["plant_rec"], want["plant_rec"][idx])
    assert torch.equal(state, small[1].plant_state[idx]) and torch.equal(r["leg_fired"], want["leg_fired"][idx]) and torch.equal(r["legs_done"], want["legs_done"][idx])
    _close(small[:2], big[:2])


# ---- 6. the refusals ----
def test_argument_errors_launch_nothing():
    """BMPC_ERR_ARG with a plant table: plant without plant_state, and what the sweeps entry refuses; the errors of the Python layer"""
    import torch
    from boundmpc_amd._lib import BoundMPCHipError
    from boundmpc_amd.solver import _ptr
    solver, sb, mpcs, recs = _made()
    Q, ev, tab = _queue(mpcs, recs, sb.entries), _events(), _fixed_table()
    state = torch.zeros((B, 16), dtype=torch.float64, device=sb.path.device)
    torch.cuda.synchronize()
    before = _snapshot(sb)
    call = lambda ticks=2, queue=Q, ev=ev, state=state, **kw: _every_output_on(solver, sb, ticks, queue, ev, tab, state, **kw)[0]
    for kw in (dict(state=None), dict(queue=None, ev={}, state=None), dict(ev=dict(disturb=None)), dict(legs_done=None), dict(update_flags=8), dict(update_flags=4), dict(ticks=0), dict(flags=0),
               dict(flags=2), dict(goal_tol=-1.0), dict(goal_tol=float("nan")), dict(audit_tol=-1.0), dict(queue=None, ev={}, audit_tol=float("nan")), dict(log_stages=0),
               dict(log_stages=N + 1), dict(max_iter=-1), dict(handle=None)):
        assert call(**kw) == 1, kw
    L, p = solver._lib, _ptr
    plant = torch.as_tensor(tab, device=sb.path.device)
    for args in ((None, B, p(sb.robot), p(sb.state), p(plant), p(state)), (solver._h, 0, p(sb.robot), p(sb.state), p(plant), p(state)), (solver._h, B, None, p(sb.state), p(plant), p(state)),
                 (solver._h, B, p(sb.robot), None, p(plant), p(state)), (solver._h, B, p(sb.robot), p(sb.state), None, p(state)), (solver._h, B, p(sb.robot), p(sb.state), p(plant), None)):
        assert L.bmpc_stream_plant(*args, None, None, 0, None) != 0
    with pytest.raises(ValueError, match="does not go with"):
        sb.rollout(2, warm_dual=True, plant=tab, replan=Q[:, 0], replan_tick=[1] * B)
    with pytest.raises(ValueError, match="plant must be"):
        sb.rollout(2, warm_dual=True, plant=tab[:3])
    with pytest.raises(ValueError, match="goes with plant"):
        sb.rollout(2, warm_dual=True, want_plant_rec=True)
    with pytest.raises(BoundMPCHipError, match="invalid argument"):
        sb.rollout(0, warm_dual=True, plant=tab)
    torch.cuda.synchronize()
    _assert_equal(before, _snapshot(sb), "nothing was launched")
    assert (state == 0).all()
    _close((solver, sb))


# ---- 7. ordering ----
def test_a_graph_replay_behind_a_rollout_with_plants_on_another_stream_is_ordered():
    """A replay of the tick's graph enqueued on a second stream directly behind a rollout with plants of the same handle runs after it: the arrays equal
    those of the twin that synchronises between the two."""
    import torch
    a, b = _made(), _made()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _, sb, _, _ in (a, b):
        sb.tick_graph(warm_dual=True, stream=s1)      # tick 0, and the graph is in place
    torch.cuda.synchronize()
    Q = _queue(a[2], a[3], a[1].entries, 2)
    kw = dict(warm_dual=True, legs=Q, leg_tick=[[1, 3]] * B, plant=_fixed_table(), stream=s1)
    a[1].rollout(5, **kw); torch.cuda.synchronize(); a[1].tick_graph(warm_dual=True, stream=s2)
    b[1].rollout(5, **kw); b[1].tick_graph(warm_dual=True, stream=s2)
    torch.cuda.synchronize()
    _assert_equal(_snapshot(a[1]), _snapshot(b[1]), "rollout with plants, then a tick replay on another stream")
    assert torch.equal(a[1].path, b[1].path) and torch.equal(a[1].legs, b[1].legs) and torch.equal(a[1].plant_state, b[1].plant_state)
    _close(a[:2], b[:2])
