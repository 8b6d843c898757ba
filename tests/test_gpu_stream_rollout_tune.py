"""GPU: sweeps inside a rollout (bmpc_stream_rollout_tuned, StreamBatch.rollout(tune=..., want_tune_used=); the kernels of csrc/bmpc_rollout_tune.hip and
csrc/bmpc_team_rollout_tune.hip: csrc/bmpc_rollout_kernel.inl with TU) -- against the contract: stream b of a tuned rollout against the rollout WITHOUT a
table of the one-stream batch {b} on a handle of its own whose options and setters carry tune_used[b], bit for bit, on a converged and on a held launch,
on one wave per stream and on teams; the table of NaN and no table against rollout(legs=...); invalid rows; tune_used and tune_defaults against the
handle; the g++ build of the same text; the stride over more streams than resident workgroups; the refusals.  (2, 2), B = 4 streams of
tests/emu/emu_rollout.py, T = 6, the table of tests/emu/emu_rollout.py."""
import numpy as np
import pytest

from tests.rollout_contract import (ARRAYS, HELD, assert_equal as _assert_equal, batch as _batch, close as _close, raw_rollout, records as _records, small_streams as _small_streams,
                                    snapshot as _snapshot)

pytestmark = pytest.mark.gpu
N, S, T, B = 2, 2, 6, 4
NW = 4
HELD_KW = dict(max_iter=5, warm_dual=True, accept_capped=True)
CONV_KW = dict(max_iter=0, warm_dual=True, accept_capped=True)
ON = dict(want_traj=True, audit=True, want_tube=True, want_log=True, log_stages=N, track=True)
OUT = ("hist", "traj_hist", "tube_hist", "log_hist")      # [ticks][B][..]
PER = ("ticks_run", "audit", "track", "legs_done", "leg_fired", "leg_why", "replan_info")      # [B][..]


def _table():
    from tests.emu import emu_rollout as ee
    return ee.table()


def _queue(mpcs, recs, entries, K=2):
    kinds = [_records(mpcs, recs, entries), _records(mpcs, recs, entries, detour=0.05)]
    return np.ascontiguousarray(np.stack([kinds[k % 2] for k in range(K)], axis=1))


def _events():
    from tests.emu import emu_rollout as ee
    return dict(leg_tick=np.array([[1, 4], [2, 4], [1, 4], [2, 4]], dtype=np.int32), disturb=ee.disturbances(T, B, on=(1, 4)))


def _made(held=False, n=B):
    mpcs, recs = _small_streams(N, S, n=n)
    solver, sb = _batch(N, S, mpcs, recs, one_wave=True, held=held)
    return solver, sb, mpcs, recs


def _solver_of(row):
    """a handle whose options and setters carry the resolved row"""
    from boundmpc_amd import BatchedOCPSolver, _lib, stream as bstream
    u = bstream.unpack_tune(row)
    s = BatchedOCPSolver(N, S, 0.1, tol=u["tol"], max_iter=u["max_iter"], mu_init=u["mu_init"], slack_push=u["slack_push"], mu_warm=u["mu_warm"], stall_window=u["stall_window"],
                         bound_margin=u["bound_margin"], mu_min_fac=u["mu_min_fac"])
    _lib.check(s._lib.bmpc_set_barrier_hold(s._h, u["hold"]), "bmpc_set_barrier_hold")
    _lib.check(s._lib.bmpc_stream_set_level_rule(s._h, u["lvl_c"], u["lvl_lo"], u["lvl_hi"]), "bmpc_stream_set_level_rule")
    s.set_rt_feasibility_tol(u["rt_tol"]); s.set_rt_position_row_cap(u["rt_row_cap"])
    s.set_team_waves(1)
    return s


def _one_stream_batch(row, sb, mpcs, b, before, path):
    """the one-stream batch {b} on a handle of its own set up from `row`, its arrays those stream b of `sb` had (`before`, `path`)"""
    import torch
    from boundmpc_amd import stream as bstream
    solver = _solver_of(row)
    one = bstream.StreamBatch(solver, [mpcs[b]])
    for k in ARRAYS:
        getattr(one, k).copy_(torch.as_tensor(before[k][b:b + 1]))
    one.path.copy_(path[b:b + 1])
    return solver, one


def _assert_stream(out, b, got, one_out, one, what):
    """stream b of the batch result against the one-stream result: arrays, path, every output"""
    import torch
    w = _snapshot(one)
    for k in ARRAYS:
        assert np.array_equal(got[k][b], w[k][0], equal_nan=True), f"{what}, stream {b}: {k} differs"
    for k in OUT:
        if k in one_out:
            assert np.array_equal(out[k][:, b].cpu().numpy(), one_out[k][:, 0].cpu().numpy(), equal_nan=True), f"{what}, stream {b}: {k}"
    for k in PER:
        if k in one_out:
            assert np.array_equal(out[k][b].cpu().numpy(), one_out[k][0].cpu().numpy(), equal_nan=True), f"{what}, stream {b}: {k}"


def _contract(held, waves):
    import torch
    solver, sb, mpcs, recs = _made(held)
    kw = HELD_KW if held else CONV_KW
    sb.tick(max_iter=100, warm_dual=True)
    torch.cuda.synchronize()
    before, path = _snapshot(sb), sb.path.clone()
    Q, ev, tab = _queue(mpcs, recs, sb.entries), _events(), _table()
    out = sb.rollout(T, legs=Q, tune=tab, want_tune_used=True, waves=waves, **ev, **ON, **kw)
    torch.cuda.synchronize()
    got, used = _snapshot(sb), out["tune_used"].cpu().numpy()
    what = f"{'held' if held else 'converged'}, waves {waves}"
    assert out["tune_info"].tolist() == [0] * B and out["ticks_run"].tolist() == [T] * B and not np.isnan(used).any()
    assert np.array_equal(used[0], solver.tune_defaults(kw["max_iter"]))
    iters = out["hist"][:, :, 45].cpu().numpy()
    print(what, "iterations per tick and stream:", iters.T.tolist())
    for b in range(B):
        s1, one = _one_stream_batch(used[b], sb, mpcs, b, before, path)
        one_out = one.rollout(T, legs=Q[b:b + 1], leg_tick=ev["leg_tick"][b:b + 1], disturb=ev["disturb"][:, b:b + 1], waves=waves, warm_dual=True, accept_capped=True, **ON)
        torch.cuda.synchronize()
        _assert_stream(out, b, got, one_out, one, what)
        assert torch.equal(sb.path[b], one.path[0]) and torch.equal(sb.legs[b], one.legs[0]), f"{what}, stream {b}: path table / queue"
        _close((s1, one))
    # an ignored table cannot pass: rows 1 to 3 change the iterations or the iterate of their streams against the launch without a table
    s2, sb2, _, _ = _made(held)
    for k in ARRAYS:
        getattr(sb2, k).copy_(torch.as_tensor(before[k]))
    sb2.path.copy_(path)
    plain = sb2.rollout(T, legs=Q, waves=waves, **ev, **ON, **kw)
    torch.cuda.synchronize()
    p_it, px = plain["hist"][:, :, 45].cpu().numpy(), sb2.x.cpu().numpy()
    assert np.array_equal(iters[:, 0], p_it[:, 0]) and np.array_equal(got["x"][0], px[0])
    for b in (1, 2, 3):
        assert not np.array_equal(iters[:, b], p_it[:, b]) or not np.array_equal(got["x"][b], px[b]), f"{what}: row {b} changed nothing"
    assert (iters[:, 1] <= 3).all() and (iters[:, 2] == HELD["max_iter"]).all()
    _close((solver, sb), (s2, sb2))


# ---- 1. the contract ----
@pytest.mark.parametrize("mode", ["converged", "held"])
def test_a_tuned_rollout_equals_four_one_stream_rollouts_on_four_handles(mode):
    _contract(mode == "held", None)


@pytest.mark.parametrize("mode", ["converged", "held"])
def test_a_tuned_rollout_on_teams_equals_four_team_one_stream_rollouts(mode):
    _contract(mode == "held", NW)


# ---- 2. the table of NaN, no table ----
@pytest.mark.parametrize("waves", [None, NW])
def test_a_table_of_nan_and_no_table_are_the_queue_entry(waves):
    import torch
    made = [_made() for _ in range(3)]
    for _, sb, _, _ in made:
        sb.tick(max_iter=100, warm_dual=True)
    Q, ev = _queue(made[0][2], made[0][3], made[0][1].entries), _events()
    want = made[0][1].rollout(T, legs=Q, waves=waves, **ev, **ON, **CONV_KW)
    nan = made[1][1].rollout(T, legs=Q, tune=np.full((B, 16), np.nan), want_tune_used=True, waves=waves, **ev, **ON, **CONV_KW)
    rc, none = _every_output_on(made[2][0], made[2][1], T, Q, ev, None, waves=waves)
    torch.cuda.synchronize()
    assert rc == 0
    for r, sb, what in ((nan, made[1][1], "a table of NaN"), (none, made[2][1], "no table")):
        _assert_equal(_snapshot(made[0][1]), _snapshot(sb), what)
        assert torch.equal(made[0][1].path, sb.path)
        for k in OUT + PER:
            assert np.array_equal(want[k].cpu().numpy(), r[k].cpu().numpy(), equal_nan=True), f"{what}: {k}"
    assert torch.equal(made[0][1].legs, made[1][1].legs) and torch.equal(made[0][1].legs, none["replan"])
    assert nan["tune_info"].tolist() == [0] * B and np.array_equal(nan["tune_used"].cpu().numpy(), np.tile(made[1][0].tune_defaults(), (B, 1)))
    assert none["tune_info"].tolist() == [-7] * B and (none["tune_used"] == -7.0).all()      # (not looked at)
    _close(*[m[:2] for m in made])


def _every_output_on(solver, sb, ticks, Q, ev, tune, **kw):
    """bmpc_stream_rollout_tuned on the tensors of the batch with every output on, the log rows of all N stages, the real-time rule and leg_on = 0; tune:
    [B][16] array or None; kw: arguments of raw_rollout -> (rc, dict of what was passed)"""
    lt = ev.get("leg_tick")
    return raw_rollout(solver, sb, 5, outputs=True, **{**dict(ticks=ticks, flags=3, log_stages=N, replan=Q, leg_tick=lt, leg_on=None if lt is None else np.zeros_like(lt),
                                                              disturb=ev.get("disturb"), tune=tune), **kw})


# ---- 3. invalid rows ----
@pytest.mark.parametrize("waves", [None, NW])
def test_invalid_rows_do_not_run_and_their_neighbours_do(waves):
    import torch
    from boundmpc_amd.stream import TUNE, TUNE_CROSS
    a, b = _made(), _made()
    for _, sb, _, _ in (a, b):
        sb.tick(max_iter=100, warm_dual=True)
    Q, ev, tab = _queue(a[2], a[3], a[1].entries), _events(), _table()
    bad = tab.copy()
    bad[0, TUNE["STALL_WINDOW"]], bad[0, TUNE["TOL"]] = 15.0, 0.0
    bad[2] = np.nan; bad[2, TUNE["LVL_HI"]] = 0.1
    for k in ("x", "g", "kkt"):
        getattr(b[1], k)[[0, 2]] = 7.25
    b[1].iters[[0, 2]] = 77; b[1].status[[0, 2]] = 9
    torch.cuda.synchronize()
    before, path = _snapshot(b[1]), b[1].path.clone()
    good = a[1].rollout(T, legs=Q, tune=tab, waves=waves, **ev, **ON, **CONV_KW)
    r = b[1].rollout(T, legs=Q, tune=bad, want_tune_used=True, waves=waves, **ev, **ON, **CONV_KW)
    torch.cuda.synchronize()
    assert r["tune_info"].tolist() == [1 << TUNE["STALL_WINDOW"] | 1 << TUNE["TOL"], 0, 1 << TUNE_CROSS, 0] and r["ticks_run"].tolist() == [0, T, 0, T]
    used = r["tune_used"].cpu().numpy()
    assert used[0, TUNE["STALL_WINDOW"]] == 15.0 and used[0, TUNE["TOL"]] == 0.0 and used[2, TUNE["LVL_HI"]] == 0.1 and used[2, TUNE["LVL_LO"]] == 0.0
    got, ok = _snapshot(b[1]), _snapshot(a[1])
    _assert_equal(before, got, "invalid rows keep every bit", rows=[0, 2])
    _assert_equal(ok, got, "the neighbours", rows=[1, 3])
    assert torch.equal(b[1].path[[0, 2]], path[[0, 2]]) and torch.equal(b[1].path[[1, 3]], a[1].path[[1, 3]]) and torch.equal(b[1].legs[[1, 3]], a[1].legs[[1, 3]])
    assert np.array_equal(b[1].legs[[0, 2]].cpu().numpy(), Q[[0, 2]])      # (their records keep their flags)
    for k in OUT:
        assert torch.isnan(r[k][:, [0, 2]]).all() and np.array_equal(r[k][:, [1, 3]].cpu().numpy(), good[k][:, [1, 3]].cpu().numpy(), equal_nan=True), k
    for k in PER:
        assert np.array_equal(r[k][[1, 3]].cpu().numpy(), good[k][[1, 3]].cpu().numpy(), equal_nan=True), k
    assert r["legs_done"][[0, 2]].tolist() == [0, 0] and (r["leg_fired"][[0, 2]] == -1).all() and (r["replan_info"][[0, 2]] == -1).all() and (r["leg_why"][[0, 2]] == 0).all()
    # their audit and tracking records: those of a stream lost on entry
    lost = _made()
    lost[1].tick(max_iter=100, warm_dual=True)
    from boundmpc_amd.stream import SS
    lost[1].state[:, SS["ERRCNT"]] = N
    lo = lost[1].rollout(T, legs=Q, waves=waves, **ev, **ON, **CONV_KW)
    torch.cuda.synchronize()
    assert lo["ticks_run"].tolist() == [0] * B
    for k in ("audit", "track"):
        assert np.array_equal(r[k][[0, 2]].cpu().numpy(), lo[k][[0, 2]].cpu().numpy(), equal_nan=True), k
    _close(a[:2], b[:2], lost[:2])


# ---- 4. tune_used and tune_defaults against the handle ----
def test_tune_used_and_tune_defaults_are_the_handles_settings():
    import torch
    from boundmpc_amd import stream as bstream
    from boundmpc_amd._lib import BoundMPCHipError
    solver, sb, mpcs, recs = _made(held=True)
    d = solver.tune_defaults()
    want = bstream.tune_table(1, tol=HELD["tol"], max_iter=HELD["max_iter"], fixed_barrier=HELD["fixed_barrier"], bound_margin=HELD["bound_margin"], rt_tol=1e-2, rt_row_cap=1e-5,
                              slack_push=1e-2, stall_window=40)[0]
    want[14:] = 0.0
    assert np.array_equal(d, want), (d, want)      # (tune_table(fixed_barrier=...) sets what the constructor sets)
    assert solver.tune_defaults(7)[0] == 7.0 and np.array_equal(solver.tune_defaults(7)[1:], d[1:])
    assert bstream.unpack_tune(d)["hold"] == 1 and bstream.tune_check(d) == 0
    conv, sbc, _, _ = _made()
    dc = bstream.unpack_tune(conv.tune_defaults())
    assert (dc["max_iter"], dc["tol"], dc["mu_init"], dc["mu_warm"], dc["mu_min_fac"], dc["slack_push"], dc["bound_margin"], dc["hold"], dc["stall_window"]) == (500, 1e-8, 0.1, 1e-2, 0.1, 1e-2, 0.0, 0, 40)
    assert (dc["lvl_c"], dc["lvl_lo"], dc["lvl_hi"], dc["rt_tol"], dc["rt_row_cap"]) == (0.0, 0.0, 0.0, 1e-4, 0.0)
    # tune_used: the launch's values where the row has NaN -- the max_iter ARGUMENT among them --, the row's elsewhere
    sb.tick(max_iter=100, warm_dual=True)
    tab = _table()
    out = sb.rollout(2, tune=tab, want_tune_used=True, **HELD_KW)
    torch.cuda.synchronize()
    used = out["tune_used"].cpu().numpy()
    launch = solver.tune_defaults(HELD_KW["max_iter"])
    assert np.array_equal(used, np.where(np.isnan(tab), launch[None], tab)) and (used[:, 14:] == 0.0).all() and out["tune_info"].tolist() == [0] * B
    with pytest.raises(BoundMPCHipError, match="invalid argument"):
        solver.tune_defaults(-1)
    _close((solver, sb), (conv, sbc))


# ---- 5. the GPU against the CPU build of the same text ----
def test_a_sweep_on_the_gpu_equals_the_cpu_build_of_the_same_text():
    """From the cold start with the dual state, T = 6, the table of the tests and a two-record queue: the device arrays against tests/emu's g++ build of
    the kernel text -- the comparison of test_a_mission_on_the_gpu_equals_the_cpu_build_of_the_same_text: 1e-11 with its two exclusions (iterations, kkt)."""
    import torch
    from tests.emu import emu, emu_rollout as ee
    solver, sb, mpcs, recs = _made()
    _, A, Tab, _ = ee.small_batch(N, S, B)
    Q, ev, tab = _queue(mpcs, recs, sb.entries), _events(), _table()
    out = sb.rollout(T, warm_dual=True, accept_capped=True, want_traj=True, legs=Q, tune=tab, want_tune_used=True, **ev)
    torch.cuda.synchronize()
    got, hist, th = _snapshot(sb), out["hist"].cpu().numpy(), out["traj_hist"].cpu().numpy()
    R = Q.copy()
    r = ee.rollout(N, S, 0.1, Tab, A, T, entry=5, tune=tab, replan=R, leg_on=np.zeros((B, 2)), accept_capped=True, opts=emu.opts_for(N, start_rollout=0), **ev)
    for k in ("ticks_run", "legs_done", "leg_fired", "leg_why", "replan_info", "tune_info"):
        assert out[k].tolist() == r[k].tolist(), k
    assert np.array_equal(out["tune_used"].cpu().numpy(), r["tune_used"]) and r["ticks_run"].tolist() == [T] * B
    pairs = [(got["state"], A["ss"]), (got["robot"], A["rb"]), (got["p"], A["p"]), (got["x0"], A["x0"]), (got["x"], A["x"]), (got["g"], A["g"]), (got["traj"], A["traj"]),
             (np.delete(hist, [45, 47], axis=2), np.delete(r["hist"], [45, 47], axis=2)), (th, r["traj_hist"]), (sb.path.cpu().numpy(), Tab), (sb.legs.cpu().numpy(), R)]
    devs = [float(np.abs(x - y).max()) for x, y in pairs]
    print("largest deviation GPU - CPU build: state, robot, p, x0, x, g, traj, hist, traj_hist, path, queue:", " ".join(f"{d:.3e}" for d in devs))
    print("iterations GPU", hist[:, :, 45].T.tolist(), "CPU build", r["hist"][:, :, 45].T.tolist())
    assert max(devs) <= 1e-11
    _close((solver, sb))


# ---- 6. the stride ----
def test_the_stride_serves_sweeps_of_more_streams_than_resident_workgroups():
    """The arrays of the 4-stream batch tiled to B = grid + 2 rows, rows cycling through the table, T = 4: every replica of stream i bit-equal to the
    4-stream run, its table outputs included"""
    import torch
    Ts = 4
    small, big = _made(), _made()
    Q, tab = _queue(small[2], small[3], small[1].entries), _table()
    ev = dict(leg_tick=np.array([[0, 2], [1, 1], [-1, 3], [2, 3]], dtype=np.int32))
    want = small[1].rollout(Ts, warm_dual=True, accept_capped=True, legs=Q, tune=tab, want_tune_used=True, **ev)
    solver, sb = big[:2]
    dev = sb.path.device
    Bn = solver.launch_info()["grid"] + 2
    idx = torch.arange(Bn, device=dev) % B
    t = {k: getattr(sb, k)[idx].contiguous() for k in ARRAYS + ("path",)}
    i = idx.cpu().numpy()
    rc, r = _every_output_on(solver, sb, Ts, Q[i], dict(leg_tick=ev["leg_tick"][i]), tab[i], tensors=t, B=Bn)
    torch.cuda.synchronize()
    assert rc == 0
    assert (r["ticks_run"] == Ts).all() and (r["tune_info"] == 0).all()
    for k in ARRAYS + ("path",):
        assert torch.equal(t[k], getattr(small[1], k)[idx]), k
    assert torch.equal(r["replan"], small[1].legs[idx]) and torch.equal(r["hist"], want["hist"][:, idx]) and torch.equal(r["tune_used"], want["tune_used"][idx])
    assert torch.equal(r["leg_fired"], want["leg_fired"][idx]) and torch.equal(r["legs_done"], want["legs_done"][idx])
    _close(small[:2], big[:2])


# ---- 7. the refusals ----
def test_argument_errors_launch_nothing():
    """BMPC_ERR_ARG with a table: what the queue entry refuses; the errors of the Python layer"""
    import torch
    from boundmpc_amd._lib import BoundMPCHipError
    solver, sb, mpcs, recs = _made()
    Q, ev, tab = _queue(mpcs, recs, sb.entries), _events(), _table()
    torch.cuda.synchronize()
    before = _snapshot(sb)
    call = lambda ticks=2, queue=Q, ev=ev, **kw: _every_output_on(solver, sb, ticks, queue, ev, tab, **kw)[0]
    for kw in (dict(ev=dict(disturb=None)), dict(legs_done=None), dict(update_flags=8), dict(update_flags=4), dict(ticks=0), dict(flags=0), dict(flags=2), dict(goal_tol=-1.0), dict(goal_tol=float("nan")),
               dict(audit_tol=-1.0), dict(queue=None, ev={}, audit_tol=float("nan")), dict(log_stages=0), dict(log_stages=N + 1), dict(max_iter=-1), dict(handle=None)):
        assert call(**kw) == 1, kw
    with pytest.raises(ValueError, match="does not go with"):
        sb.rollout(2, warm_dual=True, tune=tab, replan=Q[:, 0], replan_tick=[1] * B)
    with pytest.raises(ValueError, match="tune must be"):
        sb.rollout(2, warm_dual=True, tune=tab[:3])
    with pytest.raises(ValueError, match="goes with tune"):
        sb.rollout(2, warm_dual=True, want_tune_used=True)
    with pytest.raises(BoundMPCHipError, match="invalid argument"):
        sb.rollout(0, warm_dual=True, tune=tab)
    torch.cuda.synchronize()
    _assert_equal(before, _snapshot(sb), "nothing was launched")
    _close((solver, sb))
