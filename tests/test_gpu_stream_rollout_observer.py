"""GPU: observers inside a rollout (bmpc_stream_rollout_observer, bmpc_stream_observe; StreamBatch.rollout(observer=, want_sample=, want_observer_rec=),
StreamBatch.observe; the kernels of csrc/bmpc_rollout_observer.hip and csrc/bmpc_team_rollout_observer.hip: csrc/bmpc_rollout_body.inl with SE and OB) --
against the contract: the entry against the loop {observe(), tick() on one wave per stream or on teams, unsense(), plant_step(), tube(), log(), disturb(),
update_device(splice=True) of the head records due} on a twin, bit for bit, converged and held, on the rows of tests/test_stream_rollout_observer.py; an
N = 12 handle for the instantiations with the iterate in the workspace; no table (through the raw C entry), the table of NaN and the identity table against
rollout(sensor=); exact delay compensation, the filter and the gate with the assertions of the CPU tests; the g++ build of the same text at (2, 2); the stride
over more streams than resident workgroups; the refusals; a graph replay on another stream behind the launch.  (10, 4), B = 4 streams, T = 6."""
import numpy as np
import pytest

from tests.rollout_contract import (ARRAYS, RAW_GROUPS, RAW_HEAD, RAW_INT32, assert_equal as _assert_equal, close as _close, cut, history_rows, snapshot as _snapshot)
from tests.test_gpu_stream_rollout_sensor import CONV_KW, HELD_KW, NW, OUT, PER, SENSOR_GROUP, _deviation, _events, _made, _on, _plant, _queue

pytestmark = pytest.mark.gpu
N, S, T, B = 10, 4, 6, 4
NAN = float("nan")
OBSERVER_GROUP = ("observer", "observer_state", "observer_info", "observer_rec", "sample_hist")
FRESH_REC = [0, 0, -np.inf, -1, -1, -np.inf, -1, 0]
ROW_SETS = {"ident-gains-lead-gate": [0, 1, 2, 3], "nan-lead-gains-gate": [4, 2, 1, 3]}


def _rows(idx, ticks=T):
    """rows `idx` of the five (observer, sensor, noise) rows of tests/test_stream_rollout_observer.py"""
    from tests.test_stream_rollout_observer import _rows as rows
    ob, se, nz = rows(ticks)
    return np.ascontiguousarray(ob[idx]), np.ascontiguousarray(se[idx]), np.ascontiguousarray(nz[:, idx])


def _loop(sb, ticks, sensor, observer, noise=None, dist=None, queue=None, leg_tick=None, plant=None, **kw):
    """The contract's loop on the batch `sb`: the sensors' loop (tests/test_gpu_stream_rollout_sensor.py _loop) with observe() in the place of sense(); the sensors,
    the observers and the drives start where the launch starts them.  Every stream must keep its plan.
    -> the dict of that loop and sample_hist, observer_state, observer_rec"""
    import torch
    from boundmpc_amd import stream as bstream
    from tests.emu.emu_rollout import due as due_of
    SS, n = bstream.SS, sb.B
    r = dict(hist=np.full((ticks, n, 52), np.nan), traj_hist=np.full((ticks, n, sb.tr_len), np.nan), tube_hist=np.full((ticks, n, 16), np.nan),
             log_hist=np.full((ticks, n, bstream.log_len(sb.N)), np.nan), meas_hist=np.full((ticks, n, 43), np.nan), sample_hist=np.full((ticks, n, 21), np.nan),
             truth_hist=np.full((ticks, n, 43), np.nan), ticks_run=np.zeros(n, dtype=int))
    if queue is not None:
        K = queue.shape[1]
        r.update(queue=queue.copy(), legs_done=np.zeros(n, dtype=int), leg_fired=np.full((n, K), -1), replan_info=np.full((n, K), -1))
    sb.sensor_reset()
    sb.observer_reset()
    if plant is not None:
        sb.plant_reset()
    for t in range(ticks):
        assert (sb.state[:, SS["ERRCNT"]].cpu().numpy() < sb.N).all(), "a stream lost its plan"
        r["truth_hist"][t] = sb.robot.cpu().numpy()
        oinfo = sb.observe(sensor, observer, None if noise is None else noise[t], tick=t)
        sb.tick(simulate=True, **kw)
        sb.unsense(sensor)
        pinfo = sb.plant_step(plant, tick=t) if plant is not None else None
        tube, log = sb.tube(), sb.log()
        torch.cuda.synchronize()
        assert not oinfo.any() and not sb.sensor_info.any() and (pinfo is None or not pinfo.any())
        s = _snapshot(sb)
        r["hist"][t], r["traj_hist"][t], r["ticks_run"][:] = history_rows(s), s["traj"], t + 1
        r["tube_hist"][t], r["log_hist"][t], r["meas_hist"][t], r["sample_hist"][t] = tube.cpu().numpy(), log.cpu().numpy(), sb.meas.cpu().numpy(), sb.sample.cpu().numpy()
        if dist is not None:
            sb.disturb(dist[t])
        if queue is not None:
            head = np.minimum(r["legs_done"], K - 1)
            why = np.array([due_of(sb.N, s["state"][b], t, leg_tick[b, head[b]], 0, 0.0) if r["legs_done"][b] < K else 0 for b in range(n)])
            if why.any():
                recs = r["queue"][np.arange(n), head].copy()
                recs[why == 0, 0] = 0.0
                i = sb.update_device(recs, set_goal=True, splice=True)
                torch.cuda.synchronize()
                after = sb.replan.cpu().numpy()
                for b in np.nonzero(why)[0]:
                    r["queue"][b, head[b]] = after[b]
                    r["replan_info"][b, head[b]], r["leg_fired"][b, head[b]] = int(i[b]), t
                    r["legs_done"][b] += 1
    torch.cuda.synchronize()
    r["sensor_state"], r["sensor_rec"] = sb.sensor_state().cpu().numpy(), sb.sensor_rec.cpu().numpy()
    r["observer_state"], r["observer_rec"] = sb.observer_state().cpu().numpy(), sb.observer_rec.cpu().numpy()
    if plant is not None:
        r["plant_state"], r["plant_rec"] = sb.plant_state.cpu().numpy(), sb.plant_rec.cpu().numpy()
    return r


def _compare(what, out, loop, entry_sb, loop_sb, n_stages, plant=True, queue=True):
    """the entry's arrays against the loop's: -> (deviations by array, the arrays that are not bit-equal)"""
    got, want = _snapshot(entry_sb), _snapshot(loop_sb)
    pairs = {k: (got[k], want[k]) for k in ARRAYS}
    pairs.update({k: (out[k].cpu().numpy(), loop[k]) for k in ("hist", "traj_hist", "tube_hist", "meas_hist", "sample_hist")})
    pairs.update(log_hist=(out["log_hist"].cpu().numpy(), cut(loop["log_hist"], entry_sb.N, n_stages)), path=(entry_sb.path.cpu().numpy(), loop_sb.path.cpu().numpy()),
                 sensor_state=(entry_sb.sensor_state().cpu().numpy(), loop["sensor_state"]), sensor_rec=(out["sensor_rec"].cpu().numpy(), loop["sensor_rec"]),
                 observer_state=(entry_sb.observer_state().cpu().numpy(), loop["observer_state"]), observer_rec=(out["observer_rec"].cpu().numpy(), loop["observer_rec"]))
    if queue:
        pairs.update(queue=(entry_sb.legs.cpu().numpy(), loop["queue"]))
    if plant:
        pairs.update(plant_state=(entry_sb.plant_state.cpu().numpy(), loop["plant_state"]), plant_rec=(out["plant_rec"].cpu().numpy(), loop["plant_rec"]))
    devs = {k: _deviation(x, y) for k, (x, y) in pairs.items()}
    off = [k for k, (x, y) in pairs.items() if not np.array_equal(x, y, equal_nan=True)]
    print(f"{what}: largest deviation entry - loop", " ".join(f"{k} {d:.2e}" for k, d in devs.items()), "| not bit-equal:", off)
    return devs, off


# ---- 1. the contract ----
@pytest.mark.parametrize("rows", sorted(ROW_SETS))
@pytest.mark.parametrize("team", [False, True])
@pytest.mark.parametrize("mode", ["converged", "held"])
def test_a_rollout_with_observers_equals_the_per_tick_loop(mode, team, rows):
    """bit for bit: every tick array, history (meas_hist, sample_hist), the queue, the states and the records of plant, sensor and observer"""
    import torch
    from boundmpc_amd.stream import OBSERVER_REC
    held = mode == "held"
    kw, waves = HELD_KW if held else CONV_KW, NW if team else None
    what = f"{mode}, {'teams' if team else 'one wave'}, {rows}"
    (ob, se, nz), plant = _rows(ROW_SETS[rows]), _plant()
    a, b = _made(held, team), _made(held, team)
    for _, sb, _, _ in (a, b):
        sb.tick(max_iter=100, warm_dual=True)
    Q, ev = _queue(a[2], a[3], a[1].entries), _events()
    loop = _loop(a[1], T, se, ob, nz, dist=ev["disturb"], queue=Q, leg_tick=ev["leg_tick"], plant=plant, **kw)
    out = b[1].rollout(T, legs=Q, plant=plant, want_plant_rec=True, sensor=se, sensor_noise=nz, want_meas=True, want_sensor_rec=True, observer=ob, want_sample=True,
                       want_observer_rec=True, waves=waves, **ev, **_on(N), **kw)
    torch.cuda.synchronize()
    assert out["observer_info"].tolist() == [0] * B and out["sensor_info"].tolist() == [0] * B and out["plant_info"].tolist() == [0] * B
    assert out["ticks_run"].tolist() == [T] * B == loop["ticks_run"].tolist()
    for k in ("legs_done", "leg_fired", "replan_info"):
        assert out[k].cpu().numpy().tolist() == loop[k].tolist(), f"{what}: {k}"
    devs, off = _compare(what, out, loop, b[1], a[1], N)
    assert not off, (off, devs)
    rec = out["observer_rec"].cpu().numpy()
    assert (rec[:, OBSERVER_REC["SAMPLES"]] == T).all() and np.array_equal(b[1].robot.cpu().numpy(), out["hist"][T - 1].cpu().numpy()[:, :43])
    lead = ROW_SETS[rows].index(2)
    assert b[1].observer_state()[:, 36].tolist() == [float(i == lead) for i in range(B)]      # (LAGS: the LEAD row alone)
    _close(a[:2], b[:2])


def test_the_kernels_with_the_iterate_in_the_workspace():
    """one N = 12 handle, 2 streams, T = 3: the two instantiations without ZLDS, against the loop, bit for bit"""
    import torch
    from tests.emu import emu_rollout as ee
    n12, Ts = 12, 3
    ob, se, nz = _rows([1, 2], Ts)
    d = ee.disturbances(Ts, 2, on=(1,))
    a, b = _made(n=2, horizon=n12), _made(n=2, horizon=n12)
    for _, sb, _, _ in (a, b):
        sb.tick(max_iter=100, warm_dual=True)
    loop = _loop(a[1], Ts, se, ob, nz, dist=d, **CONV_KW)
    out = b[1].rollout(Ts, sensor=se, sensor_noise=nz, want_meas=True, want_sensor_rec=True, observer=ob, want_sample=True, want_observer_rec=True, disturb=d, **_on(n12), **CONV_KW)
    torch.cuda.synchronize()
    assert out["observer_info"].tolist() == [0, 0] and out["ticks_run"].tolist() == [Ts] * 2
    devs, off = _compare("N = 12", out, loop, b[1], a[1], n12, plant=False, queue=False)
    assert not off, (off, devs)
    assert (out["observer_rec"][:, 2] > 0).all()
    _close(a[:2], b[:2])


def _raw(solver, sb, tensors=None, waves=None, **over):
    """bmpc_stream_rollout_observer called directly with the batch's own tensors (or `tensors`: ARRAYS + path, of `B` streams) and every output array of the entry
    filled with -7: the sensors' _raw with the observer's group behind the sensor's.  -> (the return code, dict of what was passed by name)"""
    import torch
    from boundmpc_amd.solver import _ptr
    dev = sb.path.device
    names = RAW_HEAD + tuple(n for g in RAW_GROUPS for n in g if n != "replan_tick") + SENSOR_GROUP + OBSERVER_GROUP
    a = dict(handle=solver._h, B=sb.B, ticks=2, entries=sb.entries, max_iter=0, flags=3, goal_tol=0.0, update_flags=3, audit_tol=1e-6, log_stages=1, legs=1)
    a.update({k: getattr(sb, k) for k in ARRAYS + ("path",)} if tensors is None else tensors)
    for k, v in over.items():
        assert k in names, k
        a[k] = v if v is None or np.isscalar(v) or torch.is_tensor(v) else torch.as_tensor(np.ascontiguousarray(v), device=dev).to(torch.int32 if k in RAW_INT32 else torch.float64).contiguous()
    if a.get("replan") is not None and "legs" not in over:
        a["legs"] = a["replan"].shape[1]
    n, nb, K = a["ticks"], a["B"], (max(a["legs"], 1),)
    shapes = dict(hist=(n, nb, 52), traj_hist=(n, nb, sb.tr_len), ticks_run=(nb,), replan_info=(nb,) + K, tube_hist=(n, nb, 16), audit=(nb, 12), log_hist=(n, nb, 88 * a["log_stages"] + 4),
                  track=(nb, 12), legs_done=(nb,), leg_fired=(nb,) + K, leg_why=(nb,) + K, tune_info=(nb,), tune_used=(nb, 16), plant_info=(nb,), plant_rec=(nb, 8),
                  sensor_info=(nb,), sensor_rec=(nb, 8), meas_hist=(n, nb, 43), observer_info=(nb,), observer_rec=(nb, 8), sample_hist=(n, nb, 21))
    ints = ("ticks_run", "replan_info", "legs_done", "leg_fired", "leg_why", "tune_info", "plant_info", "sensor_info", "observer_info")
    for k, shape in shapes.items():
        if k not in over:
            a[k] = torch.full(shape, -7, dtype=torch.int32 if k in ints else torch.float64, device=dev)
    former = solver.rollout_waves
    if waves is not None:
        solver.set_rollout_waves(waves)
    rc = solver._lib.bmpc_stream_rollout_observer(*[_ptr(a.get(k)) if torch.is_tensor(a.get(k)) else a.get(k) for k in names], None)
    solver.set_rollout_waves(former)
    return rc, a


# ---- 2. P1: no table, the table of NaN, the identity table ----
@pytest.mark.parametrize("waves", [None, NW])
def test_no_table_a_table_of_nan_and_the_identity_table_are_the_sensors_entry(waves):
    """on the sensors' HOLD table with noise, a queue, disturbances and a plant table; no table through the raw C entry"""
    import torch
    from tests.emu import emu_rollout_sensor as es
    from tests.test_stream_rollout_sensor import _tables
    from tests.test_stream_rollout_observer import IDENT
    made = [_made() for _ in range(4)]
    for _, sb, _, _ in made:
        sb.tick(max_iter=100, warm_dual=True)
    Q, ev, plant, nz, tab = _queue(made[0][2], made[0][3], made[0][1].entries), _events(), _plant(), es.noise(T, B), _tables()["hold"]
    sen = dict(sensor=tab, sensor_noise=nz, want_meas=True, want_sensor_rec=True)
    want = made[0][1].rollout(T, legs=Q, plant=plant, want_plant_rec=True, waves=waves, **sen, **ev, **_on(N), **CONV_KW)
    obs = dict(want_sample=True, want_observer_rec=True)
    nan = made[1][1].rollout(T, legs=Q, plant=plant, want_plant_rec=True, observer=np.full((B, 8), NAN), waves=waves, **sen, **obs, **ev, **_on(N), **CONV_KW)
    ident = made[2][1].rollout(T, legs=Q, plant=plant, want_plant_rec=True, observer=np.tile(IDENT, (B, 1)), waves=waves, **sen, **obs, **ev, **_on(N), **CONV_KW)
    pst, sst = made[3][1].plant_reset(), made[3][1].sensor_reset()
    rc, none = _raw(made[3][0], made[3][1], waves=waves, ticks=T, log_stages=N, replan=Q, leg_tick=ev["leg_tick"], leg_on=np.zeros_like(ev["leg_tick"]), disturb=ev["disturb"],
                    plant=plant, plant_state=pst, sensor=tab, sensor_state=sst, sensor_noise=nz, observer=None, observer_state=None)
    torch.cuda.synchronize()
    assert rc == 0
    for r, sb, what in ((nan, made[1][1], "a table of NaN"), (ident, made[2][1], "the identity table"), (none, made[3][1], "no table")):
        _assert_equal(_snapshot(made[0][1]), _snapshot(sb), what)
        assert torch.equal(made[0][1].path, sb.path) and torch.equal(made[0][1].plant_state, sb.plant_state) and torch.equal(made[0][1].sensor_state(), sb.sensor_state())
        for k in OUT + PER + ("plant_info", "plant_rec", "sensor_info", "sensor_rec", "meas_hist"):
            assert np.array_equal(want[k].cpu().numpy(), r[k].cpu().numpy(), equal_nan=True), f"{what}: {k}"
    assert torch.equal(made[0][1].legs, made[1][1].legs) and torch.equal(made[0][1].legs, made[2][1].legs) and torch.equal(made[0][1].legs, none["replan"])
    for r, sb in ((nan, made[1][1]), (ident, made[2][1])):      # the estimates are the samples
        rec, srec = r["observer_rec"].cpu().numpy(), r["sensor_rec"].cpu().numpy()
        assert r["observer_info"].tolist() == [0] * B and np.array_equal(rec[:, 2:], srec[:, 1:7]) and rec[:, :2].tolist() == [[T, 0]] * B
        assert np.array_equal(r["sample_hist"].cpu().numpy(), r["meas_hist"].cpu().numpy()[:, :, :21])
        st = sb.observer_state().cpu().numpy()
        assert (st[:, 35] == 1).all() and (st[:, 36] == 0).all() and np.array_equal(st[:, :21], r["meas_hist"][T - 1].cpu().numpy()[:, :21])
    assert none["observer_info"].tolist() == [-7] * B and (none["observer_rec"] == -7.0).all() and (none["sample_hist"] == -7.0).all()      # (not looked at)
    _close(*[m[:2] for m in made])


# ---- 3. P2, P3 and the gate, with the assertions of the CPU tests ----
@pytest.mark.parametrize("waves", [None, NW])
def test_a_lead_row_compensates_the_hold_of_an_exact_sensor(waves):
    """P2 (tests/test_stream_rollout_observer.py, where the bound is derived): an exact sensor with HOLD, LEAD with gains (0.3, 0.5, 1), no noise, no disturbance,
    with and without a plant table: meas_hist[t] equals the plant the tick started from to 1e-12; HOLD without LEAD is off by more than 1e-6"""
    import torch
    from boundmpc_amd import stream as bstream
    sensor = bstream.sensor_table(B, hold=1.0)
    for plant in (None, _plant()):
        worst = {}
        for name, otab in (("lead", bstream.observer_table(B, lq=0.3, ldq=0.5, lddq=1.0, lead=1.0)), ("no lead", bstream.observer_table(B))):
            solver, sb, _, _ = _made()
            sb.tick(max_iter=100, warm_dual=True)
            torch.cuda.synchronize()
            rb0 = sb.robot.cpu().numpy()
            out = sb.rollout(T, sensor=sensor, want_meas=True, observer=otab, plant=plant, waves=waves, **CONV_KW)
            torch.cuda.synchronize()
            assert out["ticks_run"].tolist() == [T] * B and out["observer_info"].tolist() == [0] * B
            hist, meas = out["hist"].cpu().numpy(), out["meas_hist"].cpu().numpy()
            start = np.concatenate([rb0[None, :, :21], hist[:-1, :, :21]])
            worst[name] = float(np.abs(meas[:, :, :21] - start).max())
            _close((solver, sb))
        print(f"waves {waves}, plant {plant is not None}: |meas_hist - plant at the tick's start| with LEAD {worst['lead']:.3e}, with HOLD alone {worst['no lead']:.3e}")
        assert worst["no lead"] > 1e-6
        assert worst["lead"] <= 1e-12


@pytest.mark.parametrize("waves", [None, NW])
def test_a_gain_below_one_filters_the_noise_and_the_gate_rejects_the_outlier(waves):
    """P3: noise on q only (NQ = 1e-3), gains (0.3, 1, 1), the CPU test's draws, 12 ticks: observer_rec.SUMSQ_DQ < 0.5 sensor_rec.SUMSQ_DQ; with gain 1 the records
    agree word for word.  The gate: the outlier tick alone is counted, its sample_hist row carries the outlier, its meas_hist row the mirror's prior (to 1e-12: the
    mirror runs on the host)."""
    import torch
    from boundmpc_amd import stream as bstream
    from tests.emu import emu_rollout_sensor as es
    from tests.test_stream_rollout_observer import OUTLIER, P3_TICKS, _p3_draws
    sensor, nz = bstream.sensor_table(B, nq=1e-3), _p3_draws()
    for lq in (0.3, 1.0):
        solver, sb, _, _ = _made()
        sb.tick(max_iter=100, warm_dual=True)
        out = sb.rollout(P3_TICKS, sensor=sensor, sensor_noise=nz, want_sensor_rec=True, observer=bstream.observer_table(B, lq=lq, ldq=1.0, lddq=1.0), want_observer_rec=True,
                         waves=waves, **CONV_KW)
        torch.cuda.synchronize()
        rec, srec = out["observer_rec"].cpu().numpy(), out["sensor_rec"].cpu().numpy()
        assert out["ticks_run"].tolist() == [P3_TICKS] * B
        print(f"waves {waves}, LQ {lq}: SUMSQ_DQ observer / sensor", rec[:, 7] / srec[:, 6])
        if lq == 1.0:
            assert np.array_equal(rec[:, 2:], srec[:, 1:7]) and np.array_equal(rec[:, 0], srec[:, 0])
        else:
            assert (srec[:, 6] > 0).all() and (rec[:, 7] < 0.5 * srec[:, 6]).all()
        _close((solver, sb))
    ob, se, _ = _rows([3, 3, 3, 3])
    t0, j0, big = OUTLIER
    nz = es.noise(T, B); nz[t0, :, j0] = big
    solver, sb, _, _ = _made()
    sb.tick(max_iter=100, warm_dual=True)
    torch.cuda.synchronize()
    rb0 = sb.robot.cpu().numpy()
    out = sb.rollout(T, sensor=se, sensor_noise=nz, want_meas=True, want_sensor_rec=True, observer=ob, want_sample=True, want_observer_rec=True, waves=waves, **CONV_KW)
    torch.cuda.synchronize()
    rec, hist, meas, smp = (out[k].cpu().numpy() for k in ("observer_rec", "hist", "meas_hist", "sample_hist"))
    assert out["ticks_run"].tolist() == [T] * B and (rec[:, 1] == 1).all() and (rec[:, 0] == T).all()
    start = np.concatenate([rb0[None], hist[:-1, :, :43]])
    assert np.allclose(smp[t0, :, j0] - start[t0, :, j0], 0.1, atol=1e-12) and (np.abs(meas[t0, :, j0] - start[t0, :, j0]) < 1e-3).all()
    for b in range(B):
        st, ost = np.zeros(64), np.zeros(40)
        for t in range(T):
            rb, st, ost, m, _, _, _, _, rej = bstream.observe_robot(start[t, b], se[b], st, ob[b], ost, solver.dt, nz[t, b])
            assert rej == (t == t0), (b, t)
            np.testing.assert_allclose(meas[t, b, :21], rb[:21], rtol=0, atol=1e-12)
            np.testing.assert_allclose(smp[t, b], m, rtol=0, atol=1e-12)
    _close((solver, sb))


# ---- 4. the GPU against the CPU build of the same text ----
def test_a_rollout_with_observers_on_the_gpu_equals_the_cpu_build_of_the_same_text():
    """(2, 2), the shape of every comparison of the device with the g++ build in this suite (not (10, 4): the sensors' test records an unexplained 1.3e-7 there),
    from the cold start with the dual state, T = 6, disturbances: the device arrays against tests/emu's g++ build of the kernel text at 1e-11 with its two
    exclusions (iterations, kkt) -- the tolerance of tests/test_gpu_stream_rollout_sensor.py for the same comparison: the observer adds linear arithmetic only."""
    import torch
    from tests.emu import emu, emu_rollout as ee, emu_rollout_observer as eo
    n2, s2 = 2, 2
    solver, sb, mpcs, recs = _made(horizon=n2, segs=s2)
    _, A, Tab, _ = ee.small_batch(n2, s2, B)
    ob, se, nz = _rows([0, 1, 2, 3])
    d = ee.disturbances(T, B, on=(1, 4))
    out = sb.rollout(T, warm_dual=True, accept_capped=True, want_traj=True, disturb=d, sensor=se, sensor_noise=nz, want_meas=True, want_sensor_rec=True, observer=ob, want_sample=True,
                     want_observer_rec=True)
    torch.cuda.synchronize()
    got, hist, th = _snapshot(sb), out["hist"].cpu().numpy(), out["traj_hist"].cpu().numpy()
    st, ost = np.zeros((B, 64)), np.zeros((B, 40))
    r = eo.rollout(n2, s2, 0.1, Tab, A, T, sensor=se, sensor_state=st, sensor_noise=nz, observer=ob, observer_state=ost, disturb=d, accept_capped=True, opts=emu.opts_for(n2, start_rollout=0))
    assert r["ran"] == eo.RAN_OBSERVER and out["ticks_run"].tolist() == r["ticks_run"].tolist() == [T] * B and out["observer_info"].tolist() == r["observer_info"].tolist() == [0] * B
    rec, srec = out["observer_rec"].cpu().numpy(), out["sensor_rec"].cpu().numpy()
    assert np.array_equal(rec[:, [0, 1, 3, 4, 6]], r["observer_rec"][:, [0, 1, 3, 4, 6]]) and np.array_equal(srec[:, [0, 2, 3, 5]], r["sensor_rec"][:, [0, 2, 3, 5]])
    pairs = [(got["state"], A["ss"]), (got["robot"], A["rb"]), (got["p"], A["p"]), (got["x0"], A["x0"]), (got["x"], A["x"]), (got["g"], A["g"]), (got["traj"], A["traj"]),
             (np.delete(hist, [45, 47], axis=2), np.delete(r["hist"], [45, 47], axis=2)), (th, r["traj_hist"]), (sb.path.cpu().numpy(), Tab),
             (out["meas_hist"].cpu().numpy(), r["meas_hist"]), (out["sample_hist"].cpu().numpy(), r["sample_hist"]), (sb.sensor_state().cpu().numpy(), st),
             (sb.observer_state().cpu().numpy(), ost), (rec[:, [2, 5]], r["observer_rec"][:, [2, 5]]), (np.sqrt(rec[:, 7]), np.sqrt(r["observer_rec"][:, 7])),
             (srec[:, [1, 4]], r["sensor_rec"][:, [1, 4]]), (np.sqrt(srec[:, 6]), np.sqrt(r["sensor_rec"][:, 6]))]
    devs = [float(np.abs(x - y).max()) for x, y in pairs]
    print("largest deviation GPU - CPU build: state, robot, p, x0, x, g, traj, hist, traj_hist, path, meas_hist, sample_hist, sensor_state, observer_state, observer MAX_DQ / MAX_DP, "
          "sqrt(SUMSQ_DQ), sensor MAX_DQ / MAX_DP, sqrt(SUMSQ_DQ):", " ".join(f"{v:.3e}" for v in devs))
    assert max(devs) <= 1e-11
    _close((solver, sb))


# ---- 5. the stride ----
def test_the_stride_serves_more_streams_than_resident_workgroups():
    """The arrays of the 4-stream batch tiled to B = grid + 2 rows, the rows cycling through the tables, 2 ticks: every replica of stream i bit-equal to the
    4-stream run, its states, records, meas_hist and sample_hist rows included"""
    import torch
    Ts = 2
    small, big = _made(), _made()
    ob, se, nz = _rows([0, 1, 2, 3], Ts)
    want = small[1].rollout(Ts, warm_dual=True, accept_capped=True, sensor=se, sensor_noise=nz, want_meas=True, want_sensor_rec=True, observer=ob, want_sample=True, want_observer_rec=True)
    solver, sb = big[:2]
    dev = sb.path.device
    Bn = solver.launch_info()["grid"] + 2
    idx = torch.arange(Bn, device=dev) % B
    t = {k: getattr(sb, k)[idx].contiguous() for k in ARRAYS + ("path",)}
    state, ostate = torch.zeros((Bn, 64), dtype=torch.float64, device=dev), torch.zeros((Bn, 40), dtype=torch.float64, device=dev)
    i = idx.cpu().numpy()
    rc, r = _raw(solver, sb, tensors=t, B=Bn, ticks=Ts, sensor=se[i], sensor_state=state, sensor_noise=nz[:, i], observer=ob[i], observer_state=ostate)
    torch.cuda.synchronize()
    assert rc == 0 and (r["ticks_run"] == Ts).all() and (r["sensor_info"] == 0).all() and (r["observer_info"] == 0).all()
    for k in ARRAYS + ("path",):
        assert torch.equal(t[k], getattr(small[1], k)[idx]), k
    assert torch.equal(r["hist"], want["hist"][:, idx]) and torch.equal(r["sensor_rec"], want["sensor_rec"][idx]) and torch.equal(r["meas_hist"], want["meas_hist"][:, idx])
    assert torch.equal(r["observer_rec"], want["observer_rec"][idx]) and torch.equal(r["sample_hist"], want["sample_hist"][:, idx])
    assert torch.equal(state, small[1].sensor_state()[idx]) and torch.equal(ostate, small[1].observer_state()[idx])
    _close(small[:2], big[:2])


# ---- 6. invalid rows and the refusals ----
def test_invalid_rows_and_argument_errors_launch_nothing():
    """an invalid observer row does not run, its neighbours do; BMPC_ERR_ARG with an observer table: observer without sensor, observer without observer_state, and
    what the sensors' entry refuses; the stand-alone step; the errors of the Python layer"""
    import torch
    from boundmpc_amd._lib import BoundMPCHipError
    from boundmpc_amd.solver import _ptr
    from boundmpc_amd.stream import OBSERVER
    solver, sb, mpcs, recs = _made()
    sb.tick(max_iter=100, warm_dual=True)
    ob, se, nz = _rows([1, 1, 2, 3])
    bad = ob.copy(); bad[0, OBSERVER["LQ"]], bad[0, OBSERVER["GATE"]] = 0.0, -1.0
    sb.observer_state()[0] = 2.5; sb.sensor_state()[0] = 1.5
    torch.cuda.synchronize()
    before = _snapshot(sb)
    r = sb.rollout(T, sensor=se, sensor_noise=nz, want_meas=True, observer=bad, want_sample=True, want_observer_rec=True, **_on(N), **CONV_KW)
    torch.cuda.synchronize()
    assert r["observer_info"].tolist() == [1 << OBSERVER["LQ"] | 1 << OBSERVER["GATE"], 0, 0, 0] and r["sensor_info"].tolist() == [0] * B and r["ticks_run"].tolist() == [0, T, T, T]
    _assert_equal(before, _snapshot(sb), "an invalid row keeps every bit", rows=[0])
    assert (sb.observer_state()[0] == 2.5).all() and (sb.sensor_state()[0] == 1.5).all() and r["observer_rec"][0].tolist() == FRESH_REC
    for k in OUT + ("meas_hist", "sample_hist"):
        assert torch.isnan(r[k][:, 0]).all() and not torch.isnan(r[k][:, 1:, :21]).any(), k
    # the stand-alone step: the masks, and nothing touched
    rb = sb.robot.clone()
    info = sb.observe(se, bad, nz[0], tick=9)
    torch.cuda.synchronize()
    assert info.tolist() == r["observer_info"].tolist() and torch.equal(sb.robot[0], rb[0]) and not torch.equal(sb.robot[1:], rb[1:]) and (sb.observer_state()[0] == 2.5).all()
    sb.unsense(se)
    sb.sensor_reset(); sb.observer_reset()
    torch.cuda.synchronize()
    # the refusals, on a fresh batch
    sb2 = _made()
    sb2[1].tick(max_iter=100, warm_dual=True)
    Q, ev = _queue(sb2[2], sb2[3], sb2[1].entries), _events(2)
    state = torch.zeros((B, 64), dtype=torch.float64, device=sb.path.device)
    ostate = torch.zeros((B, 40), dtype=torch.float64, device=sb.path.device)
    torch.cuda.synchronize()
    before = _snapshot(sb2[1])
    ok = dict(replan=Q, leg_tick=ev["leg_tick"], leg_on=np.zeros_like(ev["leg_tick"]), disturb=ev["disturb"], sensor=se, sensor_state=state, observer=ob, observer_state=ostate)
    for kw in (dict(observer_state=None), dict(sensor=None, sensor_state=None), dict(sensor=None), dict(sensor_state=None), dict(plant=_plant(), plant_state=None), dict(leg_tick=None),
               dict(update_flags=8), dict(ticks=0), dict(flags=0), dict(goal_tol=-1.0), dict(audit_tol=-1.0), dict(log_stages=N + 1), dict(max_iter=-1), dict(handle=None)):
        assert _raw(sb2[0], sb2[1], **{**ok, **kw})[0] == 1, kw
    L, p = solver._lib, _ptr
    sensor, observer = torch.as_tensor(se, device=sb.path.device), torch.as_tensor(ob, device=sb.path.device)
    s2 = sb2[1]
    for args, oargs in (((None, B, p(s2.robot), p(s2.state), p(sensor), p(state)), (p(observer), p(ostate))), ((sb2[0]._h, 0, p(s2.robot), p(s2.state), p(sensor), p(state)), (p(observer), p(ostate))),
                        ((sb2[0]._h, B, p(s2.robot), p(s2.state), None, p(state)), (p(observer), p(ostate))), ((sb2[0]._h, B, p(s2.robot), p(s2.state), p(sensor), p(state)), (None, p(ostate))),
                        ((sb2[0]._h, B, p(s2.robot), p(s2.state), p(sensor), p(state)), (p(observer), None))):
        assert L.bmpc_stream_observe(*args, None, None, None, None, 0, *oargs, None, None, None, None) != 0
    with pytest.raises(ValueError, match="observer goes with sensor"):
        s2.rollout(2, warm_dual=True, observer=ob)
    with pytest.raises(ValueError, match="observer must be"):
        s2.rollout(2, warm_dual=True, sensor=se, observer=ob[:3])
    for kw in (dict(want_sample=True), dict(want_observer_rec=True)):
        with pytest.raises(ValueError, match="go with observer"):
            s2.rollout(2, warm_dual=True, sensor=se, **kw)
    with pytest.raises(BoundMPCHipError, match="invalid argument"):
        s2.rollout(0, warm_dual=True, sensor=se, observer=ob)
    torch.cuda.synchronize()
    _assert_equal(before, _snapshot(s2), "nothing was launched")
    assert (state == 0).all() and (ostate == 0).all() and (s2.observer_state() == 0).all()
    _close((solver, sb), sb2[:2])


# ---- 7. ordering ----
def test_a_graph_replay_behind_a_rollout_with_observers_on_another_stream_is_ordered():
    """A replay of the tick's graph enqueued on a second stream directly behind a rollout with observers of the same handle runs after it: the arrays equal
    those of the twin that synchronises between the two."""
    import torch
    a, b = _made(), _made()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _, sb, _, _ in (a, b):
        sb.tick_graph(warm_dual=True, stream=s1)      # tick 0, and the graph is in place
    torch.cuda.synchronize()
    Q = _queue(a[2], a[3], a[1].entries, 2)
    ob, se, nz = _rows([0, 1, 2, 3], 5)
    kw = dict(warm_dual=True, legs=Q, leg_tick=[[1, 3]] * B, sensor=se, sensor_noise=nz, observer=ob, stream=s1)
    a[1].rollout(5, **kw); torch.cuda.synchronize(); a[1].tick_graph(warm_dual=True, stream=s2)
    b[1].rollout(5, **kw); b[1].tick_graph(warm_dual=True, stream=s2)
    torch.cuda.synchronize()
    _assert_equal(_snapshot(a[1]), _snapshot(b[1]), "rollout with observers, then a tick replay on another stream")
    assert torch.equal(a[1].path, b[1].path) and torch.equal(a[1].legs, b[1].legs) and torch.equal(a[1].sensor_state(), b[1].sensor_state())
    assert torch.equal(a[1].observer_state(), b[1].observer_state())
    _close(a[:2], b[:2])
