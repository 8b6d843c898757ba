"""GPU: sensors inside a rollout (bmpc_stream_rollout_sensor, bmpc_stream_sense, bmpc_stream_unsense; StreamBatch.rollout(sensor=, sensor_noise=, want_meas=,
want_sensor_rec=), StreamBatch.sense, unsense; the kernels of csrc/bmpc_rollout_sensor.hip and csrc/bmpc_team_rollout_sensor.hip: csrc/bmpc_rollout_body.inl
with SE) -- against the contract: the entry against the loop {sense(), tick() on one wave per stream or on teams, unsense(), plant_step(), tube(), log(),
disturb(), update_device(splice=True) of the head records due} on a twin, converged and held, on the four tables of tests/test_stream_rollout_sensor.py; an
N = 12 handle for the instantiations with the iterate in the workspace; no table, the table of NaN and the identity table against rollout(plant=); invalid
rows; the g++ build of the same text; the stride over more streams than resident workgroups; a graph replay on another stream behind the launch; the
refusals.  (10, 4), B = 4 streams of tests/emu/emu_rollout.py, T = 6."""
import numpy as np
import pytest

from tests.rollout_contract import (ARRAYS, RAW_GROUPS, RAW_HEAD, RAW_INT32, assert_equal as _assert_equal, batch as _batch, close as _close, cut, history_rows,
                                    records as _records, small_streams as _small_streams, snapshot as _snapshot)

pytestmark = pytest.mark.gpu
N, S, T, B = 10, 4, 6, 4
NW = 4
HELD_KW = dict(max_iter=5, warm_dual=True, accept_capped=True)
CONV_KW = dict(max_iter=0, warm_dual=True, accept_capped=True)
OUT = ("hist", "traj_hist", "tube_hist", "log_hist")      # [ticks][B][..]
PER = ("ticks_run", "audit", "track", "legs_done", "leg_fired", "leg_why", "replan_info")      # [B][..]
NAN = float("nan")
SENSOR_GROUP = ("sensor", "sensor_state", "sensor_info", "sensor_rec", "sensor_noise", "meas_hist")
# The entry against the loop: asserted at 1e-11, the plants' bound for the same comparison -- the stand-alone kernels bmpc_stream_sense and
# bmpc_stream_unsense are another translation unit than the rollout kernels --; whether the run was bit-equal on top is printed.
LOOP_ATOL = 1e-11
FRESH_REC = [0, -np.inf, -1, -1, -np.inf, -1, 0, 0]


def _on(n):
    return dict(want_traj=True, audit=True, want_tube=True, want_log=True, log_stages=n, track=True)


def _queue(mpcs, recs, entries, K=2):
    kinds = [_records(mpcs, recs, entries), _records(mpcs, recs, entries, detour=0.05)]
    return np.ascontiguousarray(np.stack([kinds[k % 2] for k in range(K)], axis=1))


def _events(ticks=T, n=B):
    from tests.emu import emu_rollout as ee
    return dict(leg_tick=np.array([[1, 4], [2, 4], [1, 4], [2, 4]], dtype=np.int32)[:n], disturb=ee.disturbances(ticks, n, on=(1, 4)))


def _made(held=False, team=False, n=B, horizon=N, segs=S):
    mpcs, recs = _small_streams(horizon, segs, n=n)
    solver, sb = _batch(horizon, segs, mpcs, recs, one_wave=not team, held=held)
    if team:
        solver.set_team_waves(NW)
    return solver, sb, mpcs, recs


def _tables():
    from tests.test_stream_rollout_sensor import _tables as tables
    return tables()


def _plant(n=B):
    from tests.test_stream_rollout_sensor import _plant as plant
    return plant()[:n]


def _noise(which, ticks=T, n=B):
    from tests.emu import emu_rollout_sensor as es
    return None if which in ("res", "nan") else es.noise(ticks, n)


def _deviation(x, y):
    x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
    assert x.shape == y.shape and np.array_equal(np.isnan(x), np.isnan(y)), "shapes or NaN slots differ"
    with np.errstate(invalid="ignore"):
        d = np.abs(x - y)
    return float(np.nanmax(np.where(np.isinf(x) & (x == y), 0.0, d), initial=0.0))


def _loop(sb, ticks, sensor, noise=None, dist=None, queue=None, leg_tick=None, plant=None, **kw):
    """The contract's loop on the batch `sb` (tests/rollout_contract.py contract_loop with the two steps of the sensor around the tick): per tick sense(tick t, the
    noise rows of tick t), one fused tick (on one wave per stream or on teams, as the batch's handle is set), unsense(), plant_step(tick t) with a plant table,
    tube(), log(), disturb() with the rows of the tick, update_device(set_goal, splice) with the flags of the streams raised whose HEAD record is due (leg_tick
    [B][K]: no condition but the tick).  The sensors and the drives start where the launch starts them: sensor_reset and plant_reset ahead of the first tick.
    Every stream must keep its plan (a stream without one stops in the rollout, and takes no sample here).
    -> dict(hist, traj_hist, tube_hist, log_hist: whole rows, meas_hist, truth_hist: the robot records ahead of every sample, ticks_run, replan_info, legs_done,
    leg_fired, queue, plant_state, plant_rec, sensor_state, sensor_rec)"""
    import torch
    from boundmpc_amd import stream as bstream
    from tests.emu.emu_rollout import due as due_of
    SS, n = bstream.SS, sb.B
    r = dict(hist=np.full((ticks, n, 52), np.nan), traj_hist=np.full((ticks, n, sb.tr_len), np.nan), tube_hist=np.full((ticks, n, 16), np.nan),
             log_hist=np.full((ticks, n, bstream.log_len(sb.N)), np.nan), meas_hist=np.full((ticks, n, 43), np.nan), truth_hist=np.full((ticks, n, 43), np.nan),
             ticks_run=np.zeros(n, dtype=int))
    if queue is not None:
        K = queue.shape[1]
        r.update(queue=queue.copy(), legs_done=np.zeros(n, dtype=int), leg_fired=np.full((n, K), -1), replan_info=np.full((n, K), -1))
    sb.sensor_reset()
    if plant is not None:
        sb.plant_reset()
    for t in range(ticks):
        assert (sb.state[:, SS["ERRCNT"]].cpu().numpy() < sb.N).all(), "a stream lost its plan"
        r["truth_hist"][t] = sb.robot.cpu().numpy()
        sinfo = sb.sense(sensor, None if noise is None else noise[t], tick=t)
        sb.tick(simulate=True, **kw)
        sb.unsense(sensor)
        pinfo = sb.plant_step(plant, tick=t) if plant is not None else None
        tube, log = sb.tube(), sb.log()
        torch.cuda.synchronize()
        assert not sinfo.any() and (pinfo is None or not pinfo.any())
        s = _snapshot(sb)
        r["hist"][t], r["traj_hist"][t], r["ticks_run"][:] = history_rows(s), s["traj"], t + 1
        r["tube_hist"][t], r["log_hist"][t], r["meas_hist"][t] = tube.cpu().numpy(), log.cpu().numpy(), sb.meas.cpu().numpy()
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
    if plant is not None:
        r["plant_state"], r["plant_rec"] = sb.plant_state.cpu().numpy(), sb.plant_rec.cpu().numpy()
    return r


def _compare(what, out, loop, entry_sb, loop_sb, n_stages, plant=True, queue=True):
    """the entry's arrays against the loop's: -> (deviations by array, bit-equal)"""
    got, want = _snapshot(entry_sb), _snapshot(loop_sb)
    pairs = {k: (got[k], want[k]) for k in ARRAYS if k not in ("iters", "status")}
    pairs.update({k: (out[k].cpu().numpy(), loop[k]) for k in ("hist", "traj_hist", "tube_hist", "meas_hist")})
    pairs.update(log_hist=(out["log_hist"].cpu().numpy(), cut(loop["log_hist"], entry_sb.N, n_stages)), path=(entry_sb.path.cpu().numpy(), loop_sb.path.cpu().numpy()),
                 sensor_state=(entry_sb.sensor_state().cpu().numpy(), loop["sensor_state"]), sensor_rec=(out["sensor_rec"].cpu().numpy(), loop["sensor_rec"]))
    if queue:
        pairs.update(queue=(entry_sb.legs.cpu().numpy(), loop["queue"]))
    if plant:
        pairs.update(plant_state=(entry_sb.plant_state.cpu().numpy(), loop["plant_state"]), plant_rec=(out["plant_rec"].cpu().numpy(), loop["plant_rec"]))
    devs = {k: _deviation(x, y) for k, (x, y) in pairs.items()}
    bits = all(np.array_equal(x, y, equal_nan=True) for x, y in pairs.values())
    print(f"{what}: largest deviation entry - loop", " ".join(f"{k} {d:.2e}" for k, d in devs.items()), "| bit-equal:", bits)
    assert np.array_equal(got["iters"], want["iters"]) and np.array_equal(got["status"], want["status"])
    return devs, bits


# ---- 1. the contract ----
@pytest.mark.parametrize("which", ["bn", "res", "hold", "nan"])
@pytest.mark.parametrize("team", [False, True])
@pytest.mark.parametrize("mode", ["converged", "held"])
def test_a_rollout_with_sensors_equals_the_per_tick_loop(mode, team, which):
    import torch
    from boundmpc_amd.stream import SENSOR, SENSOR_REC
    from tests.test_stream_rollout_sensor import RES16, TIE_MARGIN, _identity_row
    held = mode == "held"
    kw, waves = HELD_KW if held else CONV_KW, NW if team else None
    what = f"{mode}, {'teams' if team else 'one wave'}, {which}"
    tab, nz, plant = _tables()[which], _noise(which), _plant()
    a, b = _made(held, team), _made(held, team)
    for _, sb, _, _ in (a, b):
        sb.tick(max_iter=100, warm_dual=True)
    Q, ev = _queue(a[2], a[3], a[1].entries), _events()
    loop = _loop(a[1], T, tab, nz, dist=ev["disturb"], queue=Q, leg_tick=ev["leg_tick"], plant=plant, **kw)
    out = b[1].rollout(T, legs=Q, plant=plant, want_plant_rec=True, sensor=tab, sensor_noise=nz, want_meas=True, want_sensor_rec=True, waves=waves, **ev, **_on(N), **kw)
    torch.cuda.synchronize()
    assert out["sensor_info"].tolist() == [0] * B and out["plant_info"].tolist() == [0] * B and out["ticks_run"].tolist() == [T] * B == loop["ticks_run"].tolist()
    for k in ("legs_done", "leg_fired", "replan_info"):
        assert out[k].cpu().numpy().tolist() == loop[k].tolist(), f"{what}: {k}"
    if which == "res":      # one ulp ahead of rint must flip no step between the two builds: every m_q / RES of the run lies away from a rounding tie
        m = (loop["truth_hist"][:, :, :7] + tab[None, :, :7]) / RES16
        worst = float(np.abs(np.abs(m - np.floor(m)) - 0.5).min())
        print(f"{what}: nearest rounding tie {worst:.3e} steps away")
        assert worst >= TIE_MARGIN
    devs, bits = _compare(what, out, loop, b[1], a[1], N)
    assert max(devs.values()) <= LOOP_ATOL, devs
    # hist is the truth and meas_hist the sample: a row that is no identity has handed out something else than the plant, an identity row the plant itself
    rec = out["sensor_rec"].cpu().numpy()
    for s_ in range(B):
        assert (rec[s_, SENSOR_REC["MAX_DQ"]] == 0.0) == _identity_row(tab[s_]) == np.array_equal(loop["meas_hist"][:, s_], loop["truth_hist"][:, s_]), f"{what}: row {s_}"
    assert (rec[:, SENSOR_REC["SAMPLES"]] == T).all() and np.array_equal(b[1].robot.cpu().numpy(), out["hist"][T - 1].cpu().numpy()[:, :43])
    _close(a[:2], b[:2])


def test_the_kernels_with_the_iterate_in_the_workspace():
    """one N = 12 handle, 2 streams, T = 3: the two instantiations without ZLDS, against the loop"""
    import torch
    from boundmpc_amd import stream as bstream
    from tests.emu import emu_rollout as ee, emu_rollout_sensor as es
    n12, Ts = 12, 3
    tab = bstream.sensor_table(2, bias=[[1e-3] * 7, [NAN] * 7], nq=[1e-4, 1e-4], hold=[NAN, 1.0])
    nz, d = es.noise(Ts, 2), ee.disturbances(Ts, 2, on=(1,))
    a, b = _made(n=2, horizon=n12), _made(n=2, horizon=n12)
    for _, sb, _, _ in (a, b):
        sb.tick(max_iter=100, warm_dual=True)
    loop = _loop(a[1], Ts, tab, nz, dist=d, **CONV_KW)
    out = b[1].rollout(Ts, sensor=tab, sensor_noise=nz, want_meas=True, want_sensor_rec=True, disturb=d, **_on(n12), **CONV_KW)
    torch.cuda.synchronize()
    assert out["sensor_info"].tolist() == [0, 0] and out["ticks_run"].tolist() == [Ts] * 2
    devs, bits = _compare("N = 12", out, loop, b[1], a[1], n12, plant=False, queue=False)
    assert max(devs.values()) <= LOOP_ATOL, devs
    assert (out["sensor_rec"][:, 1] > 0).all()
    _close(a[:2], b[:2])


def _raw(solver, sb, tensors=None, waves=None, **over):
    """bmpc_stream_rollout_sensor called directly with the batch's own tensors (or `tensors`: ARRAYS + path, of `B` streams) and every output array of the entry
    filled with -7 (tests/rollout_contract.py raw_rollout with the sensor's group behind the plant's): `over` names arguments of the entry; an array is put on the
    device, a tensor taken as it is, None is NULL.  What is not named: ticks 2, max_iter 0, flags 3, goal_tol 0, update_flags 3, audit_tol 1e-6, log_stages 1,
    legs = the K of a queue `replan` (1 without one), every other input pointer NULL.  -> (the return code, dict of what was passed by name)"""
    import torch
    from boundmpc_amd.solver import _ptr
    dev = sb.path.device
    names = RAW_HEAD + tuple(n for g in RAW_GROUPS for n in g if n != "replan_tick") + SENSOR_GROUP
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
                  sensor_info=(nb,), sensor_rec=(nb, 8), meas_hist=(n, nb, 43))
    ints = ("ticks_run", "replan_info", "legs_done", "leg_fired", "leg_why", "tune_info", "plant_info", "sensor_info")
    for k, shape in shapes.items():
        if k not in over:
            a[k] = torch.full(shape, -7, dtype=torch.int32 if k in ints else torch.float64, device=dev)
    former = solver.rollout_waves
    if waves is not None:
        solver.set_rollout_waves(waves)
    rc = solver._lib.bmpc_stream_rollout_sensor(*[_ptr(a.get(k)) if torch.is_tensor(a.get(k)) else a.get(k) for k in names], None)
    solver.set_rollout_waves(former)
    return rc, a


# ---- 2. no table, the table of NaN, the identity table ----
@pytest.mark.parametrize("waves", [None, NW])
def test_no_table_a_table_of_nan_and_the_identity_table_are_the_plants_entry(waves):
    import torch
    from tests.emu import emu_rollout_sensor as es
    made = [_made() for _ in range(4)]
    for _, sb, _, _ in made:
        sb.tick(max_iter=100, warm_dual=True)
    Q, ev, plant, nz = _queue(made[0][2], made[0][3], made[0][1].entries), _events(), _plant(), es.noise(T, B)
    want = made[0][1].rollout(T, legs=Q, plant=plant, want_plant_rec=True, waves=waves, **ev, **_on(N), **CONV_KW)
    sen = dict(sensor_noise=nz, want_meas=True, want_sensor_rec=True)
    nan = made[1][1].rollout(T, legs=Q, plant=plant, want_plant_rec=True, sensor=np.full((B, 16), NAN), waves=waves, **sen, **ev, **_on(N), **CONV_KW)
    ident = made[2][1].rollout(T, legs=Q, plant=plant, want_plant_rec=True, sensor=np.zeros((B, 16)), waves=waves, **sen, **ev, **_on(N), **CONV_KW)
    pst = made[3][1].plant_reset()
    rc, none = _raw(made[3][0], made[3][1], waves=waves, ticks=T, log_stages=N, replan=Q, leg_tick=ev["leg_tick"], leg_on=np.zeros_like(ev["leg_tick"]), disturb=ev["disturb"],
                    plant=plant, plant_state=pst, sensor=None, sensor_state=None, sensor_noise=nz)
    torch.cuda.synchronize()
    assert rc == 0
    for r, sb, what in ((nan, made[1][1], "a table of NaN"), (ident, made[2][1], "the identity table"), (none, made[3][1], "no table")):
        _assert_equal(_snapshot(made[0][1]), _snapshot(sb), what)
        assert torch.equal(made[0][1].path, sb.path) and torch.equal(made[0][1].plant_state, sb.plant_state)
        for k in OUT + PER + ("plant_info", "plant_rec"):
            assert np.array_equal(want[k].cpu().numpy(), r[k].cpu().numpy(), equal_nan=True), f"{what}: {k}"
    assert torch.equal(made[0][1].legs, made[1][1].legs) and torch.equal(made[0][1].legs, made[2][1].legs) and torch.equal(made[0][1].legs, none["replan"])
    for r, sb in ((nan, made[1][1]), (ident, made[2][1])):      # the samples are the truth
        assert r["sensor_info"].tolist() == [0] * B and r["sensor_rec"].tolist() == [[T, 0, 0, 0, 0, 0, 0, 0]] * B
        st = sb.sensor_state().cpu().numpy()
        assert (st[:, 21] == 1).all() and (st[:, 22] == 1).all() and np.array_equal(st[:, :21], r["meas_hist"][T - 1].cpu().numpy()[:, :21])
    assert none["sensor_info"].tolist() == [-7] * B and (none["sensor_rec"] == -7.0).all() and (none["meas_hist"] == -7.0).all()      # (not looked at)
    _close(*[m[:2] for m in made])


# ---- 3. invalid rows ----
@pytest.mark.parametrize("waves", [None, NW])
def test_invalid_rows_do_not_run_and_their_neighbours_do(waves):
    import torch
    from boundmpc_amd.stream import SENSOR
    from tests.emu import emu_rollout_sensor as es
    a, b = _made(), _made()
    for _, sb, _, _ in (a, b):
        sb.tick(max_iter=100, warm_dual=True)
    Q, ev, tab, nz = _queue(a[2], a[3], a[1].entries), _events(), _tables()["bn"], es.noise(T, B)
    bad = tab.copy()
    bad[0, SENSOR["RES"]], bad[0, SENSOR["BIAS"] + 5] = -1.0, np.inf
    bad[3, SENSOR["HOLD"]] = 0.5
    for k in ("x", "g", "kkt"):
        getattr(b[1], k)[[0, 3]] = 7.25
    b[1].iters[[0, 3]] = 77; b[1].status[[0, 3]] = 9
    b[1].sensor_state()[[0, 3]] = 1.5
    torch.cuda.synchronize()
    before, path = _snapshot(b[1]), b[1].path.clone()
    sen = dict(sensor_noise=nz, want_meas=True, want_sensor_rec=True)
    good = a[1].rollout(T, legs=Q, sensor=tab, waves=waves, **sen, **ev, **_on(N), **CONV_KW)
    r = b[1].rollout(T, legs=Q, sensor=bad, waves=waves, **sen, **ev, **_on(N), **CONV_KW)
    torch.cuda.synchronize()
    assert r["sensor_info"].tolist() == [1 << SENSOR["RES"] | 1 << SENSOR["BIAS"] + 5, 0, 0, 1 << SENSOR["HOLD"]] and r["ticks_run"].tolist() == [0, T, T, 0]
    got, ok = _snapshot(b[1]), _snapshot(a[1])
    _assert_equal(before, got, "invalid rows keep every bit", rows=[0, 3])
    _assert_equal(ok, got, "the neighbours", rows=[1, 2])
    assert torch.equal(b[1].path[[0, 3]], path[[0, 3]]) and torch.equal(b[1].path[[1, 2]], a[1].path[[1, 2]]) and torch.equal(b[1].legs[[1, 2]], a[1].legs[[1, 2]])
    assert np.array_equal(b[1].legs[[0, 3]].cpu().numpy(), Q[[0, 3]])      # (their records keep their flags)
    assert (b[1].sensor_state()[[0, 3]] == 1.5).all() and torch.equal(b[1].sensor_state()[[1, 2]], a[1].sensor_state()[[1, 2]])      # (the state they started from: untouched)
    for k in OUT + ("meas_hist",):
        assert torch.isnan(r[k][:, [0, 3]]).all() and np.array_equal(r[k][:, [1, 2]].cpu().numpy(), good[k][:, [1, 2]].cpu().numpy(), equal_nan=True), k
    for k in PER + ("sensor_rec",):
        assert np.array_equal(r[k][[1, 2]].cpu().numpy(), good[k][[1, 2]].cpu().numpy(), equal_nan=True), k
    assert r["legs_done"][[0, 3]].tolist() == [0, 0] and (r["leg_fired"][[0, 3]] == -1).all() and (r["replan_info"][[0, 3]] == -1).all()
    assert r["sensor_rec"][[0, 3]].tolist() == [FRESH_REC] * 2
    # the stand-alone steps: the mask, and nothing touched
    rb, st = b[1].robot.clone(), b[1].sensor_state().clone()
    b[1].sensor_rec = None
    info = b[1].sense(bad, nz[0], tick=9)
    torch.cuda.synchronize()
    assert info.tolist() == r["sensor_info"].tolist() and torch.equal(b[1].robot[[0, 3]], rb[[0, 3]]) and not torch.equal(b[1].robot[[1, 2]], rb[[1, 2]])
    assert torch.equal(b[1].sensor_state()[[0, 3]], st[[0, 3]]) and b[1].sensor_rec[[0, 3]].tolist() == [FRESH_REC] * 2 and torch.isnan(b[1].meas[[0, 3]]).all()
    sample = b[1].robot.clone()
    b[1].unsense(bad)
    torch.cuda.synchronize()
    assert torch.equal(b[1].robot[[0, 3]], rb[[0, 3]]) and not torch.equal(b[1].robot[[1, 2], :33], sample[[1, 2], :33])
    _close(a[:2], b[:2])


# ---- 4. the GPU against the CPU build of the same text ----
def test_a_rollout_with_sensors_on_the_gpu_equals_the_cpu_build_of_the_same_text():
    """(2, 2) -- the shape of every comparison of the device with the g++ build in this suite; at (10, 4) a first run of this test found the state rows of the two
    builds 1.3e-7 apart behind six converged ticks, and did not separate two solvers that stop at a tolerance from the sensor text, which the comparisons with
    the loop pin at (10, 4) bit for bit on either build --, from the cold start with the dual state, T = 6, a run whose
    ticks all converge, disturbances: the device arrays against tests/emu's g++ build of the kernel text at 1e-11 with its two exclusions (iterations, kkt),
    as the plants' test.  The RES row: its margin from a rounding tie asserted on the CPU build's values."""
    import torch
    from boundmpc_amd import stream as bstream
    from tests.emu import emu, emu_rollout as ee, emu_rollout_sensor as es
    from tests.test_stream_rollout_sensor import RES16, TIE_MARGIN
    n2, s2 = 2, 2
    solver, sb, mpcs, recs = _made(horizon=n2, segs=s2)
    _, A, Tab, _ = ee.small_batch(n2, s2, B)
    A0rb = A["rb"].copy()
    bias = np.random.default_rng(29).uniform(-1e-3, 1e-3, 7)
    tab = bstream.sensor_table(B, bias=[[1e-3] * 7, bias, [NAN] * 7, [NAN] * 7], res=[NAN, RES16, NAN, NAN], nq=[1e-4, NAN, 1e-4, NAN], hold=[NAN, NAN, 1.0, NAN])
    nz, d = es.noise(T, B), ee.disturbances(T, B, on=(1, 4))
    out = sb.rollout(T, warm_dual=True, accept_capped=True, want_traj=True, disturb=d, sensor=tab, sensor_noise=nz, want_meas=True, want_sensor_rec=True)
    torch.cuda.synchronize()
    got, hist, th = _snapshot(sb), out["hist"].cpu().numpy(), out["traj_hist"].cpu().numpy()
    st = np.zeros((B, 64))
    r = es.rollout(n2, s2, 0.1, Tab, A, T, sensor=tab, sensor_state=st, sensor_noise=nz, disturb=d, accept_capped=True, opts=emu.opts_for(n2, start_rollout=0))
    assert r["ran"] == es.RAN_SENSOR and out["ticks_run"].tolist() == r["ticks_run"].tolist() == [T] * B and out["sensor_info"].tolist() == r["sensor_info"].tolist() == [0] * B
    # the truth ahead of tick t on the CPU build: the history row behind tick t - 1 with its disturbance
    truth = np.concatenate([A0rb[None], np.stack([np.stack([bstream.disturb_robot(r["hist"][t, b, :43], d[t, b]) for b in range(B)]) for t in range(T - 1)])])
    m = (truth[:, 1, :7] + tab[1, :7]) / RES16
    worst = float(np.abs(np.abs(m - np.floor(m)) - 0.5).min())
    print(f"RES row: nearest rounding tie {worst:.3e} steps away")
    assert worst >= TIE_MARGIN
    rec = out["sensor_rec"].cpu().numpy()
    assert np.array_equal(rec[:, [0, 2, 3, 5]], r["sensor_rec"][:, [0, 2, 3, 5]])
    pairs = [(got["state"], A["ss"]), (got["robot"], A["rb"]), (got["p"], A["p"]), (got["x0"], A["x0"]), (got["x"], A["x"]), (got["g"], A["g"]), (got["traj"], A["traj"]),
             (np.delete(hist, [45, 47], axis=2), np.delete(r["hist"], [45, 47], axis=2)), (th, r["traj_hist"]), (sb.path.cpu().numpy(), Tab),
             (out["meas_hist"].cpu().numpy(), r["meas_hist"]), (sb.sensor_state().cpu().numpy(), st), (rec[:, [1, 4]], r["sensor_rec"][:, [1, 4]]), (np.sqrt(rec[:, 6]), np.sqrt(r["sensor_rec"][:, 6]))]
    devs = [float(np.abs(x - y).max()) for x, y in pairs]
    print("largest deviation GPU - CPU build: state, robot, p, x0, x, g, traj, hist, traj_hist, path, meas_hist, sensor_state, MAX_DQ / MAX_DP, sqrt(SUMSQ_DQ):", " ".join(f"{v:.3e}" for v in devs))
    assert max(devs) <= 1e-11
    _close((solver, sb))


# ---- 5. the stride ----
def test_the_stride_serves_more_streams_than_resident_workgroups():
    """The arrays of the 4-stream batch tiled to B = grid + 2 rows, the rows cycling through the table, 2 ticks: every replica of stream i bit-equal to the
    4-stream run, its sensor state, record and meas_hist rows included"""
    import torch
    from tests.emu import emu_rollout_sensor as es
    Ts = 2
    small, big = _made(), _made()
    tab, nz = _tables()["hold"], es.noise(Ts, B)
    tab[3, 7] = 1e-3
    want = small[1].rollout(Ts, warm_dual=True, accept_capped=True, sensor=tab, sensor_noise=nz, want_meas=True, want_sensor_rec=True)
    solver, sb = big[:2]
    dev = sb.path.device
    Bn = solver.launch_info()["grid"] + 2
    idx = torch.arange(Bn, device=dev) % B
    t = {k: getattr(sb, k)[idx].contiguous() for k in ARRAYS + ("path",)}
    state = torch.zeros((Bn, 64), dtype=torch.float64, device=dev)
    i = idx.cpu().numpy()
    rc, r = _raw(solver, sb, tensors=t, B=Bn, ticks=Ts, sensor=tab[i], sensor_state=state, sensor_noise=nz[:, i])
    torch.cuda.synchronize()
    assert rc == 0 and (r["ticks_run"] == Ts).all() and (r["sensor_info"] == 0).all()
    for k in ARRAYS + ("path",):
        assert torch.equal(t[k], getattr(small[1], k)[idx]), k
    assert torch.equal(r["hist"], want["hist"][:, idx]) and torch.equal(r["sensor_rec"], want["sensor_rec"][idx]) and torch.equal(r["meas_hist"], want["meas_hist"][:, idx])
    assert torch.equal(state, small[1].sensor_state()[idx])
    _close(small[:2], big[:2])


# ---- 6. the refusals ----
def test_argument_errors_launch_nothing():
    """BMPC_ERR_ARG with a sensor table: sensor without sensor_state, and what the plants' entry refuses; the errors of the Python layer"""
    import torch
    from boundmpc_amd._lib import BoundMPCHipError
    from boundmpc_amd.solver import _ptr
    solver, sb, mpcs, recs = _made()
    Q, ev, tab = _queue(mpcs, recs, sb.entries), _events(2), _tables()["bn"]
    state = torch.zeros((B, 64), dtype=torch.float64, device=sb.path.device)
    pst = torch.zeros((B, 16), dtype=torch.float64, device=sb.path.device)
    torch.cuda.synchronize()
    before = _snapshot(sb)
    ok = dict(replan=Q, leg_tick=ev["leg_tick"], leg_on=np.zeros_like(ev["leg_tick"]), disturb=ev["disturb"], sensor=tab, sensor_state=state)
    for kw in (dict(sensor_state=None), dict(plant=_plant(), plant_state=None), dict(leg_tick=None), dict(legs_done=None), dict(update_flags=8), dict(update_flags=4), dict(ticks=0),
               dict(flags=0), dict(flags=2), dict(goal_tol=-1.0), dict(goal_tol=float("nan")), dict(audit_tol=-1.0), dict(log_stages=0), dict(log_stages=N + 1), dict(max_iter=-1),
               dict(handle=None)):
        assert _raw(solver, sb, **{**ok, **kw})[0] == 1, kw
    L, p = solver._lib, _ptr
    sensor = torch.as_tensor(tab, device=sb.path.device)
    for args in ((None, B, p(sb.robot), p(sb.state), p(sensor), p(state)), (solver._h, 0, p(sb.robot), p(sb.state), p(sensor), p(state)), (solver._h, B, None, p(sb.state), p(sensor), p(state)),
                 (solver._h, B, p(sb.robot), None, p(sensor), p(state)), (solver._h, B, p(sb.robot), p(sb.state), None, p(state)), (solver._h, B, p(sb.robot), p(sb.state), p(sensor), None)):
        assert L.bmpc_stream_sense(*args, None, None, None, None, 0, None) != 0 and L.bmpc_stream_unsense(*args, None) != 0
    with pytest.raises(ValueError, match="does not go with"):
        sb.rollout(2, warm_dual=True, sensor=tab, replan=Q[:, 0], replan_tick=[1] * B)
    with pytest.raises(ValueError, match="sensor must be"):
        sb.rollout(2, warm_dual=True, sensor=tab[:3])
    for kw in (dict(want_meas=True), dict(want_sensor_rec=True), dict(sensor_noise=np.zeros((2, B, 21)))):
        with pytest.raises(ValueError, match="go with sensor"):
            sb.rollout(2, warm_dual=True, **kw)
    with pytest.raises(BoundMPCHipError, match="invalid argument"):
        sb.rollout(0, warm_dual=True, sensor=tab)
    torch.cuda.synchronize()
    _assert_equal(before, _snapshot(sb), "nothing was launched")
    assert (state == 0).all() and (sb.sensor_state() == 0).all()
    _close((solver, sb))


# ---- 7. ordering ----
def test_a_graph_replay_behind_a_rollout_with_sensors_on_another_stream_is_ordered():
    """A replay of the tick's graph enqueued on a second stream directly behind a rollout with sensors of the same handle runs after it: the arrays equal
    those of the twin that synchronises between the two."""
    import torch
    from tests.emu import emu_rollout_sensor as es
    a, b = _made(), _made()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _, sb, _, _ in (a, b):
        sb.tick_graph(warm_dual=True, stream=s1)      # tick 0, and the graph is in place
    torch.cuda.synchronize()
    Q = _queue(a[2], a[3], a[1].entries, 2)
    kw = dict(warm_dual=True, legs=Q, leg_tick=[[1, 3]] * B, sensor=_tables()["bn"], sensor_noise=es.noise(5, B), stream=s1)
    a[1].rollout(5, **kw); torch.cuda.synchronize(); a[1].tick_graph(warm_dual=True, stream=s2)
    b[1].rollout(5, **kw); b[1].tick_graph(warm_dual=True, stream=s2)
    torch.cuda.synchronize()
    _assert_equal(_snapshot(a[1]), _snapshot(b[1]), "rollout with sensors, then a tick replay on another stream")
    assert torch.equal(a[1].path, b[1].path) and torch.equal(a[1].legs, b[1].legs) and torch.equal(a[1].sensor_state(), b[1].sensor_state())
    _close(a[:2], b[:2])
