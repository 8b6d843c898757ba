"""Plants inside a rollout -- a table of actuator models per stream between the first planned jerk of a tick and the plant, validated on the device -- as
device code compiled for the CPU (csrc/bmpc_rollout_kernel.inl with PL, csrc/bmpc_stream_plant.inl; tests/emu/bmpc_emu_rollout.cpp, once for one wave
per stream and once for teams of four).  The checker is the contract: the entry against the per-tick loop {tick text, plant step text, tube text, log text,
disturb text, update text of the head record due} for one stream (emu_rollout.contract_loop with a plant row), bit for bit.  (2, 2), B = 4 streams of
emu_rollout.small_stream behind a solved-out tick 0, T = 6, as the sweeps' and the missions' tests; (1, 2) and (10, 4) once each.
Two tables, since four streams hold four rows: LIN = gain 0.8 on all joints / a bias on one joint / LAG 0.5 / DELAY 1, and SAT = a clip placed between two
values of that stream's own |first planned jerk| trace of the plain run / gain 0.8 with the same kind of clip / LAG 0.5 with DELAY 1 / all NaN."""
import ctypes
import functools
import inspect
import os
import re

import numpy as np
import pytest

from boundmpc_amd import stream as bstream
from tests.emu import emu_rollout as er, emu_stream_tube as et

PLANT, PLANT_STATE, PLANT_REC, ROLL, RB, RP, SS, TUBE = bstream.PLANT, bstream.PLANT_STATE, bstream.PLANT_REC, bstream.ROLL, bstream.RB, bstream.RP, bstream.SS, bstream.TUBE
N, S, T, B = 2, 2, 6, 4
H = er.H
NAN = float("nan")
_copy = er.copy_arrays
JERK = slice(RB["JERK"], RB["JERK"] + 7)
CMD = slice(PLANT_STATE["CMD"], PLANT_STATE["CMD"] + 7)
ACT = slice(PLANT_STATE["ACT"], PLANT_STATE["ACT"] + 7)
BUILDS = [(1, 0, 0), (1, 0, 1), (4, 0, 0), (4, 1, 1)]      # (waves, wave order, lane order)


def _queue(K=2):
    """[B][K][len]: a leg back, then a leg back with a detour, per stream"""
    kinds = [er.small_batch(N, S, B)[3], er.small_batch(N, S, B, detour=0.05)[3]]
    return np.ascontiguousarray(np.stack([kinds[k % 2] for k in range(K)], axis=1))


def _events():
    """a two-record queue (record 0 behind tick 1 or 2, record 1 behind tick 4) and disturbances on ticks 1 and 4: the sweeps' events"""
    lt = np.array([[1, 4], [2, 4], [1, 4], [2, 4]], dtype=np.int32)
    return dict(leg_tick=lt, leg_on=np.zeros((B, 2), dtype=np.int32), disturb=er.disturbances(T, B, on=(1, 4)))


def _state0(A0):
    return bstream.plant_state_of(A0["rb"])


@functools.lru_cache(maxsize=None)
def _plain(nw, events=True):
    """the run WITHOUT a plant table on the inputs of the contract test (events: the queue, the disturbances and the sweeps' table; else none of them):
    (result, arrays).  Shared, never written."""
    A0, Tab, _ = er.start(N, S, nw, B)
    A, Tb = _copy(A0), Tab.copy()
    kw = dict(tune=er.table(), replan=_queue(), accept_capped=True, **_events()) if events else {}
    r = er.rollout(N, S, H, Tb, A, T, entry=6, plant=None, plant_state=None, nw=nw, log_stages=N, **kw)
    assert r["ran"] == (5 if events else 3) and r["ticks_run"].tolist() == [T] * B
    return r, A


def _sat_between(trace):
    """a clip between two neighbouring values of a stream's |first planned jerk| trace [T]: the middle of the widest gap, so that the stream clips on some
    ticks and not on others -- the way the missions' tests place their tolerances"""
    v = np.sort(trace)
    k = int(np.argmax(np.diff(v)))
    assert v[k + 1] > v[k]
    return 0.5 * (v[k] + v[k + 1])


def _tables(nw, events=True):
    plain = _plain(nw, events)[0]
    peak = np.abs(plain["hist"][:, :, JERK]).max(axis=2)      # [T][B]: without a plant the record's jerk IS the command
    bias = np.zeros(7); bias[3] = 0.05
    lin = bstream.plant_table(B, gain=[[0.8] * 7, [NAN] * 7, [NAN] * 7, [NAN] * 7], bias=[[NAN] * 7, bias, [NAN] * 7, [NAN] * 7], lag=[NAN, NAN, 0.5, NAN],
                              delay=[NAN, NAN, NAN, 1.0])
    sat = bstream.plant_table(B, gain=[[NAN] * 7, [0.8] * 7, [NAN] * 7, [NAN] * 7], sat=[_sat_between(peak[:, 0]), 0.8 * _sat_between(peak[:, 1]), NAN, NAN],
                              lag=[NAN, NAN, 0.5, NAN], delay=[NAN, NAN, 1.0, NAN])
    assert np.isnan(sat[3]).all()
    return dict(lin=lin, sat=sat)


# ---- 1., 2. the contract; an ignored table cannot pass ----
@pytest.mark.parametrize("nw,wave_order,lane_order,which", [b + (w,) for b, w in zip(BUILDS, ("lin", "sat", "sat", "lin"))])
def test_a_rollout_with_plants_equals_the_per_tick_loop(nw, wave_order, lane_order, which):
    """events, audit, log, tracking record, a two-record queue and the sweeps' table on: every tick array, history array, record, queue output, plant_state
    and plant_rec of every stream against contract_loop; every non-identity row changes the history of its stream against the run without a plant (on inputs
    with which every stream keeps a plan for all T ticks); the clipped stream clips on some ticks and not on others"""
    A0, Tab, _ = er.start(N, S, nw, B)
    tab = _tables(nw)[which]
    r, A, Tb, R, st = er.assert_equals_the_loop(N, S, A0, Tab, _queue(), T, f"{which}, nw {nw} orders {wave_order} {lane_order}", plant=tab, state0=_state0(A0), nw=nw, wave_order=wave_order,
                                                lane_order=lane_order, stages=N, tune=er.table(), accept_capped=True, **_events())
    assert r["plant_info"].tolist() == [0] * B and r["ticks_run"].tolist() == [T] * B and r["legs_done"].tolist() == [2] * B      # (the condition on the inputs)
    assert (r["hist"][:, :, ROLL["ERRCNT"]] < N).all() and (r["plant_rec"][:, PLANT_REC["SAMPLES"]] == T).all()
    plain = _plain(nw)[0]
    for b in range(B):
        same = np.array_equal(r["hist"][:, b], plain["hist"][:, b])
        assert same == bool(np.isnan(tab[b]).all()), f"row {b} of {which}: " + ("changed nothing" if same else "an identity row changed the history")
    if which == "sat":
        for b in (0, 1):
            assert 0 < r["plant_rec"][b, PLANT_REC["N_SAT"]] < r["plant_rec"][b, PLANT_REC["SAMPLES"]], r["plant_rec"][b]
        assert r["plant_rec"][2, PLANT_REC["N_SAT"]] == 0 and r["plant_rec"][3].tolist() == [T, 0, 0, 0, 0, 0, 0, 0]
        assert np.array_equal(st[3, CMD], A["rb"][3, JERK]) and np.array_equal(st[3, ACT], st[3, CMD])      # (the identity row: the state holds the commands)
    # the log and the tracking record describe the PLAN: stage 0 of the log row is taken from traj, not from the robot record
    assert np.array_equal(r["traj_hist"][:, :, -4:], r["hist"][:, :, ROLL["NVALID"]:ROLL["NVALID"] + 4])


@pytest.mark.parametrize("n,s,nw", [(1, 2, 1), (10, 4, 4)])
def test_the_smallest_horizon_and_the_reference_shape(n, s, nw):
    """(1, 2) on one wave and (10, 4) on teams, three streams, three ticks, disturbances, no queue and no settings table: gain / LAG with DELAY / a clip"""
    A0, Tab, _ = er.start(n, s, nw)
    tab = bstream.plant_table(3, gain=[[0.8] * 7, [NAN] * 7, [NAN] * 7], lag=[NAN, 0.5, NAN], delay=[NAN, 1.0, NAN], sat=[NAN, NAN, 0.05])
    r = er.assert_equals_the_loop(n, s, A0, Tab, None, 3, f"({n}, {s})", plant=tab, state0=_state0(A0), nw=nw, stages=n, disturb=er.disturbances(3, 3, on=(1,)))[0]
    assert r["legs_done"] is None and (r["plant_rec"][:, PLANT_REC["SAMPLES"]] == r["ticks_run"]).all() and (r["plant_rec"][:, PLANT_REC["MAX_DU"]] > 0).all()


# ---- 3. identity ----
@pytest.mark.parametrize("nw", [1, 4])
def test_no_table_a_table_of_nan_and_the_identity_table_are_the_sweeps_entry(nw):
    A0, Tab, _ = er.start(N, S, nw, B)
    Q, ev = _queue(), _events()
    A, Tb, R = _copy(A0), Tab.copy(), Q.copy()
    want = er.rollout(N, S, H, Tb, A, T, entry=5, tune=er.table(), nw=nw, replan=R, accept_capped=True, log_stages=N, **ev)
    assert want["ran"] == 5
    ident = np.tile(bstream.plant_identity(), (B, 1))
    assert np.array_equal(ident, np.stack([er.plant_check(np.full(PLANT["LEN"], NAN))[1]] * B)) and np.isinf(ident[:, PLANT["SAT"]]).all()
    for tab, ran in ((None, 5), (np.full((B, PLANT["LEN"]), NAN), 6), (ident, 6)):
        C, Tc, Rc, st = _copy(A0), Tab.copy(), Q.copy(), _state0(A0)
        st[:] += 3.0      # (whatever the state holds: an identity plant overwrites it and reads none of it)
        before = st.copy()
        r = er.rollout(N, S, H, Tc, C, T, entry=6, plant=tab, plant_state=st, nw=nw, tune=er.table(), replan=Rc, accept_capped=True, log_stages=N, **ev)
        assert r["ran"] == ran
        for k in er.TICK_ARRAYS:
            assert np.array_equal(A[k], C[k], equal_nan=True), k
        assert np.array_equal(Tb, Tc) and np.array_equal(R, Rc)
        for k in er.OUTPUTS + ("ticks_run", "replan_info", "legs_done", "leg_fired", "leg_why", "tune_info", "tune_used"):
            assert np.array_equal(want[k], r[k], equal_nan=True), k
        if tab is None:      # without a table no plant argument is looked at
            assert (r["plant_info"] == -7).all() and (r["plant_rec"] == -7.0).all() and np.array_equal(st, before)
        else:                # with one the state holds the commands: the jerk the last post stored, which a later disturbance or re-plan does not touch
            assert (r["plant_info"] == 0).all() and np.array_equal(r["plant_rec"], np.tile([T, 0, 0, 0, 0, 0, 0, 0], (B, 1)).astype(float))
            assert np.array_equal(st[:, CMD], r["hist"][T - 1][:, JERK]) and np.array_equal(st[:, ACT], st[:, CMD]) and np.array_equal(st[:, 14:], before[:, 14:])


# ---- 4. truth is what is measured ----
@pytest.mark.parametrize("nw", [1, 4])
def test_the_audit_measures_the_true_plant(nw):
    """no events: the p of tick t + 1 starts from the robot record of hist[t] -- the plant behind the drive --, and its tube row is the numpy row of that p
    (the tolerance of tests/test_stream_tube.py for that mirror); the ex_pos series of the gain stream is not the plain run's"""
    from tests.test_stream_tube import ATOL
    A0, Tab, _ = er.start(N, S, nw, B)
    tab = _tables(nw, events=False)["lin"]
    r, A, _, _, _ = er.assert_equals_the_loop(N, S, A0, Tab, None, T, f"no events, nw {nw}", plant=tab, state0=_state0(A0), nw=nw, stages=1)
    plain = _plain(nw, events=False)[0]
    o = bstream._poff(S)
    for b in range(B):
        Ab, Tl, sl = er.unstack(A0, b), Tab[b].copy(), _state0(A0)[b]
        loop = er.contract_loop(N, S, H, Tl, Ab, T, plant_row=tab[b], plant_state=sl, nw=nw, opts=er.opts(N))
        for t in range(T - 1):
            rec, p = r["hist"][t, b], loop["p_hist"][t + 1]
            assert np.array_equal(p[o["q0"]:o["q0"] + 21], rec[RB["Q"]:RB["Q"] + 21]) and np.array_equal(p[o["p0"]:o["p0"] + 12], rec[RB["P"]:RB["P"] + 12])
            assert np.array_equal(p[o["jerk"]:o["jerk"] + 7], rec[JERK])      # (the jerk the drive delivered is where the next ramp starts)
        dev = et.deviations(r["tube_hist"][1:, b], et.numpy_rows(loop["p_hist"][1:], S))
        assert max(dev.values()) <= ATOL, dev
    assert not np.array_equal(r["tube_hist"][:, 0, TUBE["EX_POS"]], plain["tube_hist"][:, 0, TUBE["EX_POS"]])
    assert np.array_equal(r["tube_hist"][0], plain["tube_hist"][0])      # (tick 0 starts from the same state)
    assert not np.array_equal(r["audit"][0], plain["audit"][0])


# ---- 5. mirror and record ----
def test_one_step_against_the_python_mirror():
    """stream.plant_robot at rtol 1e-12 (the project's figure for track_of_rows), the choices exact; a step with every D = 0 keeps every bit"""
    A0, _, _ = er.start(N, S, 1, B)
    rng = np.random.default_rng(7)
    rows = [bstream.plant_table(1, gain=0.8)[0], bstream.plant_table(1, bias=rng.normal(size=7) * 0.1, lag=0.5)[0], bstream.plant_table(1, delay=1.0, sat=0.03)[0],
            bstream.plant_table(1, gain=rng.uniform(0.5, 1.5, 7), bias=0.01, lag=0.25, sat=0.06, delay=1)[0], np.full(PLANT["LEN"], NAN), bstream.plant_identity()]
    for k, row in enumerate(rows):
        for b in range(B):
            rb, ss = A0["rb"][b], A0["ss"][b]
            st = np.zeros(PLANT_STATE["LEN"]); st[:14] = rng.normal(size=14) * 0.1
            code, got_rb, got_st, rec = er.stream_plant(N, H, rb, ss, row, st, er.fresh_rec(), tick=4)
            want_rb, want_st, D, clipped = bstream.plant_robot(rb, row, st, H)
            assert code == 0
            np.testing.assert_allclose(got_rb, want_rb, rtol=1e-12, atol=0.0)
            np.testing.assert_allclose(got_st, want_st, rtol=1e-12, atol=0.0)
            assert rec[PLANT_REC["SAMPLES"]] == 1 and rec[PLANT_REC["N_SAT"]] == float(clipped) and rec[PLANT_REC["TICK_DU"]] == 4
            assert rec[PLANT_REC["JOINT_DU"]] == int(np.argmax(np.abs(D))) and (rec[6:] == 0).all()
            np.testing.assert_allclose([rec[PLANT_REC["MAX_DU"]], rec[PLANT_REC["SUMSQ_DU"]]], [np.abs(D).max(), (D * D).sum()], rtol=1e-12)
            if k >= 4:
                assert np.array_equal(got_rb, rb) and np.array_equal(got_st[CMD], rb[JERK]) and np.array_equal(got_st[ACT], rb[JERK]) and not clipped
            else:
                assert not np.array_equal(got_rb, rb) and np.array_equal(got_rb[RB["XPHID"]:RB["XPHID"] + 3], rb[RB["XPHID"]:RB["XPHID"] + 3])
    # a stream without a plan is skipped, an invalid row answers its mask: nothing is touched
    lost = A0["ss"][0].copy(); lost[SS["ERRCNT"]] = N
    bad = rows[0].copy(); bad[PLANT["LAG"]] = 0.0
    for ss, row, want in ((lost, rows[0], -1), (A0["ss"][0], bad, 1 << PLANT["LAG"])):
        st, rec = np.arange(16.0), er.fresh_rec()
        code, rb, st2, rec2 = er.stream_plant(N, H, A0["rb"][0], ss, row, st, rec)
        assert code == want and np.array_equal(rb, A0["rb"][0]) and np.array_equal(st2, st) and np.array_equal(rec2, rec, equal_nan=True)
    # non-finite words give non-finite records, never a fault; the maximum is NaN for good
    st = _state0(A0)[0]; st[PLANT_STATE["ACT"] + 2] = NAN
    code, rb, st2, rec = er.stream_plant(N, H, A0["rb"][0], A0["ss"][0], rows[1], st, er.fresh_rec(), tick=1)
    assert code == 0 and np.isnan(rb[RB["Q"] + 2]) and np.isnan(rb[RB["P"]:RB["P"] + 6]).all() and np.isnan(rec[PLANT_REC["MAX_DU"]]) and rec[PLANT_REC["N_SAT"]] == 0
    code, rb, st2, rec = er.stream_plant(N, H, A0["rb"][0], A0["ss"][0], rows[0], _state0(A0)[0], rec, tick=2)
    assert np.isnan(rec[PLANT_REC["MAX_DU"]]) and rec[PLANT_REC["TICK_DU"]] == 1 and rec[PLANT_REC["SAMPLES"]] == 2


@pytest.mark.parametrize("nw", [1, 4])
def test_the_record_is_the_numpy_reduction_of_the_rows(nw):
    """plant_rec over the emulator's own rows: the command of a tick is the first planned jerk, stage 0 of its trajectory record (traj_hist), what the drive
    delivered is the jerk of its history row"""
    A0, Tab, _ = er.start(N, S, nw, B)
    for which, tab in _tables(nw, events=False).items():
        A, Tb, st = _copy(A0), Tab.copy(), _state0(A0)
        r = er.rollout(N, S, H, Tb, A, T, entry=6, plant=tab, plant_state=st, nw=nw, log_stages=1)
        for b in range(B):
            c = r["traj_hist"][:, b, 21 * N:28 * N:N]      # [T][7]: the jerk block [7][N] of a trajectory record sits behind q, dq and ddq; its column 0
            D = r["hist"][:, b, JERK] - c
            rec = r["plant_rec"][b]
            sumsq = 0.0
            for t in range(T):
                for j in range(7):
                    sumsq += D[t, j] * D[t, j]
            t_max, j_max = np.unravel_index(int(np.argmax(np.abs(D))), D.shape)
            assert rec[PLANT_REC["SAMPLES"]] == T and rec[PLANT_REC["SUMSQ_DU"]] == sumsq and rec[PLANT_REC["MAX_DU"]] == np.abs(D).max(), (which, b, rec)
            assert (rec[PLANT_REC["TICK_DU"]], rec[PLANT_REC["JOINT_DU"]]) == (t_max, j_max) or np.abs(D).max() == 0.0
            sat = tab[b, PLANT["SAT"]]
            if not np.isnan(sat):
                assert rec[PLANT_REC["N_SAT"]] == (np.abs(r["hist"][:, b, JERK]) == sat).any(axis=1).sum()
            u = bstream.unpack_plant_rec(rec)
            assert u["samples"] == T and u["max_du"] == rec[PLANT_REC["MAX_DU"]] and u["tick_du"] == int(rec[PLANT_REC["TICK_DU"]])


EDGE = [NAN, np.inf, -np.inf, -0.0, 0.0, 1.0, 1.0 + 2.0 ** -52, 0.5, 2.0, -1.0, -0.5, 1e-300, 1e308]


def test_the_python_rule_is_the_compiled_rule():
    """every slot on the edge values, one slot at a time: NaN, +-inf, -0.0, 0, 1, 1 + 2^-52, 0.5, 2, negative SAT, DELAY 0.5; the pad words are never looked at"""
    for k in range(PLANT["LEN"]):
        for v in EDGE:
            row = np.full(PLANT["LEN"], NAN); row[k] = v
            bad, used = er.plant_check(row)
            assert bad == bstream.plant_check(row) and bad & ~(1 << k) == 0, (k, v, bad)
            want = bstream.plant_identity(); want[k] = 0.0 if k >= 17 else (want[k] if np.isnan(v) else v)
            assert np.array_equal(used, want), (k, v, used)
    ok = lambda k: [v for v in EDGE[1:] if not bstream.plant_check(np.where(np.arange(PLANT["LEN"]) == k, v, NAN))]
    finite = [-0.0, 0.0, 1.0, 1.0 + 2.0 ** -52, 0.5, 2.0, -1.0, -0.5, 1e-300, 1e308]
    assert ok(PLANT["GAIN"]) == finite and ok(PLANT["BIAS"] + 6) == finite
    assert ok(PLANT["LAG"]) == [1.0, 0.5, 1e-300] and ok(PLANT["SAT"]) == [np.inf, 1.0, 1.0 + 2.0 ** -52, 0.5, 2.0, 1e-300, 1e308] and ok(PLANT["DELAY"]) == [-0.0, 0.0, 1.0]
    assert ok(17) == EDGE[1:] and ok(19) == EDGE[1:]
    for kw in (dict(gain=np.inf), dict(bias=[0.0] * 6 + [-np.inf]), dict(lag=0.0), dict(lag=[0.5, 1.5]), dict(sat=-1.0), dict(sat=0.0), dict(delay=0.5)):
        with pytest.raises(ValueError, match="plant row"):
            bstream.plant_table(2, **kw)


# ---- 6. invalid rows ----
@pytest.mark.parametrize("nw", [1, 4])
def test_invalid_rows_do_not_run_and_their_neighbours_do(nw):
    """rows 0 and 2 invalid (LAG 0 with an infinite gain; DELAY 0.5), rows 1 and 3 of the LIN table"""
    A0, Tab, _ = er.start(N, S, nw, B)
    Q, ev, tab = _queue(), _events(), _tables(nw)["lin"]
    bad = tab.copy()
    bad[0, PLANT["LAG"]], bad[0, PLANT["GAIN"] + 5] = 0.0, np.inf
    bad[2] = NAN; bad[2, PLANT["DELAY"]] = 0.5
    A, Tb, R, st = _copy(A0), Tab.copy(), Q.copy(), _state0(A0) + 1.5
    for k in ("x", "g", "kkt", "p", "x0"):
        A[k][[0, 2]] = 7.25      # (what the memory held: it stays)
    A["iters"][[0, 2]], A["status"][[0, 2]] = 77, 9
    before, st_before = _copy(A), st.copy()
    r = er.rollout(N, S, H, Tb, A, T, entry=6, plant=bad, plant_state=st, nw=nw, tune=er.table(), replan=R, accept_capped=True, log_stages=N, **ev)
    assert r["plant_info"].tolist() == [1 << PLANT["LAG"] | 1 << PLANT["GAIN"] + 5, 0, 1 << PLANT["DELAY"], 0] and r["ticks_run"].tolist() == [0, T, 0, T]
    assert r["tune_info"].tolist() == [0] * B
    for b in (0, 2):
        er.assert_arrays_equal(er.unstack(before, b), er.unstack(A, b), f"invalid row, stream {b}")
        assert np.array_equal(Tb[b], Tab[b]) and np.array_equal(R[b], Q[b]) and (R[b, :, RP["FLAG"]] == 1.0).all() and np.array_equal(st[b], st_before[b])
        assert all(np.isnan(r[k][:, b]).all() for k in ("hist", "traj_hist", "tube_hist", "log_hist"))
        assert r["legs_done"][b] == 0 and (r["leg_fired"][b] == -1).all() and (r["leg_why"][b] == 0).all() and (r["replan_info"][b] == -1).all()
        assert np.array_equal(r["plant_rec"][b], er.fresh_rec()) and r["plant_rec"][b].tolist() == [0, 0, -np.inf, -1, -1, 0, 0, 0]
    # ... their audit and tracking records are those of a stream lost on entry
    L, Tl = _copy(A0), Tab.copy()
    L["ss"][:, SS["ERRCNT"]] = N
    lost = er.rollout(N, S, H, Tl, L, T, entry=6, plant=tab, plant_state=_state0(A0), nw=nw, tune=er.table(), replan=Q.copy(), log_stages=N, **ev)
    assert lost["ticks_run"].tolist() == [0] * B and np.array_equal(lost["plant_rec"], np.tile(er.fresh_rec(), (B, 1)))
    for b in (0, 2):
        assert np.array_equal(r["audit"][b], lost["audit"][b], equal_nan=True) and np.array_equal(r["track"][b], lost["track"][b], equal_nan=True)
    # the neighbours: bit-equal to a run without the invalid rows
    C, Tc, Rc, sc = _copy(A0), Tab.copy(), Q.copy(), _state0(A0) + 1.5
    good = er.rollout(N, S, H, Tc, C, T, entry=6, plant=tab, plant_state=sc, nw=nw, tune=er.table(), replan=Rc, accept_capped=True, log_stages=N, **ev)
    for b in (1, 3):
        er.assert_arrays_equal(er.unstack(C, b), er.unstack(A, b), f"neighbour {b}")
        er.assert_streams_equal(er.stream_of(r, b), er.stream_of(good, b), f"neighbour {b}")
        assert np.array_equal(Tb[b], Tc[b]) and np.array_equal(R[b], Rc[b]) and np.array_equal(st[b], sc[b]) and np.array_equal(r["plant_rec"][b], good["plant_rec"][b])


# ---- 7. a plan exhausted mid-run ----
@pytest.mark.parametrize("nw,wave_order", [(1, 0), (4, 1)])
def test_the_tick_whose_post_exhausts_the_plan_takes_no_plant_step(nw, wave_order):
    """the events' rescue scenario (tests/test_stream_rollout_legs.py): one-iteration ticks on plants a push has carried off their paths -- tick 0 fails and
    replays, the post of tick 1 exhausts the plan and returns early.  Stream 0 is rescued by its ON_LOST record and runs on, stream 1 stops, stream 2 never
    runs"""
    from tests.test_stream_rollout_legs import _rescue_case
    A0, Tab, Q, lt, lo = _rescue_case(N, S, nw)
    tab = bstream.plant_table(3, gain=0.8, lag=0.5)
    r, A, Tb, R, st = er.assert_equals_the_loop(N, S, A0, Tab, Q, T, f"rescue, nw {nw}", plant=tab, state0=_state0(A0), nw=nw, wave_order=wave_order, leg_tick=lt, leg_on=lo, max_iter=1)
    assert r["ticks_run"][0] > 2 and r["ticks_run"].tolist()[1:] == [2, 0] and (r["hist"][1, :2, ROLL["ERRCNT"]] == N).all() and r["leg_fired"][0, 0] == 1
    stepped = (r["hist"][:, :, ROLL["ERRCNT"]] < N).sum(axis=0)      # (NaN rows compare False)
    assert r["plant_rec"][:, PLANT_REC["SAMPLES"]].tolist() == stepped.tolist() and stepped[1] == 1 and 1 <= stepped[0] < r["ticks_run"][0]
    # the same launch cut behind tick 0: the record of stream 1, its plant state (CMD and ACT) and its robot record are those -- tick 1 changed no bit of them
    C, Tc, Rc, sc = _copy(A0), Tab.copy(), Q.copy(), _state0(A0)
    one = er.rollout(N, S, H, Tc, C, 1, entry=6, plant=tab, plant_state=sc, nw=nw, wave_order=wave_order, replan=Rc, leg_tick=lt, leg_on=lo, max_iter=1)
    assert np.array_equal(one["plant_rec"][1], r["plant_rec"][1]) and np.array_equal(sc[1], st[1]) and np.array_equal(C["rb"][1], A["rb"][1])
    assert np.array_equal(r["hist"][1, 1, :RB["LEN"]], r["hist"][0, 1, :RB["LEN"]]) and r["plant_rec"][2].tolist() == er.fresh_rec().tolist()


# ---- 8. chaining ----
@pytest.mark.parametrize("nw", [1, 4])
def test_one_rollout_of_six_ticks_is_two_of_three_that_hand_over_the_state(nw):
    """LAG and DELAY rows make the state matter: with a fresh state in the second half the histories differ"""
    A0, Tab, _ = er.start(N, S, nw, B)
    tab = bstream.plant_table(B, lag=[0.5, NAN, 0.25, NAN], delay=[NAN, 1.0, 1.0, NAN], gain=0.9)
    d = er.disturbances(T, B, on=(1, 4))
    A, Tb, st = _copy(A0), Tab.copy(), _state0(A0)
    whole = er.rollout(N, S, H, Tb, A, T, entry=6, plant=tab, plant_state=st, nw=nw, disturb=d, log_stages=N)
    C, Tc, sc = _copy(A0), Tab.copy(), _state0(A0)
    first = er.rollout(N, S, H, Tc, C, 3, entry=6, plant=tab, plant_state=sc, nw=nw, disturb=np.ascontiguousarray(d[:3]), log_stages=N)
    second = er.rollout(N, S, H, Tc, C, 3, entry=6, plant=tab, plant_state=sc, nw=nw, disturb=np.ascontiguousarray(d[3:]), log_stages=N)
    assert whole["ticks_run"].tolist() == [T] * B and first["ticks_run"].tolist() == [3] * B
    for b in range(B):
        er.assert_arrays_equal(er.unstack(A, b), er.unstack(C, b), f"chained, stream {b}")
    assert np.array_equal(st, sc)
    for k in ("hist", "traj_hist", "tube_hist", "log_hist"):
        assert np.array_equal(whole[k], np.concatenate([first[k], second[k]]), equal_nan=True), k
    assert np.array_equal(whole["plant_rec"][:, PLANT_REC["SUMSQ_DU"]] > 0, [True] * B) and (first["plant_rec"][:, 0] + second["plant_rec"][:, 0] == T).all()
    # a second half that starts from a zeroed state is another run: the state matters (ACT to the LAG rows, CMD to the DELAY rows; row 3, a gain alone, has no memory)
    E, Te, se = _copy(A0), Tab.copy(), _state0(A0)
    er.rollout(N, S, H, Te, E, 3, entry=6, plant=tab, plant_state=se, nw=nw, disturb=np.ascontiguousarray(d[:3]), log_stages=N)
    fresh = er.rollout(N, S, H, Te, E, 3, entry=6, plant=tab, plant_state=np.zeros_like(sc), nw=nw, disturb=np.ascontiguousarray(d[3:]), log_stages=N)
    same = [np.array_equal(fresh["hist"][:, b], second["hist"][:, b]) for b in range(B)]
    assert same == [False, False, False, True], same


# ---- 9. housekeeping ----
def test_argument_errors_of_the_entry():
    """plant without plant_state, and what the sweeps entry refuses, with a plant table; the plant's outputs may be NULL"""
    A0, Tab, _ = er.start(N, S, 1, B)
    Q, tab = _queue(), _tables(1)["lin"]
    lt, lo = np.ones((B, 2), dtype=np.int32), np.zeros((B, 2), dtype=np.int32)
    ok = dict(replan=Q, leg_tick=lt, leg_on=lo, tune=er.table())
    for kw in (dict(ok, state=None), dict(state=None), dict(ok, leg_tick=None), dict(ok, leg_on=None), dict(ok, update_flags=8), dict(ok, ticks=0), dict(ok, simulate=False),
               dict(ok, goal_tol=-1.0), dict(goal_tol=NAN), dict(ok, audit_tol=-1.0), dict(audit_tol=np.inf), dict(ok, log_stages=N + 1)):
        A, Tb = _copy(A0), Tab.copy()
        kw = dict(kw); kw["replan"] = None if kw.get("replan") is None else Q.copy()
        st = kw.pop("state", _state0(A0))
        assert er.rollout(N, S, H, Tb, A, kw.pop("ticks", 2), entry=6, plant=tab, plant_state=st, want_rc=True, **kw) == 1, {k: v for k, v in kw.items() if k != "replan"}
        for b in range(B):
            er.assert_arrays_equal(er.unstack(A0, b), er.unstack(A, b), "nothing runs")
    assert er.rollout(N, S, H, Tab.copy(), _copy(A0), 2, entry=6, plant=tab, plant_state=_state0(A0), want_rc=True, want_plant_info=False, want_rec=False, **dict(ok, replan=Q.copy())) == 0
    assert er.rollout(N, S, H, Tab.copy(), _copy(A0), 2, entry=6, plant=None, plant_state=None, want_rc=True, **dict(ok, replan=Q.copy())) == 0      # (no table: no state needed)


def test_the_python_surface():
    here = os.path.dirname(os.path.abspath(__file__))
    header = open(os.path.join(here, "..", "include", "boundmpc_hip.h")).read()

    def enum_of(first):
        body = re.search(r"enum \{ (%s = 0,.*?) \};" % first, header, re.S).group(1)
        out, nxt = {}, 0
        for w in body.replace("\n", " ").split(","):
            name, _, val = w.strip().partition("=")
            nxt = int(val) if val.strip() else nxt
            out[name.strip()] = nxt
            nxt += 1
        return out
    row, st, rec = er.plant_slots()
    for first, prefix, d, kernel in (("BMPC_PLANT_GAIN", "BMPC_PLANT_", PLANT, row), ("BMPC_PLANT_STATE_ACT", "BMPC_PLANT_STATE_", PLANT_STATE, st),
                                     ("BMPC_PLANT_REC_SAMPLES", "BMPC_PLANT_REC_", PLANT_REC, rec)):
        e = {k[len(prefix):]: v for k, v in enum_of(first).items()}
        assert e == d and [v for k, v in sorted(d.items(), key=lambda kv: kv[1]) if k != "LEN"] == kernel, (prefix, e, d, kernel)
    assert (PLANT["LEN"], PLANT_STATE["LEN"], PLANT_REC["LEN"]) == (20, 16, 8)
    from boundmpc_amd import _lib
    import boundmpc_amd
    syms = ("bmpc_stream_plant_len", "bmpc_stream_plant_state_len", "bmpc_stream_plant_rec_len", "bmpc_stream_rollout_plant", "bmpc_stream_plant")
    for sym in syms:
        assert sym in _lib.SIGNATURES and re.search(r"\b%s\(" % sym, header)
    assert len(_lib.SIGNATURES["bmpc_stream_rollout_plant"][1]) == len(_lib.SIGNATURES["bmpc_stream_rollout_tuned"][1]) + 4 and len(_lib.SIGNATURES["bmpc_stream_plant"][1]) == 10
    if os.path.exists(_lib.LIB_PATH):      # (a built tree: the symbols are exported; loading the library needs no GPU)
        L = ctypes.CDLL(_lib.LIB_PATH)
        assert all(hasattr(L, sym) for sym in syms) and (L.bmpc_stream_plant_len(), L.bmpc_stream_plant_state_len(), L.bmpc_stream_plant_rec_len()) == (20, 16, 8)
    assert {"plant", "want_plant_rec"} <= set(inspect.signature(bstream.StreamBatch.rollout).parameters) and hasattr(bstream.StreamBatch, "plant_step") and hasattr(bstream.StreamBatch, "plant_reset")
    for name in ("PLANT", "PLANT_STATE", "PLANT_REC", "plant_table", "plant_check", "plant_state_of", "plant_robot", "unpack_plant_rec"):
        assert getattr(boundmpc_amd, name) is getattr(bstream, name)
    # the docstring and the header say in as many words that the log and the tracking record keep describing the plan
    assert "log_hist and track keep describing the PLAN" in bstream.StreamBatch.rollout.__doc__ and "KEEP DESCRIBING THE PLAN, NOT THE PLANT" in header
    # plant_table: scalars, [7] and [B][7] broadcast, NaN elsewhere; plant_state_of
    t = bstream.plant_table(3, gain=0.9, bias=np.arange(7.0), lag=[0.5, NAN, 1.0], sat=2.0)
    assert t.shape == (3, 20) and (t[:, :7] == 0.9).all() and (t[:, 7:14] == np.arange(7.0)).all() and t[0, 14] == 0.5 and np.isnan(t[1, 14]) and (t[:, 15] == 2.0).all()
    assert np.isnan(t[:, 16:]).all() and np.isnan(bstream.plant_table(2)).all()
    with pytest.raises(ValueError, match="must be a scalar"):
        bstream.plant_table(2, gain=[1.0] * 3)
    rb = np.arange(2 * RB["LEN"], dtype=float).reshape(2, -1)
    s0 = bstream.plant_state_of(rb)
    assert s0.shape == (2, 16) and np.array_equal(s0[:, ACT], rb[:, JERK]) and np.array_equal(s0[:, CMD], rb[:, JERK]) and (s0[:, 14:] == 0).all()
    assert bstream.plant_state_of(rb[0]).shape == (16,)


def sanitizer_cases(nw):
    A0, Tab, _ = er.start(N, S, nw, B)
    tab = bstream.plant_table(B, gain=[[0.8] * 7, [NAN] * 7, [NAN] * 7, [NAN] * 7], lag=[NAN, 0.5, NAN, NAN], delay=[NAN, 1.0, NAN, NAN], sat=[NAN, NAN, 0.1, NAN])
    bad = tab.copy(); bad[0, PLANT["SAT"]] = -1.0
    st = _state0(A0)
    return [("table", dict(N=N, S=S, h=H, T=Tab, A=A0, ticks=3, plant=tab, plant_state=st, disturb=er.disturbances(3, B, on=(1,)))),
            ("refused", dict(N=N, S=S, h=H, T=Tab, A=A0, ticks=3, plant=bad, plant_state=st))]


@pytest.mark.parametrize("nw", [1, 4])
def test_the_plant_text_is_clean_under_the_sanitizers(nw):
    """the host program with its own main, built with -fsanitize=address,undefined on exact-size buffers and run as a child process (nothing is loaded
    into this interpreter); on teams under both wave orders"""
    out = er.run_sanitized(sanitizer_cases(nw), nw)
    print("\n".join(out))
    assert len(out) == 2 and all("rc 0 ran 6" in line and "DIFFERS" not in line for line in out)
    assert "[stream 0 ticks_run 3 plant_info 0 samples 3 n_sat 0]" in out[0] and "[stream 2 ticks_run 3 plant_info 0 samples 3 n_sat" in out[0]
    assert "[stream 0 ticks_run 0 plant_info %d samples 0 n_sat 0]" % (1 << PLANT["SAT"]) in out[1] and "[stream 1 ticks_run 3 plant_info 0 samples 3" in out[1]
