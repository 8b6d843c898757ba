"""Sensors inside a rollout -- a table of measurement models per stream between the true plant and what the pack, the solve and the post of a tick read,
validated on the device -- as device code compiled for the CPU (csrc/bmpc_rollout_body.inl with SE, csrc/bmpc_stream_sensor.inl;
tests/emu/bmpc_emu_rollout_sensor.cpp, once for one wave per stream and once for teams of four).  The checker is the contract: the entry against the
per-tick loop {sense text, tick text, unsense text, plant step text, tube text, log text, disturb text, update text of the head record due} for one stream
(emu_rollout_sensor.contract_loop), bit for bit.  (10, 4), B = 4 streams of emu_rollout.small_stream behind a solved-out tick 0, T = 6; (1, 2) once; the
tick whose post exhausts the plan on the missions' rescue scenario, which is built at (2, 2).
Four tables of four rows: BN = offsets and noise, RES = a 16-bit encoder step with offsets, HOLD = a stale sample with noise, NAN = all NaN."""
import ctypes
import functools
import inspect
import os
import re

import numpy as np
import pytest

from boundmpc_amd import stream as bstream
from tests.emu import emu_rollout as er, emu_rollout_sensor as es

SENSOR, SENSOR_STATE, SENSOR_REC, ROLL, RB, RP, SS, PLANT = bstream.SENSOR, bstream.SENSOR_STATE, bstream.SENSOR_REC, bstream.ROLL, bstream.RB, bstream.RP, bstream.SS, bstream.PLANT
N, S, T, B = 10, 4, 6, 4
H = er.H
NAN = float("nan")
_copy = er.copy_arrays
Q21 = slice(0, 21)
JERK = slice(RB["JERK"], RB["JERK"] + 7)
TRUTH = slice(SENSOR_STATE["TRUTH"], SENSOR_STATE["TRUTH"] + 40)
BUILDS = [(1, 0, 0), (1, 0, 1), (4, 0, 0), (4, 1, 1)]      # (waves, wave order, lane order)
RES16 = 2.0 * np.pi / 2.0 ** 16
TIE_MARGIN = 1e-6


def _queue(K=2):
    """[B][K][len]: a leg back, then a leg back with a detour, per stream"""
    kinds = [er.small_batch(N, S, B)[3], er.small_batch(N, S, B, detour=0.05)[3]]
    return np.ascontiguousarray(np.stack([kinds[k % 2] for k in range(K)], axis=1))


def _events():
    """a two-record queue (record 0 behind tick 1 or 2, record 1 behind tick 4) and disturbances on ticks 1 and 4: the sweeps' events"""
    lt = np.array([[1, 4], [2, 4], [1, 4], [2, 4]], dtype=np.int32)
    return dict(leg_tick=lt, leg_on=np.zeros((B, 2), dtype=np.int32), disturb=er.disturbances(T, B, on=(1, 4)))


def _plant():
    return bstream.plant_table(B, gain=[[0.9] * 7, [NAN] * 7, [NAN] * 7, [NAN] * 7], lag=[NAN, 0.5, NAN, NAN], delay=[NAN, NAN, 1.0, NAN])


def _tables():
    rng = np.random.default_rng(23)
    one = np.zeros(7); one[3] = 2e-3
    bn = bstream.sensor_table(B, bias=[[1e-3] * 7, one, [NAN] * 7, [NAN] * 7], nq=[1e-4, NAN, 1e-4, NAN], ndq=[NAN, NAN, 1e-3, NAN], nddq=[NAN, NAN, 1e-2, NAN])
    res = bstream.sensor_table(B, bias=np.vstack([rng.uniform(-1e-3, 1e-3, (3, 7)), np.zeros((1, 7))]), res=RES16)
    hold = bstream.sensor_table(B, hold=[1.0, 1.0, 1.0, NAN], nq=[1e-4, NAN, 1e-4, NAN], bias=[[NAN] * 7, [NAN] * 7, [5e-4] * 7, [NAN] * 7])
    nan = bstream.sensor_table(B)
    assert np.isnan(bn[3]).all() and np.isnan(hold[3]).all() and np.isnan(nan).all() and (res[:, SENSOR["RES"]] == RES16).all()
    return dict(bn=bn, res=res, hold=hold, nan=nan)


def _noise(which):
    return None if which in ("res", "nan") else es.noise(T, B)


def _identity_row(row):
    return bool((np.nan_to_num(row[:12], nan=0.0) == 0.0).all())


@functools.lru_cache(maxsize=None)
def _plain(nw, events=True, ticks=T):
    """the run of the plants' text WITHOUT a sensor table on the inputs of the contract test (events: the queue, the disturbances, the sweeps' table and the plant
    table; else none of them): (result, arrays, plant state).  Shared, never written."""
    A0, Tab, _ = er.start(N, S, nw, B)
    A, Tb, st = _copy(A0), Tab.copy(), bstream.plant_state_of(A0["rb"])
    kw = dict(tune=er.table(), replan=_queue(), accept_capped=True, plant=_plant(), plant_state=st, **_events()) if events else {}
    if events and ticks != T:
        kw["disturb"] = np.ascontiguousarray(kw["disturb"][:ticks])
    r = er.rollout(N, S, H, Tb, A, ticks, entry=6, nw=nw, log_stages=N, **kw)
    assert r["ran"] == (6 if events else 3)
    return r, A, st


# ---- 1., 2. the contract; an ignored table or a skipped truth step cannot pass ----
@pytest.mark.parametrize("which", ["bn", "res", "hold", "nan"])
@pytest.mark.parametrize("nw,wave_order,lane_order", BUILDS)
def test_a_rollout_with_sensors_equals_the_per_tick_loop(nw, wave_order, lane_order, which):
    """events, audit, log, tracking record, a two-record queue, the sweeps' table and a plant table on: every tick array, history array (meas_hist among them),
    record, queue output, plant_state, plant_rec, sensor_state and sensor_rec of every stream against contract_loop.  Every non-identity row changes the p of
    tick 1 and the history of its stream against the run without a sensor, an identity row changes neither.  RES: every m_q / RES of the run lies at least 1e-6
    from a rounding tie, no sample omitted (what makes the comparisons of separately compiled builds at a tolerance safe: one ulp ahead of rint flips no step)."""
    A0, Tab, _ = er.start(N, S, nw, B)
    tab, nz, ev = _tables()[which], _noise(which), _events()
    r, A, Tb, R, pst, sst, loops = es.assert_equals_the_loop(N, S, A0, Tab, _queue(), T, tab, f"{which}, nw {nw} orders {wave_order} {lane_order}", sensor_noise=nz, plant=_plant(),
                                                             pstate0=bstream.plant_state_of(A0["rb"]), nw=nw, wave_order=wave_order, lane_order=lane_order, stages=N, tune=er.table(),
                                                             accept_capped=True, **ev)
    assert r["sensor_info"].tolist() == [0] * B and (r["sensor_rec"][:, SENSOR_REC["SAMPLES"]] == r["ticks_run"]).all() and (r["ticks_run"] >= 2).all()
    plain = _plain(nw)[0]
    # the p of tick 1: the same launch cut behind tick 1 leaves it in the tick arrays
    C, D = _copy(A0), _copy(A0)
    es.rollout(N, S, H, Tab.copy(), C, 2, nw=nw, sensor=tab, sensor_state=np.zeros((B, 64)), sensor_noise=None if nz is None else np.ascontiguousarray(nz[:2]), replan=_queue(),
               tune=er.table(), plant=_plant(), plant_state=bstream.plant_state_of(A0["rb"]), accept_capped=True, log_stages=N, leg_tick=ev["leg_tick"], leg_on=ev["leg_on"],
               disturb=np.ascontiguousarray(ev["disturb"][:2]))
    D = _plain(nw, True, 2)[1]
    for b in range(B):
        same_h, same_p = np.array_equal(r["hist"][:, b], plain["hist"][:, b], equal_nan=True), np.array_equal(C["p"][b], D["p"][b])
        assert same_h == same_p == _identity_row(tab[b]), f"row {b} of {which}: hist {'un' * same_h}changed, p of tick 1 {'un' * same_p}changed"
        # hist is the TRUTH and meas_hist the sample: where the row is no identity they differ on some tick, and the truth ahead of a tick is the history row behind the one before
        if not _identity_row(tab[b]):
            assert not np.array_equal(r["meas_hist"][1:, b, Q21], loops[b]["truth_hist"][1:, Q21])
        else:
            assert np.array_equal(r["meas_hist"][:, b], loops[b]["truth_hist"], equal_nan=True) and r["sensor_rec"][b, SENSOR_REC["MAX_DQ"]] == 0.0
    if which == "res":
        worst = 1.0
        for b in range(B):
            n = int(r["ticks_run"][b])
            m = (loops[b]["truth_hist"][:n, :7] + tab[b, :7]) / RES16
            worst = min(worst, float(np.abs(np.abs(m - np.floor(m)) - 0.5).min()))
            assert np.array_equal(r["meas_hist"][:n, b, :7], RES16 * np.rint(m))      # (and every sample sits on the grid)
        print(f"RES: nearest rounding tie {worst:.3e} steps away")
        assert worst >= TIE_MARGIN
    if which == "nan":
        assert np.array_equal(sst[:, SENSOR_STATE["SAME"]], np.ones(B)) and np.array_equal(pst, _plain(nw)[2])
        for k in er.TICK_ARRAYS:
            assert np.array_equal(A[k], _plain(nw)[1][k], equal_nan=True), k


def test_the_smallest_horizon():
    """(1, 2) on one wave, three streams, three ticks, disturbances, no queue, no settings table and no plant table: offsets / a step with noise / HOLD"""
    A0, Tab, _ = er.start(1, 2, 1)
    tab = bstream.sensor_table(3, bias=[[1e-3] * 7, [NAN] * 7, [NAN] * 7], res=[NAN, 1e-3, NAN], nq=[NAN, 1e-4, NAN], hold=[NAN, NAN, 1.0])
    r = es.assert_equals_the_loop(1, 2, A0, Tab, None, 3, tab, "(1, 2)", sensor_noise=es.noise(3, 3), stages=1, disturb=er.disturbances(3, 3, on=(1,)))[0]
    assert r["legs_done"] is None and r["plant_info"] is None and (r["sensor_rec"][:, SENSOR_REC["SAMPLES"]] == r["ticks_run"]).all()
    assert (r["sensor_rec"][:, SENSOR_REC["MAX_DQ"]] > 0).all()


# ---- 3. identity ----
@pytest.mark.parametrize("nw", [1, 4])
def test_no_table_a_table_of_nan_and_the_identity_table_are_the_plants_entry(nw):
    A0, Tab, _ = er.start(N, S, nw, B)
    Q, ev = _queue(), _events()
    want, A, pst = _plain(nw)
    ident = np.zeros((B, SENSOR["LEN"]))
    assert np.array_equal(ident, np.stack([es.sensor_check(np.full(SENSOR["LEN"], NAN))[1]] * B))
    for tab, ran in ((None, 6), (np.full((B, SENSOR["LEN"]), NAN), es.RAN_SENSOR), (ident, es.RAN_SENSOR)):
        C, Tc, Rc, pc = _copy(A0), Tab.copy(), Q.copy(), bstream.plant_state_of(A0["rb"])
        st = np.zeros((B, SENSOR_STATE["LEN"])); st[:, :21] = 3.0      # (a held sample that HOLD = 0 never hands out)
        before = st.copy()
        r = es.rollout(N, S, H, Tc, C, T, nw=nw, sensor=tab, sensor_state=st, sensor_noise=es.noise(T, B), plant=_plant(), plant_state=pc, tune=er.table(), replan=Rc,
                       accept_capped=True, log_stages=N, **ev)
        assert r["ran"] == ran
        for k in er.TICK_ARRAYS:
            assert np.array_equal(A[k], C[k], equal_nan=True), k
        assert np.array_equal(pst, pc)
        for k in er.OUTPUTS + ("ticks_run", "replan_info", "legs_done", "leg_fired", "leg_why", "tune_info", "tune_used", "plant_info", "plant_rec"):
            assert np.array_equal(want[k], r[k], equal_nan=True), k
        if tab is None:      # without a table no sensor argument is looked at
            assert (r["sensor_info"] == -7).all() and (r["sensor_rec"] == -7.0).all() and (r["meas_hist"] == -7.0).all() and np.array_equal(st, before)
        else:                # with one the samples are the truth
            assert (r["sensor_info"] == 0).all() and np.array_equal(r["sensor_rec"], np.tile([T, 0, 0, 0, 0, 0, 0, 0], (B, 1)).astype(float))
            assert (st[:, SENSOR_STATE["SAME"]] == 1).all() and (st[:, SENSOR_STATE["HAS"]] == 1).all()
            assert np.array_equal(st[:, :21], r["meas_hist"][T - 1][:, Q21])      # (HELD: the last sample)


# ---- 4. the mirrors ----
def test_one_sample_and_one_way_back_against_the_python_mirror():
    """stream.sense_robot and truth_robot against the g++ steps at 1e-12 (the bound of the plant's one-step test), the choices exact; an identity sample keeps
    every bit, and so does the way back behind it"""
    A0, Tab, _ = er.start(N, S, 1, B)
    rng = np.random.default_rng(7)
    rows = [bstream.sensor_table(1, bias=1e-3)[0], bstream.sensor_table(1, bias=rng.normal(size=7) * 1e-3, nq=1e-4, ndq=1e-3, nddq=1e-2)[0],
            bstream.sensor_table(1, res=1e-3, bias=rng.uniform(-1e-3, 1e-3, 7))[0], bstream.sensor_table(1, hold=1.0, nq=1e-4)[0], np.full(SENSOR["LEN"], NAN), np.zeros(SENSOR["LEN"])]
    for k, row in enumerate(rows):
        for b in range(B):
            rb, ss = A0["rb"][b], A0["ss"][b]
            nz = rng.normal(size=21); nz[5] = np.inf; nz[9] = NAN      # (non-finite draws count as 0)
            st = np.zeros(SENSOR_STATE["LEN"])
            if b % 2:
                st[:21], st[SENSOR_STATE["HAS"]] = rb[:21] + rng.normal(size=21) * 1e-3, 1.0
            code, got_rb, got_st, rec, meas = es.stream_sense(N, rb, ss, row, st, nz, es.fresh_rec(), tick=4)
            want_rb, want_st, d, dp = bstream.sense_robot(rb, row, st, nz)
            assert code == 0 and np.array_equal(meas, got_rb)
            np.testing.assert_allclose(got_rb, want_rb, rtol=1e-12, atol=1e-15)
            np.testing.assert_allclose(got_st, want_st, rtol=1e-12, atol=1e-15)
            assert got_st[SENSOR_STATE["SAME"]] == want_st[SENSOR_STATE["SAME"]] == float(k >= 4) and got_st[SENSOR_STATE["HAS"]] == 1.0
            assert np.array_equal(got_st[TRUTH][:33], rb[:33]) and np.array_equal(got_st[TRUTH][33:], rb[JERK])
            assert np.array_equal(got_rb[RB["XPHID"]:], rb[RB["XPHID"]:])      # (x_phi_d and the jerk are kept)
            assert rec[SENSOR_REC["SAMPLES"]] == 1 and rec[7] == 0
            np.testing.assert_allclose([rec[SENSOR_REC["MAX_DQ"]], rec[SENSOR_REC["SUMSQ_DQ"]], rec[SENSOR_REC["MAX_DP"]]], [np.abs(d[:7]).max(), (d[:7] ** 2).sum(), dp], rtol=1e-9, atol=1e-15)
            if k >= 4:
                assert np.array_equal(got_rb, rb) and rec.tolist() == [1, 0, 4, 0, 0, 4, 0, 0]
            else:
                assert not np.array_equal(got_rb[:21], rb[:21]) and rec[SENSOR_REC["TICK_DQ"]] == 4 and rec[SENSOR_REC["JOINT_DQ"]] == int(np.argmax(np.abs(d[:7])))
            # the way back: behind a post that stepped (the record's jerk is the command), and behind one that did not
            post = got_rb.copy(); post[:33] += rng.normal(size=33) * 1e-3; post[JERK] = rng.normal(size=7)
            for stepped, ssb in ((True, ss), (False, np.where(np.arange(ss.size) == SS["ERRCNT"], float(N), ss))):
                code, back = es.stream_unsense(N, H, post, ssb, row, got_st)
                want = bstream.truth_robot(post, got_st, H, stepped)
                assert code == 0
                np.testing.assert_allclose(back, want, rtol=1e-12, atol=1e-15)
                if k >= 4:
                    assert np.array_equal(back, post)
                elif not stepped:
                    assert np.array_equal(back[:33], rb[:33]) and np.array_equal(back[33:], post[33:])
                else:
                    assert np.array_equal(back[RB["XPHID"]:], post[RB["XPHID"]:]) and not np.array_equal(back[:33], post[:33])
    # a stream without a plan takes no sample (SAME = 1 keeps the way back off it), an invalid row answers its mask: nothing else is touched
    lost = A0["ss"][0].copy(); lost[SS["ERRCNT"]] = N
    bad = rows[0].copy(); bad[SENSOR["RES"]] = -1.0
    for ss, row, want in ((lost, rows[0], -1), (A0["ss"][0], bad, 1 << SENSOR["RES"])):
        st, rec = np.arange(64.0), es.fresh_rec()
        code, rb, st2, rec2, meas = es.stream_sense(N, A0["rb"][0], ss, row, st, None, rec)
        if want == -1:
            st[SENSOR_STATE["SAME"]] = 1.0
        assert code == want and np.array_equal(rb, A0["rb"][0]) and np.array_equal(st2, st) and np.array_equal(rec2, rec, equal_nan=True) and np.isnan(meas).all()
    code, rb = es.stream_unsense(N, H, A0["rb"][0], A0["ss"][0], bad, np.zeros(64))
    assert code == 1 << SENSOR["RES"] and np.array_equal(rb, A0["rb"][0])
    # rint rounds half to even
    row, st, rb = bstream.sensor_table(1, res=0.5)[0], np.zeros(64), A0["rb"][0].copy()
    rb[:7] = [0.25, 0.75, -0.25, 1.25, 0.24, 0.26, -0.75]
    got = es.stream_sense(N, rb, A0["ss"][0], row, st)[1]
    assert got[:7].tolist() == [0.0, 1.0, -0.0, 1.0, 0.0, 0.5, -1.0] and bstream.sense_robot(rb, row, st)[0][:7].tolist() == got[:7].tolist()


@pytest.mark.parametrize("nw", [1, 4])
def test_hist_is_the_truth_and_meas_hist_the_sample(nw):
    """no events and no plant table: hist[t] is truth_robot applied to hist[t - 1] and the tick's first planned jerk (stage 0 of traj_hist[t]); meas_hist[t]
    under HOLD is the sample of tick t - 1, meas_hist[0] the sample of tick 0; the record is the numpy reduction of the emulator's own rows, exactly"""
    A0, Tab, _ = er.start(N, S, nw, B)
    nz = es.noise(T, B)
    for which in ("bn", "hold"):
        tab = _tables()[which]
        A, st = _copy(A0), np.zeros((B, 64))
        r = es.rollout(N, S, H, Tab.copy(), A, T, nw=nw, sensor=tab, sensor_state=st, sensor_noise=nz, log_stages=1)
        assert r["ran"] == es.RAN_SENSOR and r["ticks_run"].tolist() == [T] * B
        assert np.array_equal(A["rb"], r["hist"][T - 1][:, :RB["LEN"]])      # (the caller's robot array: the truth)
        for b in range(B):
            truth = np.concatenate([A0["rb"][None, b], r["hist"][:-1, b, :RB["LEN"]]])      # [T][43]: the record ahead of every tick
            c = r["traj_hist"][:, b, 21 * N:28 * N:N]                                          # [T][7]: the first planned jerk of every tick
            for t in range(T):
                if np.array_equal(r["meas_hist"][t, b], truth[t]):      # (SAME: the post stepped the truth itself)
                    assert _identity_row(tab[b]) or (which == "hold" and t == 0 and tab[b, SENSOR["NQ"]] != tab[b, SENSOR["NQ"]])
                s_ = np.zeros(64); s_[TRUTH][:33] = truth[t, :33]; s_[SENSOR_STATE["TRUTH"] + 33:SENSOR_STATE["TRUTH"] + 40] = truth[t, JERK]
                post = r["hist"][t, b, :RB["LEN"]].copy(); post[JERK] = c[t]
                want = bstream.truth_robot(post, s_, H, True)
                np.testing.assert_allclose(r["hist"][t, b, :33], want[:33], rtol=1e-12, atol=1e-15)
                assert np.array_equal(r["hist"][t, b, JERK], c[t])
                # the sample: the compiled step with HOLD off on the truth and the noise row of the tick the sample is from
                row = tab[b].copy(); row[SENSOR["HOLD"]] = NAN
                u = t - 1 if tab[b, SENSOR["HOLD"]] == 1.0 and t > 0 else t
                m = es.stream_sense(N, truth[u], A0["ss"][b], row, np.zeros(64), nz[u, b])[4]
                assert np.array_equal(r["meas_hist"][t, b, Q21], m[Q21]), (which, b, t)
            # the record
            d = r["meas_hist"][:, b, :7] - truth[:, :7]
            sumsq, dp = 0.0, np.zeros(T)
            for t in range(T):
                for j in range(7):
                    sumsq += d[t, j] * d[t, j]
                s2 = 0.0
                for k in range(3):
                    e = r["meas_hist"][t, b, RB["P"] + k] - truth[t, RB["P"] + k]
                    s2 += e * e
                dp[t] = np.sqrt(s2)
            rec = r["sensor_rec"][b]
            t_max, j_max = np.unravel_index(int(np.argmax(np.abs(d))), d.shape)
            assert rec[SENSOR_REC["SAMPLES"]] == T and rec[SENSOR_REC["SUMSQ_DQ"]] == sumsq and rec[SENSOR_REC["MAX_DQ"]] == np.abs(d).max(), (which, b, rec)
            assert rec[SENSOR_REC["MAX_DP"]] == dp.max() and rec[SENSOR_REC["TICK_DP"]] == int(np.argmax(dp)) and rec[7] == 0.0
            assert (rec[SENSOR_REC["TICK_DQ"]], rec[SENSOR_REC["JOINT_DQ"]]) == (t_max, j_max) or np.abs(d).max() == 0.0
            u = bstream.unpack_sensor_rec(rec)
            assert u["samples"] == T and u["max_dq"] == rec[SENSOR_REC["MAX_DQ"]] and u["max_dp"] == rec[SENSOR_REC["MAX_DP"]] and u["tick_dp"] == int(rec[SENSOR_REC["TICK_DP"]])


EDGE = [NAN, np.inf, -np.inf, -0.0, 0.0, 1.0, 1.0 + 2.0 ** -52, 0.5, 2.0, -1.0, -0.5, 1e-300, 1e308]


def test_the_python_rule_is_the_compiled_rule():
    """every slot on the edge values, one slot at a time: NaN, +-inf, -0.0, 0, negatives, 0.5, 2; the pad words are never looked at"""
    for k in range(SENSOR["LEN"]):
        for v in EDGE:
            row = np.full(SENSOR["LEN"], NAN); row[k] = v
            bad, used = es.sensor_check(row)
            assert bad == bstream.sensor_check(row) and bad & ~(1 << k) == 0, (k, v, bad)
            want = np.zeros(SENSOR["LEN"]); want[k] = 0.0 if k >= 12 or np.isnan(v) else v
            assert np.array_equal(used, want), (k, v, used)
    ok = lambda k: [v for v in EDGE[1:] if not bstream.sensor_check(np.where(np.arange(SENSOR["LEN"]) == k, v, NAN))]
    finite = [-0.0, 0.0, 1.0, 1.0 + 2.0 ** -52, 0.5, 2.0, -1.0, -0.5, 1e-300, 1e308]
    nonneg = [-0.0, 0.0, 1.0, 1.0 + 2.0 ** -52, 0.5, 2.0, 1e-300, 1e308]
    assert ok(SENSOR["BIAS"]) == finite and ok(SENSOR["BIAS"] + 6) == finite
    assert all(ok(SENSOR[k]) == nonneg for k in ("RES", "NQ", "NDQ", "NDDQ")) and ok(SENSOR["HOLD"]) == [-0.0, 0.0, 1.0]
    assert ok(12) == EDGE[1:] and ok(15) == EDGE[1:]
    for kw in (dict(bias=np.inf), dict(bias=[0.0] * 6 + [-np.inf]), dict(res=-1e-3), dict(res=np.inf), dict(nq=-1.0), dict(nddq=[0.5, -0.5]), dict(hold=0.5), dict(hold=2.0)):
        with pytest.raises(ValueError, match="sensor row"):
            bstream.sensor_table(2, **kw)


# ---- 5. invalid rows ----
@pytest.mark.parametrize("nw", [1, 4])
def test_invalid_rows_do_not_run_and_their_neighbours_do(nw):
    """rows 0 and 2 invalid (a negative step with an infinite offset; HOLD 0.5), rows 1 and 3 of the BN table"""
    A0, Tab, _ = er.start(N, S, nw, B)
    Q, ev, tab, nz = _queue(), _events(), _tables()["bn"], es.noise(T, B)
    bad = tab.copy()
    bad[0, SENSOR["RES"]], bad[0, SENSOR["BIAS"] + 5] = -1.0, np.inf
    bad[2] = NAN; bad[2, SENSOR["HOLD"]] = 0.5
    A, Tb, R, st, pst = _copy(A0), Tab.copy(), Q.copy(), np.full((B, 64), 1.5), bstream.plant_state_of(A0["rb"])
    for k in ("x", "g", "kkt", "p", "x0"):
        A[k][[0, 2]] = 7.25      # (what the memory held: it stays)
    A["iters"][[0, 2]], A["status"][[0, 2]] = 77, 9
    st[[1, 3]] = 0.0
    before, st_before, pst_before = _copy(A), st.copy(), pst.copy()
    common = dict(nw=nw, sensor_noise=nz, tune=er.table(), plant=_plant(), accept_capped=True, log_stages=N, **ev)
    r = es.rollout(N, S, H, Tb, A, T, sensor=bad, sensor_state=st, plant_state=pst, replan=R, **common)
    assert r["sensor_info"].tolist() == [1 << SENSOR["RES"] | 1 << SENSOR["BIAS"] + 5, 0, 1 << SENSOR["HOLD"], 0] and r["ticks_run"].tolist()[::2] == [0, 0]
    assert r["tune_info"].tolist() == [0] * B and r["plant_info"].tolist() == [0] * B
    for b in (0, 2):
        er.assert_arrays_equal(er.unstack(before, b), er.unstack(A, b), f"invalid row, stream {b}")
        assert np.array_equal(Tb[b], Tab[b]) and np.array_equal(R[b], Q[b]) and (R[b, :, RP["FLAG"]] == 1.0).all()
        assert np.array_equal(st[b], st_before[b]) and np.array_equal(pst[b], pst_before[b])
        assert all(np.isnan(r[k][:, b]).all() for k in ("hist", "traj_hist", "tube_hist", "log_hist", "meas_hist"))
        assert r["legs_done"][b] == 0 and (r["leg_fired"][b] == -1).all() and (r["leg_why"][b] == 0).all() and (r["replan_info"][b] == -1).all()
        assert np.array_equal(r["sensor_rec"][b], es.fresh_rec()) and r["sensor_rec"][b].tolist() == [0, -np.inf, -1, -1, -np.inf, -1, 0, 0]
    # the neighbours: bit-equal to a run without the invalid rows
    C, Tc, Rc, sc, pc = _copy(A0), Tab.copy(), Q.copy(), np.zeros((B, 64)), bstream.plant_state_of(A0["rb"])
    good = es.rollout(N, S, H, Tc, C, T, sensor=tab, sensor_state=sc, plant_state=pc, replan=Rc, **common)
    for b in (1, 3):
        er.assert_arrays_equal(er.unstack(C, b), er.unstack(A, b), f"neighbour {b}")
        er.assert_streams_equal(er.stream_of(r, b), er.stream_of(good, b), f"neighbour {b}")
        assert np.array_equal(Tb[b], Tc[b]) and np.array_equal(R[b], Rc[b]) and np.array_equal(st[b], sc[b]) and np.array_equal(pst[b], pc[b])
        assert np.array_equal(r["sensor_rec"][b], good["sensor_rec"][b]) and np.array_equal(r["meas_hist"][:, b], good["meas_hist"][:, b], equal_nan=True)


# ---- 6. a plan exhausted mid-run ----
@pytest.mark.parametrize("nw,wave_order", [(1, 0), (4, 1)])
def test_the_tick_whose_post_exhausts_the_plan_gets_its_truth_back_and_no_step(nw, wave_order):
    """the missions' rescue scenario (tests/test_stream_rollout_legs.py, built at (2, 2)): one-iteration ticks on plants a push has carried off their paths --
    tick 0 fails and replays, the post of tick 1 exhausts the plan and returns early.  Stream 0 is rescued by its ON_LOST record and runs on, stream 1 stops,
    stream 2 never runs.  Behind tick 1 the robot record is the truth ahead of it, bit for bit: the sample has gone, no step was taken"""
    from tests.test_stream_rollout_legs import _rescue_case
    n, s = 2, 2
    A0, Tab, Q, lt, lo = _rescue_case(n, s, nw)
    tab = bstream.sensor_table(3, bias=1e-3, nq=1e-4)
    nz = es.noise(T, 3)
    r, A, Tb, R, _, st, loops = es.assert_equals_the_loop(n, s, A0, Tab, Q, T, tab, f"rescue, nw {nw}", sensor_noise=nz, nw=nw, wave_order=wave_order, leg_tick=lt, leg_on=lo, max_iter=1)
    assert r["ticks_run"][0] > 2 and r["ticks_run"].tolist()[1:] == [2, 0] and (r["hist"][1, :2, ROLL["ERRCNT"]] == n).all() and r["leg_fired"][0, 0] == 1
    assert r["sensor_rec"][:, SENSOR_REC["SAMPLES"]].tolist() == r["ticks_run"].tolist()
    for b in (0, 1):
        assert np.array_equal(r["hist"][1, b, :33], r["hist"][0, b, :33]) and np.array_equal(r["hist"][1, b, :33], st[b, TRUTH][:33])      # the truth ahead of tick 1, restored
        assert not np.array_equal(r["meas_hist"][1, b, :33], r["hist"][0, b, :33])                                                         # ... which the pack did not see
        assert not np.array_equal(r["hist"][0, b, :33], A0["rb"][b, :33])                                                                  # (tick 0 did step)
    assert np.array_equal(A["rb"][1], r["hist"][1, 1, :RB["LEN"]]) and np.array_equal(r["sensor_rec"][2], es.fresh_rec()) and not st[2].any()


# ---- 7. chaining ----
@pytest.mark.parametrize("nw", [1, 4])
def test_one_rollout_of_six_ticks_is_two_of_three_that_hand_over_the_state(nw):
    """HOLD rows make the state matter: with a fresh state in the second half their histories differ"""
    A0, Tab, _ = er.start(N, S, nw, B)
    tab, nz, d = _tables()["hold"], es.noise(T, B), er.disturbances(T, B, on=(1, 4))
    half = lambda a, k: np.ascontiguousarray(a[3 * k:3 * k + 3])
    A, st = _copy(A0), np.zeros((B, 64))
    whole = es.rollout(N, S, H, Tab.copy(), A, T, nw=nw, sensor=tab, sensor_state=st, sensor_noise=nz, disturb=d, log_stages=N)
    C, sc = _copy(A0), np.zeros((B, 64))
    first = es.rollout(N, S, H, Tab.copy(), C, 3, nw=nw, sensor=tab, sensor_state=sc, sensor_noise=half(nz, 0), disturb=half(d, 0), log_stages=N)
    second = es.rollout(N, S, H, Tab.copy(), C, 3, nw=nw, sensor=tab, sensor_state=sc, sensor_noise=half(nz, 1), disturb=half(d, 1), log_stages=N)
    assert whole["ticks_run"].tolist() == [T] * B and first["ticks_run"].tolist() == [3] * B
    for b in range(B):
        er.assert_arrays_equal(er.unstack(A, b), er.unstack(C, b), f"chained, stream {b}")
    assert np.array_equal(st, sc)
    for k in es.HISTORIES:
        assert np.array_equal(whole[k], np.concatenate([first[k], second[k]]), equal_nan=True), k
    assert (first["sensor_rec"][:, 0] + second["sensor_rec"][:, 0] == T).all() and np.array_equal(whole["sensor_rec"][:, SENSOR_REC["SUMSQ_DQ"]] > 0, [True, True, True, False])
    # a second half that starts from a fresh state is another run for the HOLD rows: its first tick is handed its own sample
    E, se = _copy(A0), np.zeros((B, 64))
    es.rollout(N, S, H, Tab.copy(), E, 3, nw=nw, sensor=tab, sensor_state=se, sensor_noise=half(nz, 0), disturb=half(d, 0), log_stages=N)
    fresh = es.rollout(N, S, H, Tab.copy(), E, 3, nw=nw, sensor=tab, sensor_state=np.zeros((B, 64)), sensor_noise=half(nz, 1), disturb=half(d, 1), log_stages=N)
    same = [np.array_equal(fresh["hist"][:, b], second["hist"][:, b]) for b in range(B)]
    assert same == [False, False, False, True], same


# ---- 8. housekeeping ----
def test_argument_errors_of_the_entry():
    """sensor without sensor_state, and what the plants' entry refuses, with a sensor table; the sensor's outputs and the noise may be NULL"""
    A0, Tab, _ = er.start(N, S, 1, B)
    Q, tab = _queue(), _tables()["bn"]
    lt, lo = np.ones((B, 2), dtype=np.int32), np.zeros((B, 2), dtype=np.int32)
    ok = dict(replan=Q, leg_tick=lt, leg_on=lo, tune=er.table(), plant=_plant(), plant_state=bstream.plant_state_of(A0["rb"]))
    for kw in (dict(ok, state=None), dict(state=None), dict(ok, plant_state=None), dict(ok, leg_tick=None), dict(ok, leg_on=None), dict(ok, update_flags=8), dict(ok, ticks=0),
               dict(ok, simulate=False), dict(ok, goal_tol=-1.0), dict(goal_tol=NAN), dict(ok, audit_tol=-1.0), dict(audit_tol=np.inf), dict(ok, log_stages=N + 1)):
        A, Tb = _copy(A0), Tab.copy()
        kw = dict(kw); kw["replan"] = None if kw.get("replan") is None else Q.copy()
        st = kw.pop("state", np.zeros((B, 64)))
        assert es.rollout(N, S, H, Tb, A, kw.pop("ticks", 2), sensor=tab, sensor_state=st, want_rc=True, **kw) == 1, {k: v for k, v in kw.items() if k != "replan"}
        for b in range(B):
            er.assert_arrays_equal(er.unstack(A0, b), er.unstack(A, b), "nothing runs")
    free = dict(ok, replan=Q.copy(), plant_state=bstream.plant_state_of(A0["rb"]))
    assert es.rollout(N, S, H, Tab.copy(), _copy(A0), 1, sensor=tab, sensor_state=np.zeros((B, 64)), want_rc=True, want_meas=False, want_sensor_rec=False, want_sensor_info=False, **free) == 0
    free = dict(ok, replan=Q.copy(), plant_state=bstream.plant_state_of(A0["rb"]))
    assert es.rollout(N, S, H, Tab.copy(), _copy(A0), 1, sensor=None, sensor_state=None, want_rc=True, **free) == 0      # (no table: no state needed)
    L = es.lib()
    assert L.bmpc_emu_rollout_sensor_ok(ctypes.byref(es.NArgs())) == 1 and L.bmpc_emu_rollout_sensor_ok(ctypes.byref(es.NArgs(sensor=1))) == 0
    assert L.bmpc_emu_rollout_sensor_ok(ctypes.byref(es.NArgs(sensor=1, sensor_state=1))) == 1 and L.bmpc_emu_rollout_sensor_ok(ctypes.byref(es.NArgs(sensor_state=1, meas_hist=1))) == 1


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
    row, st, rec = es.sensor_slots()
    for first, prefix, d, kernel in (("BMPC_SENSOR_BIAS", "BMPC_SENSOR_", SENSOR, row), ("BMPC_SENSOR_STATE_HELD", "BMPC_SENSOR_STATE_", SENSOR_STATE, st),
                                     ("BMPC_SENSOR_REC_SAMPLES", "BMPC_SENSOR_REC_", SENSOR_REC, rec)):
        e = {k[len(prefix):]: v for k, v in enum_of(first).items()}
        assert e == d and [v for k, v in sorted(d.items(), key=lambda kv: kv[1]) if k != "LEN"] == kernel, (prefix, e, d, kernel)
    assert (SENSOR["LEN"], SENSOR_STATE["LEN"], SENSOR_REC["LEN"]) == (16, 64, 8) and es.lib().bmpc_emu_sensor_slot(0, -2) == 12
    # the records: RArgs keeps its 30 members, NArgs is the six of the entry in their order, in both builds
    for nw in (1, 4):
        L = es.lib(nw)
        assert len(er.RArgs._fields_) == 30 and L.bmpc_emu_sensor_rargs_size() == ctypes.sizeof(er.RArgs) == er.lib(nw).bmpc_emu_rargs_size()
        assert [L.bmpc_emu_nargs_offset(name.encode()) for name, _ in es.NArgs._fields_] == [getattr(es.NArgs, name).offset for name, _ in es.NArgs._fields_]
        assert [name for name, _ in es.NArgs._fields_] == ["sensor", "sensor_state", "sensor_info", "sensor_rec", "sensor_noise", "meas_hist"] and L.bmpc_emu_nargs_offset(b"plant") == -1
    from boundmpc_amd import _lib, build
    import boundmpc_amd
    syms = ("bmpc_stream_sensor_len", "bmpc_stream_sensor_state_len", "bmpc_stream_sensor_rec_len", "bmpc_stream_rollout_sensor", "bmpc_stream_sense", "bmpc_stream_unsense")
    for sym in syms:
        assert sym in _lib.SIGNATURES and re.search(r"\b%s\(" % sym, header)
    assert len(_lib.SIGNATURES["bmpc_stream_rollout_sensor"][1]) == len(_lib.SIGNATURES["bmpc_stream_rollout_plant"][1]) + 6
    assert len(_lib.SIGNATURES["bmpc_stream_sense"][1]) == 12 and len(_lib.SIGNATURES["bmpc_stream_unsense"][1]) == 7
    if os.path.exists(_lib.LIB_PATH):      # (a built tree: the symbols are exported; loading the library needs no GPU)
        L = ctypes.CDLL(_lib.LIB_PATH)
        assert all(hasattr(L, sym) for sym in syms) and (L.bmpc_stream_sensor_len(), L.bmpc_stream_sensor_state_len(), L.bmpc_stream_sensor_rec_len()) == (16, 64, 8)
    units = [os.path.basename(u) for u in build.UNITS]
    assert "bmpc_rollout_sensor.hip" in units and "bmpc_team_rollout_sensor.hip" in units
    params = set(inspect.signature(bstream.StreamBatch.rollout).parameters)
    assert {"sensor", "sensor_noise", "want_meas", "want_sensor_rec"} <= params and all(hasattr(bstream.StreamBatch, m) for m in ("sense", "unsense", "sensor_reset", "sensor_state"))
    assert bstream.ROLLOUT_ENTRIES[-1] == "bmpc_stream_rollout_plant" and bstream.rollout_entry(plant=True) == "bmpc_stream_rollout_plant"      # (they stay as they are)
    for name in ("SENSOR", "SENSOR_STATE", "SENSOR_REC", "sensor_table", "sensor_check", "sense_robot", "truth_robot", "unpack_sensor_rec"):
        assert getattr(boundmpc_amd, name) is getattr(bstream, name)
    # the docstring and the header say what each output describes
    for text in (bstream.StreamBatch.rollout.__doc__, header):
        assert "WHAT EACH OUTPUT THEN DESCRIBES" in text and "the TRUTH" in text and "MEASUREMENT and the plan made from it" in text
    # sensor_table: scalars, [7] and [B][7] broadcast, NaN elsewhere
    t = bstream.sensor_table(3, bias=np.arange(7.0), res=[1e-3, NAN, 0.0], nq=2.0, hold=[1.0, 0.0, NAN])
    assert t.shape == (3, 16) and (t[:, :7] == np.arange(7.0)).all() and t[0, 7] == 1e-3 and np.isnan(t[1, 7]) and (t[:, 8] == 2.0).all() and np.isnan(t[:, 9:11]).all()
    assert t[:2, 11].tolist() == [1.0, 0.0] and np.isnan(t[:, 12:]).all() and np.isnan(bstream.sensor_table(2)).all()
    with pytest.raises(ValueError, match="must be a scalar"):
        bstream.sensor_table(2, bias=[1.0] * 3)


def sanitizer_cases(nw):
    A0, Tab, _ = er.start(N, S, nw, B)
    tab = _tables()["hold"]; tab[3, SENSOR["RES"]] = RES16
    bad = tab.copy(); bad[0, SENSOR["NQ"]] = -1.0
    return [("table", dict(N=N, S=S, h=H, T=Tab, A=A0, ticks=3, sensor=tab, sensor_noise=es.noise(3, B), plant=_plant(), plant_state=bstream.plant_state_of(A0["rb"]),
                           disturb=er.disturbances(3, B, on=(1,)))),
            ("refused", dict(N=N, S=S, h=H, T=Tab, A=A0, ticks=3, sensor=bad))]


@pytest.mark.parametrize("nw", [1, 4])
def test_the_sensor_text_is_clean_under_the_sanitizers(nw):
    """the host program with its own main, built with -fsanitize=address,undefined on exact-size buffers and run as a child process (nothing is loaded into
    this interpreter, nothing preloaded); on teams under both wave orders"""
    out = es.run_sanitized(sanitizer_cases(nw), nw)
    print("\n".join(out))
    assert len(out) == 2 and all("rc 0 ran 7" in line and "DIFFERS" not in line for line in out)
    assert "[stream 0 ticks_run 3 sensor_info 0 samples 3]" in out[0] and "[stream 3 ticks_run 3 sensor_info 0 samples 3]" in out[0]
    assert "[stream 0 ticks_run 0 sensor_info %d samples 0]" % (1 << SENSOR["NQ"]) in out[1] and "[stream 1 ticks_run 3 sensor_info 0 samples 3]" in out[1]
