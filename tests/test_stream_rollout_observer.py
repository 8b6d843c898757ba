"""Observers inside a rollout -- a table of state estimators per stream between the sample of the stream's sensor and what the pack, the solve and the post of
a tick read, validated on the device -- as device code compiled for the CPU (csrc/bmpc_rollout_body.inl with SE and OB, csrc/bmpc_stream_observer.inl;
tests/emu/bmpc_emu_rollout_observer.cpp, once for one wave per stream and once for teams of four).  The checkers: the numpy mirror
boundmpc_amd.stream.observe_robot (the specification of one step), the sensor's entry (an identity observer leaves what it leaves), the contract -- the entry
against the per-tick loop {observe text, tick text, unsense text, plant step text, tube text, log text, disturb text, update text of the head record due} for
one stream (emu_rollout_observer.contract_loop), bit for bit -- and the two properties the level exists for: a LEAD row compensates the sensor's HOLD exactly
(P2), and a gain below 1 filters the sensor's noise (P3).  (10, 4), B = 4 streams of emu_rollout.small_stream behind a solved-out tick 0, T = 6; the contract
on B = 5, one stream per row of ROWS.
ROWS, five observer rows, each with a sensor row that makes it matter: IDENT = the identity values behind offsets and noise, GAINS = 0.3 / 0.5 / 0.7 behind
noise on q, dq and ddq, LEAD = one step of lead with gains (0.3, 0.5, 1) behind the sensor's HOLD and noise on q, GATE = a gate of 1e-3 rad with gain 0.5
behind noise on q with one draw of 0.1 rad, NAN = all NaN behind a 16-bit encoder step."""
import ctypes
import functools
import inspect
import os
import re

import numpy as np
import pytest

from boundmpc_amd import stream as bstream
from tests.emu import emu_rollout as er, emu_rollout_observer as eo, emu_rollout_sensor as es
from tests.test_stream_rollout_sensor import RES16, _events, _noise, _plant, _queue, _tables

OBSERVER, OBSERVER_STATE, OBSERVER_REC = bstream.OBSERVER, bstream.OBSERVER_STATE, bstream.OBSERVER_REC
SENSOR, SENSOR_STATE, SENSOR_REC, ROLL, RB, SS = bstream.SENSOR, bstream.SENSOR_STATE, bstream.SENSOR_REC, bstream.ROLL, bstream.RB, bstream.SS
N, S, T, B = 10, 4, 6, 4
H = er.H
NAN = float("nan")
_copy = er.copy_arrays
Q21 = slice(0, 21)
JERK = slice(RB["JERK"], RB["JERK"] + 7)
ROWS = ("ident", "gains", "lead", "gate", "nan")
OUTLIER = (3, 2, 1000.0)      # tick, joint and unit draw of the GATE row's outlier: 1000 x NQ = 0.1 rad
IDENT = np.array([1.0, 1.0, 1.0, 0.0, np.inf, NAN, NAN, NAN])


def _rows(ticks=T, seed=11):
    """-> (observer rows [5][8], sensor rows [5][16], noise [ticks][5][21]) in the order of ROWS"""
    ob = bstream.observer_table(5, lq=[1.0, 0.3, 0.3, 0.5, NAN], ldq=[1.0, 0.5, 0.5, NAN, NAN], lddq=[1.0, 0.7, 1.0, NAN, NAN], lead=[0.0, NAN, 1.0, NAN, NAN],
                                gate=[np.inf, NAN, NAN, 1e-3, NAN])
    assert np.array_equal(ob[0], IDENT, equal_nan=True) and np.isnan(ob[4]).all()
    bias = np.random.default_rng(23).uniform(-1e-3, 1e-3, 7)
    se = bstream.sensor_table(5, bias=[[1e-3] * 7, [NAN] * 7, [NAN] * 7, [NAN] * 7, bias], nq=[1e-4, 1e-4, 1e-4, 1e-4, NAN], ndq=[NAN, 1e-3, NAN, NAN, NAN],
                              nddq=[NAN, 1e-2, NAN, NAN, NAN], hold=[NAN, NAN, 1.0, NAN, NAN], res=[NAN, NAN, NAN, NAN, RES16])
    nz = es.noise(ticks, 5, seed)
    if ticks > OUTLIER[0]:
        nz[OUTLIER[0], 3, OUTLIER[1]] = OUTLIER[2]
    return ob, se, nz


def _acc(rec, d, dp, tick, at):
    """a record's words from MAX_DQ on (at = its place) as stream_sense and stream_observe accumulate them"""
    for j in range(7):
        e = abs(d[j])
        if e > rec[at]:
            rec[at], rec[at + 1], rec[at + 2] = e, tick, j
        rec[at + 5] += d[j] * d[j]
    if dp > rec[at + 3]:
        rec[at + 3], rec[at + 4] = dp, tick


def _truths(rb0, ticks, rng):
    """[ticks][43]: a plant that starts at rb0 and takes the model's chain step under a new random jerk every tick (p_lie and v: the kinematics of the state)"""
    from boundmpc_amd.robot_model import RobotModel
    out, rb = [], np.array(rb0, dtype=float)
    for _ in range(ticks):
        out.append(rb.copy())
        c = rng.normal(size=7) * 5.0
        x = bstream._observer_step(rb[Q21], rb[JERK], c, H)
        p, J, _ = RobotModel().forward_kinematics(x[:7], x[7:14])
        rb[Q21], rb[JERK], rb[RB["P"]:RB["P"] + 6], rb[RB["V"]:RB["V"] + 6] = x, c, p, J @ x[7:14]
    return np.array(out)


# ---- 1. validity ----
EDGE = [NAN, np.inf, -np.inf, -0.0, 0.0, 1.0, 1.0 + 2.0 ** -52, 0.5, 2.0, -1.0, -0.5, 1e-300, 1e308]


def test_the_python_rule_is_the_compiled_rule():
    """every slot on the edge values, one slot at a time: 0, negatives, > 1, NaN, +-inf per gain; LEAD 0.5; GATE 0, -1, +inf; the identity row; the pad words
    are never looked at; observer_table raises on what the device refuses"""
    for k in range(OBSERVER["LEN"]):
        for v in EDGE:
            row = np.full(OBSERVER["LEN"], NAN); row[k] = v
            bad, used = eo.observer_check(row)
            assert bad == bstream.observer_check(row) and bad & ~(1 << k) == 0, (k, v, bad)
            want = np.array([1.0, 1.0, 1.0, 0.0, np.inf, 0.0, 0.0, 0.0])
            if k < 5 and not np.isnan(v):
                want[k] = v
            assert np.array_equal(used, want), (k, v, used)
    ok = lambda k: [v for v in EDGE[1:] if not bstream.observer_check(np.where(np.arange(OBSERVER["LEN"]) == k, v, NAN))]
    assert all(ok(OBSERVER[k]) == [1.0, 0.5, 1e-300] for k in ("LQ", "LDQ", "LDDQ"))
    assert ok(OBSERVER["LEAD"]) == [-0.0, 0.0, 1.0] and ok(OBSERVER["GATE"]) == [np.inf, 1.0, 1.0 + 2.0 ** -52, 0.5, 2.0, 1e-300, 1e308]
    assert ok(5) == EDGE[1:] and ok(7) == EDGE[1:]
    assert eo.observer_check(IDENT)[0] == 0 == bstream.observer_check(IDENT) and np.array_equal(eo.observer_check(IDENT)[1][:5], IDENT[:5])
    assert np.array_equal(eo.observer_check(np.full(8, NAN))[1], eo.observer_check(IDENT)[1])
    for kw in (dict(lq=0.0), dict(lq=-0.5), dict(ldq=1.5), dict(lddq=np.inf), dict(lddq=[0.5, -np.inf]), dict(lead=0.5), dict(lead=2.0), dict(gate=0.0), dict(gate=-1.0)):
        with pytest.raises(ValueError, match="observer row"):
            bstream.observer_table(2, **kw)
    t = bstream.observer_table(3, lq=[0.3, NAN, 1.0], lead=1.0, gate=np.inf)
    assert t.shape == (3, 8) and t[0, 0] == 0.3 and np.isnan(t[1, 0]) and (t[:, 3] == 1.0).all() and np.isinf(t[:, 4]).all() and np.isnan(t[:, [1, 2, 5, 6, 7]]).all()
    with pytest.raises(ValueError, match="must be a scalar"):
        bstream.observer_table(2, lq=[0.5] * 3)


# ---- 2. the mirror against the text; the sample is stream_sense's ----
def test_eight_chained_steps_against_the_python_mirror():
    """stream.observe_robot against the g++ step over 8 chained ticks of a plant under random jerks, on the five ROWS, each side carrying its own states and
    records: the record's q, dq, ddq, the raw sample, the sensor state, the observer state and every word of the two records that the joint state decides, bit
    for bit.  The words that come out of the KINEMATICS -- p_lie and v of the record, MAX_DP of the two records -- are compared at 1e-12, the bound of the
    sensor's one-step test for the same words: the mirror's kinematics is RobotModel's, another text than fk_motion (sin and cos included), and equals it to
    rounding only.  The GATE row rejects its outlier and nothing else; the LEAD row lags from its second tick on."""
    A0, _, _ = er.start(N, S, 1, B)
    ob, se, nz = _rows(8)
    rng = np.random.default_rng(5)
    for k, name in enumerate(ROWS):
        truth = _truths(A0["rb"][k % B], 8, rng)
        st_c, ost_c, rec_c, orec_c = np.zeros(64), np.zeros(40), es.fresh_rec(), eo.fresh_rec()
        st_m, ost_m, rec_m, orec_m = np.zeros(64), np.zeros(40), es.fresh_rec(), eo.fresh_rec()
        rejected = []
        for t in range(8):
            code, rb, st_c, ost_c, rec_c, orec_c, meas, smp, _ = eo.stream_observe(N, H, truth[t], A0["ss"][0], se[k], st_c, ob[k], ost_c, nz[t, k], rec_c, orec_c, t)
            want, st_m, ost_m, m, d_e, dp_e, d_s, dp_s, rej = bstream.observe_robot(truth[t], se[k], st_m, ob[k], ost_m, H, nz[t, k])
            rejected.append(rej)
            rec_m[0] += 1; orec_m[0] += 1; orec_m[1] += rej
            _acc(rec_m, d_s, dp_s, t, SENSOR_REC["MAX_DQ"]); _acc(orec_m, d_e, dp_e, t, OBSERVER_REC["MAX_DQ"])
            what = f"{name}, tick {t}"
            assert code == 0 and np.array_equal(meas, rb), what
            assert np.array_equal(rb[Q21], want[Q21]) and np.array_equal(rb[RB["XPHID"]:], want[RB["XPHID"]:]) and np.array_equal(smp, m), what
            np.testing.assert_allclose(rb[21:33], want[21:33], rtol=1e-12, atol=1e-15, err_msg=what)
            assert np.array_equal(st_c, st_m) and np.array_equal(ost_c, ost_m), what
            for got, mine, dpw in ((rec_c, rec_m, SENSOR_REC["MAX_DP"]), (orec_c, orec_m, OBSERVER_REC["MAX_DP"])):
                keep = [i for i in range(8) if i != dpw]
                assert np.array_equal(got[keep], mine[keep]), (what, got, mine)
                np.testing.assert_allclose(got[dpw], mine[dpw], rtol=1e-12, atol=1e-15, err_msg=what)
            # the record is the estimate where it is not the truth, the sensor's state carries the truth, SAME is decided on the estimate
            assert np.array_equal(st_c[24:57], truth[t, :33]) and st_c[SENSOR_STATE["SAME"]] == float(np.array_equal(rb[Q21], truth[t, Q21]))
        assert rejected == [name == "gate" and t == OUTLIER[0] for t in range(8)], (name, rejected)
        assert ost_c[OBSERVER_STATE["HAS"]] == 1.0 and ost_c[OBSERVER_STATE["LAGS"]] == float(name == "lead") and orec_c[OBSERVER_REC["N_REJ"]] == float(name == "gate")
        assert bstream.unpack_observer_rec(orec_c)["n_rej"] == int(name == "gate") and bstream.unpack_observer_rec(orec_c)["samples"] == 8


def test_the_sample_of_the_observer_is_the_sample_of_the_sensor():
    """stream_observe restates the arithmetic of stream_sense: over 4 chained ticks on the sensor rows of ROWS and of the sensors' HOLD table, with draws that are
    not finite among them, the raw sample, HELD, HAS and TRUTH equal what stream_sense leaves, bit for bit, whatever the observer row; behind an identity or NaN
    observer row the robot record, the whole sensor state and the sensor record do"""
    A0, _, _ = er.start(N, S, 1, B)
    ob, se, nz = _rows(4)
    nz[1, :, 5], nz[2, :, 9] = np.inf, NAN
    rng = np.random.default_rng(9)
    sensors = list(se) + list(_tables()["hold"][:3]) + list(_tables()["bn"][:2])
    for k, srow in enumerate(sensors):
        truth = _truths(A0["rb"][k % B], 4, rng)
        for which, orow in enumerate((ob[k % 5], IDENT, np.full(8, NAN))):
            st_s, rec_s, st_o, ost, rec_o = np.zeros(64), es.fresh_rec(), np.zeros(64), np.zeros(40), es.fresh_rec()
            for t in range(4):
                code, rb_s, st_s, rec_s, meas = es.stream_sense(N, truth[t], A0["ss"][0], srow, st_s, nz[t, k % 5], rec_s, t)
                code2, rb_o, st_o, ost, rec_o, _, _, smp, _ = eo.stream_observe(N, H, truth[t], A0["ss"][0], srow, st_o, orow, ost, nz[t, k % 5], rec_o, None, t)
                assert code == code2 == 0 and np.array_equal(smp, rb_s[Q21]), (k, t)
                keep = [i for i in range(64) if i != SENSOR_STATE["SAME"]]
                assert np.array_equal(st_o[keep], st_s[keep]), (k, t)
                assert np.array_equal(rec_o[[0, 1, 2, 3, 6, 7]], rec_s[[0, 1, 2, 3, 6, 7]]), (k, t)      # (the sample against the truth, whatever the estimate)
                if which or k % 5 in (0, 4):
                    assert np.array_equal(rb_o, rb_s) and np.array_equal(st_o, st_s) and np.array_equal(rec_o, rec_s), (k, t)
                else:      # (a second kinematics pass, or none: the position word to rounding)
                    np.testing.assert_allclose(rec_o[[4, 5]], rec_s[[4, 5]], rtol=1e-12, atol=1e-15)
    # a stream without a plan takes no sample and makes no estimate; an invalid row of either table leaves its masks and touches nothing
    lost = np.where(np.arange(A0["ss"].shape[1]) == SS["ERRCNT"], float(N), A0["ss"][0])
    code, rb, st, ost, _, _, meas, smp, _ = eo.stream_observe(N, H, A0["rb"][0], lost, se[1], np.zeros(64), ob[1], np.zeros(40))
    assert code == -1 and np.array_equal(rb, A0["rb"][0]) and st[SENSOR_STATE["SAME"]] == 1.0 and not ost.any() and np.isnan(meas).all() and np.isnan(smp).all()
    bad_o, bad_s = ob[1].copy(), se[1].copy()
    bad_o[OBSERVER["GATE"]], bad_s[SENSOR["HOLD"]] = 0.0, 0.5
    for srow, orow, masks in ((se[1], bad_o, (0, 1 << OBSERVER["GATE"])), (bad_s, ob[1], (1 << SENSOR["HOLD"], 0)), (bad_s, bad_o, (1 << SENSOR["HOLD"], 1 << OBSERVER["GATE"]))):
        code, rb, st, ost, _, _, meas, smp, got = eo.stream_observe(N, H, A0["rb"][0], A0["ss"][0], srow, np.full(64, 1.5), orow, np.full(40, 2.5))
        assert code == -2 and got == masks and np.array_equal(rb, A0["rb"][0]) and (st == 1.5).all() and (ost == 2.5).all() and np.isnan(meas).all()


# ---- 3. P1: identity ----
def _mode_kw(mode):
    """converged: the handle's settings; held: the held mode of tests/rollout_contract.py on every stream, as a settings table (row 2 of er.table())"""
    return dict(tune=np.ascontiguousarray(np.tile(er.table()[2], (B, 1)))) if mode == "held" else {}


@pytest.mark.parametrize("which", ["bn", "res", "hold", "nan"])
@pytest.mark.parametrize("mode", ["converged", "held"])
@pytest.mark.parametrize("nw", [1, 4])
def test_no_table_a_table_of_nan_and_the_identity_table_are_the_sensors_entry(nw, mode, which):
    """P1, on the four sensor tables of tests/test_stream_rollout_sensor.py with a queue, disturbances and a plant table: every tick array, every output of the
    sensor's entry, the plant and sensor states and records, bit for bit; without a table no observer argument is looked at"""
    A0, Tab, _ = er.start(N, S, nw, B)
    ev, mk = _events(), _mode_kw(mode)
    for tab in (_tables()[which],):
        nz = _noise(which)
        A, Tb, R, pst, sst = _copy(A0), Tab.copy(), _queue(), bstream.plant_state_of(A0["rb"]), np.zeros((B, 64))
        common = dict(nw=nw, sensor=tab, sensor_noise=nz, plant=_plant(), accept_capped=True, log_stages=N, **ev, **mk)
        want = es.rollout(N, S, H, Tb, A, T, sensor_state=sst, plant_state=pst, replan=R, **common)
        assert want["ran"] == es.RAN_SENSOR and (want["ticks_run"] >= 2).all()
        for otab, ran in ((None, es.RAN_SENSOR), (np.full((B, 8), NAN), eo.RAN_OBSERVER), (np.tile(IDENT, (B, 1)), eo.RAN_OBSERVER)):
            C, Tc, Rc, pc, sc, oc = _copy(A0), Tab.copy(), _queue(), bstream.plant_state_of(A0["rb"]), np.zeros((B, 64)), np.zeros((B, 40))
            r = eo.rollout(N, S, H, Tc, C, T, sensor_state=sc, plant_state=pc, replan=Rc, observer=otab, observer_state=oc if otab is not None else None, **common)
            what = f"{which}, nw {nw}, {mode}, observer {'none' if otab is None else 'NaN' if np.isnan(otab).all() else 'identity'}"
            assert r["ran"] == ran, what
            for k in er.TICK_ARRAYS:
                assert np.array_equal(A[k], C[k], equal_nan=True), (what, k)
            assert np.array_equal(Tb, Tc) and np.array_equal(R, Rc, equal_nan=True) and np.array_equal(pst, pc) and np.array_equal(sst, sc), what
            for k in want:
                if k != "ran":
                    assert (want[k] is None and r[k] is None) or np.array_equal(want[k], r[k], equal_nan=True), (what, k)
            if otab is None:
                assert r["observer_info"] is None and r["sample_hist"] is None and not oc.any()
            else:      # the estimate is the sample: the two records agree word for word, the raw sample is the record's
                assert (r["observer_info"] == 0).all() and (r["observer_rec"][:, OBSERVER_REC["N_REJ"]] == 0).all()
                assert np.array_equal(r["observer_rec"][:, 2:], r["sensor_rec"][:, 1:7]) and np.array_equal(r["observer_rec"][:, 0], r["sensor_rec"][:, 0])
                assert np.array_equal(r["sample_hist"], r["meas_hist"][:, :, Q21], equal_nan=True)
                for b in range(B):
                    n = int(r["ticks_run"][b])
                    assert np.array_equal(oc[b, :21], r["meas_hist"][n - 1, b, Q21]) and oc[b, OBSERVER_STATE["HAS"]] == 1.0 and oc[b, OBSERVER_STATE["LAGS"]] == 0.0


# ---- 4. P2: exact delay compensation ----
@pytest.mark.parametrize("with_plant", [False, True])
@pytest.mark.parametrize("nw", [1, 4])
def test_a_lead_row_compensates_the_hold_of_an_exact_sensor(nw, with_plant):
    """P2.  An exact sensor with HOLD = 1, observer LEAD = 1 with gains (0.3, 0.5, 1), no noise, no disturbance, with and without a non-identity plant table: in the
    same run the q, dq, ddq the pack of tick t read (meas_hist[t]) equal the plant the tick started from (hist[t - 1], or the initial records) to 1e-12, for
    every tick run.  The bound is derived: the estimate repeats the truth's own chain step on equal inputs and the innovation is a rounding residue contracted
    by 1 - L; 1e-12 is about three orders above an ulp of the largest joint word of these streams and six or more orders below the effect of HOLD without LEAD
    on the same case, which is asserted here to exceed 1e-6: that is what shows the test can fail."""
    A0, Tab, _ = er.start(N, S, nw, B)
    sensor = bstream.sensor_table(B, hold=1.0)
    pl = dict(plant=_plant()) if with_plant else {}
    worst = {}
    for name, otab in (("lead", bstream.observer_table(B, lq=0.3, ldq=0.5, lddq=1.0, lead=1.0)), ("no lead", bstream.observer_table(B))):
        A, pst = _copy(A0), bstream.plant_state_of(A0["rb"]) if with_plant else None
        r = eo.rollout(N, S, H, Tab.copy(), A, T, nw=nw, sensor=sensor, sensor_state=np.zeros((B, 64)), observer=otab, observer_state=np.zeros((B, 40)), plant_state=pst,
                       log_stages=N, **pl)
        assert r["ran"] == eo.RAN_OBSERVER and (r["ticks_run"] == T).all() and not r["observer_info"].any()
        start = np.concatenate([A0["rb"][None, :, Q21], r["hist"][:-1, :, Q21]])      # [T][B][21]: the plant tick t started from
        worst[name] = float(np.abs(r["meas_hist"][:, :, Q21] - start).max())
        assert np.abs(start).max() < 16.0 and np.abs(start[:, :, :7]).max() > 0.5      # (the joint words the bound was derived for: an ulp below 16 is 1.8e-15)
        if with_plant:
            assert (r["plant_rec"][:, er.PLANT_REC["MAX_DU"]] > 0).any()
    print(f"nw {nw}, plant {with_plant}: |meas_hist - plant at the tick's start| with LEAD {worst['lead']:.3e}, with HOLD alone {worst['no lead']:.3e}")
    assert worst["no lead"] > 1e-6
    assert worst["lead"] <= 1e-12


# ---- 5. P3: the filter filters ----
P3_TICKS, P3_SEED = 12, 4


def _p3_draws():
    return es.noise(P3_TICKS, B, P3_SEED)


def test_the_draws_of_the_filter_test_on_the_mirror():
    """The error of the estimate under noise on q alone with gains (0.3, 1, 1) obeys e+ = (1 - L) e- + L n (dq and ddq are handed on exactly, so the prediction
    leaks nothing), from e_0 = n_0: on the draws the test below fixes, the mirror's ratio of the two sums of squares is below 0.35 for every stream."""
    n = _p3_draws()[:, :, :7]
    e = np.zeros_like(n)
    e[0] = n[0]
    for t in range(1, P3_TICKS):
        e[t] = 0.7 * e[t - 1] + 0.3 * n[t]
    ratio = (e ** 2).sum(axis=(0, 2)) / (n ** 2).sum(axis=(0, 2))
    print("mirror ratios:", ratio)
    assert (ratio < 0.35).all()


@pytest.mark.parametrize("nw", [1, 4])
def test_a_gain_below_one_filters_the_noise_of_the_sensor(nw):
    """P3.  Noise on q only (NQ = 1e-3), no HOLD, gains (0.3, 1, 1), fixed draws, 12 ticks: observer_rec.SUMSQ_DQ < 0.5 sensor_rec.SUMSQ_DQ for every stream.  The
    stationary variance of e+ = (1 - L)(e- + leak) + L n for q-only noise is L / (2 - L) = 0.18 of the sensor's at L = 0.3; 0.5 leaves room for the first tick,
    where post = m.  With gain 1 the two records are equal word for word."""
    A0, Tab, _ = er.start(N, S, nw, B)
    sensor, nz = bstream.sensor_table(B, nq=1e-3), _p3_draws()
    for lq in (0.3, 1.0):
        r = eo.rollout(N, S, H, Tab.copy(), _copy(A0), P3_TICKS, nw=nw, sensor=sensor, sensor_state=np.zeros((B, 64)), sensor_noise=nz,
                       observer=bstream.observer_table(B, lq=lq, ldq=1.0, lddq=1.0), observer_state=np.zeros((B, 40)), log_stages=N)
        assert (r["ticks_run"] == P3_TICKS).all() and not r["observer_info"].any()
        so, ss_ = r["observer_rec"][:, OBSERVER_REC["SUMSQ_DQ"]], r["sensor_rec"][:, SENSOR_REC["SUMSQ_DQ"]]
        print(f"nw {nw}, LQ {lq}: SUMSQ_DQ observer / sensor", so / ss_)
        if lq == 1.0:
            assert np.array_equal(r["observer_rec"][:, 2:], r["sensor_rec"][:, 1:7]) and np.array_equal(r["observer_rec"][:, 0], r["sensor_rec"][:, 0])
        else:
            assert (ss_ > 0).all() and (so < 0.5 * ss_).all()


# ---- 6. the gate ----
@pytest.mark.parametrize("nw", [1, 4])
def test_the_gate_rejects_the_outlier_and_hands_out_the_prior(nw):
    """every stream on the GATE row: the outlier tick is counted in N_REJ and no other; its sample_hist row carries the outlier; its meas_hist row carries the
    prior, the mirror's bit for bit (the mirror chained over the run's own truths and draws)"""
    A0, Tab, _ = er.start(N, S, nw, B)
    ob, se, _ = _rows()
    otab, sensor, nz = np.tile(ob[3], (B, 1)), np.tile(se[3], (B, 1)), es.noise(T, B)
    t0, j0, big = OUTLIER
    nz[t0, :, j0] = big
    r = eo.rollout(N, S, H, Tab.copy(), _copy(A0), T, nw=nw, sensor=sensor, sensor_state=np.zeros((B, 64)), sensor_noise=nz, observer=otab, observer_state=np.zeros((B, 40)),
                   log_stages=N)
    assert (r["ticks_run"] == T).all() and (r["observer_rec"][:, OBSERVER_REC["N_REJ"]] == 1).all() and (r["observer_rec"][:, 0] == T).all()
    start = np.concatenate([A0["rb"][None], r["hist"][:-1, :, :RB["LEN"]]])
    assert np.allclose(r["sample_hist"][t0, :, j0] - start[t0, :, j0], 0.1, atol=1e-12) and (np.abs(r["meas_hist"][t0, :, j0] - start[t0, :, j0]) < 1e-3).all()
    assert (r["sensor_rec"][:, SENSOR_REC["TICK_DQ"]] == t0).all() and (r["sensor_rec"][:, SENSOR_REC["JOINT_DQ"]] == j0).all()
    for b in range(B):
        st, ost = np.zeros(64), np.zeros(40)
        for t in range(T):
            rb, st, ost, m, _, _, _, _, rej = bstream.observe_robot(start[t, b], sensor[b], st, otab[b], ost, H, nz[t, b])
            assert rej == (t == t0) and np.array_equal(rb[Q21], r["meas_hist"][t, b, Q21]) and np.array_equal(m, r["sample_hist"][t, b]), (b, t)


# ---- 7. invalid rows ----
@pytest.mark.parametrize("nw", [1, 4])
def test_invalid_rows_do_not_run_and_their_neighbours_do(nw):
    """row 0: an invalid observer row (gain 0, gate -1); row 2: an invalid sensor row under a valid observer row; rows 1 and 3 valid"""
    A0, Tab, _ = er.start(N, S, nw, B)
    ob, se, nz = _rows()
    otab, sensor, nz = ob[[1, 1, 2, 3]].copy(), se[[1, 1, 2, 3]].copy(), np.ascontiguousarray(nz[:, [1, 1, 2, 3]])
    bad_o, bad_s = otab.copy(), sensor.copy()
    bad_o[0, OBSERVER["LQ"]], bad_o[0, OBSERVER["GATE"]], bad_s[2, SENSOR["HOLD"]] = 0.0, -1.0, 0.5
    A, sst, ost = _copy(A0), np.full((B, 64), 1.5), np.full((B, 40), 2.5)
    for k in ("x", "g", "kkt", "p", "x0"):
        A[k][[0, 2]] = 7.25      # (what the memory held: it stays)
    A["iters"][[0, 2]], A["status"][[0, 2]] = 77, 9
    sst[[1, 3]], ost[[1, 3]] = 0.0, 0.0
    before = _copy(A)
    common = dict(nw=nw, sensor_noise=nz, log_stages=N, disturb=er.disturbances(T, B, on=(1, 4)))
    r = eo.rollout(N, S, H, Tab.copy(), A, T, sensor=bad_s, sensor_state=sst, observer=bad_o, observer_state=ost, **common)
    assert r["observer_info"].tolist() == [1 << OBSERVER["LQ"] | 1 << OBSERVER["GATE"], 0, 0, 0] and r["sensor_info"].tolist() == [0, 0, 1 << SENSOR["HOLD"], 0]
    assert r["ticks_run"].tolist() == [0, T, 0, T]
    for b in (0, 2):
        er.assert_arrays_equal(er.unstack(before, b), er.unstack(A, b), f"invalid row, stream {b}")
        assert (sst[b] == 1.5).all() and (ost[b] == 2.5).all()
        assert all(np.isnan(r[k][:, b]).all() for k in ("hist", "traj_hist", "tube_hist", "log_hist", "meas_hist", "sample_hist"))
        assert np.array_equal(r["observer_rec"][b], eo.fresh_rec()) and r["observer_rec"][b].tolist() == [0, 0, -np.inf, -1, -1, -np.inf, -1, 0]
        assert np.array_equal(r["sensor_rec"][b], es.fresh_rec())
    C, sc, oc = _copy(A0), np.zeros((B, 64)), np.zeros((B, 40))
    good = eo.rollout(N, S, H, Tab.copy(), C, T, sensor=sensor, sensor_state=sc, observer=otab, observer_state=oc, **common)
    for b in (1, 3):
        er.assert_arrays_equal(er.unstack(C, b), er.unstack(A, b), f"neighbour {b}")
        assert np.array_equal(sst[b], sc[b]) and np.array_equal(ost[b], oc[b])
        for k in eo.HISTORIES + ("observer_rec", "sensor_rec"):
            sl = (slice(None), b) if k in eo.HISTORIES else (b,)
            assert np.array_equal(r[k][sl], good[k][sl], equal_nan=True), (b, k)


# ---- 8. the contract ----
B5 = 5


@functools.lru_cache(maxsize=None)
def _five(nw):
    """five streams behind their tick 0 with a two-record queue each: (arrays, tables, queue [5][2][len]); copy before use"""
    A0, Tab, _ = er.start(N, S, nw, B5)
    kinds = [er.small_batch(N, S, B5)[3], er.small_batch(N, S, B5, detour=0.05)[3]]
    return A0, Tab, np.ascontiguousarray(np.stack(kinds, axis=1))


@pytest.mark.parametrize("nw,wave_order,lane_order", [(1, 0, 0), (4, 1, 1)])
def test_a_rollout_with_observers_equals_the_per_tick_loop(nw, wave_order, lane_order):
    """one stream per row of ROWS; events, audit, log with every stage, tracking record, a two-record queue, disturbances, the sweeps' table and a plant table on:
    every tick array, history array (meas_hist and sample_hist among them), record, queue output, plant_state, plant_rec, sensor_state, sensor_rec,
    observer_state and observer_rec of every stream against contract_loop.  Every row but IDENT and NAN hands the pack something else than the sample."""
    A0, Tab, Q = _five(nw)
    ob, se, nz = _rows()
    idx = [0, 1, 2, 3, 0]
    lt = np.array([[1, 4], [2, 4], [1, 4], [2, 4], [1, 4]], dtype=np.int32)
    r, A, Tb, R, pst, sst, ost, loops = eo.assert_equals_the_loop(N, S, A0, Tab, Q, T, se, ob, f"nw {nw} orders {wave_order} {lane_order}", sensor_noise=nz, plant=_plant()[idx],
                                                                  pstate0=bstream.plant_state_of(A0["rb"]), nw=nw, wave_order=wave_order, lane_order=lane_order, stages=N,
                                                                  tune=er.table()[idx], accept_capped=True, leg_tick=lt, leg_on=np.zeros((B5, 2), dtype=np.int32),
                                                                  disturb=er.disturbances(T, B5, on=(1, 4)))
    assert (r["observer_rec"][:, OBSERVER_REC["SAMPLES"]] == r["ticks_run"]).all() and (r["ticks_run"] >= 2).all()
    for b, name in enumerate(ROWS):
        n = int(r["ticks_run"][b])
        assert np.array_equal(r["sample_hist"][:n, b], r["meas_hist"][:n, b, Q21]) == (name in ("ident", "nan")), name
        assert np.isnan(r["sample_hist"][n:, b]).all() and not np.isnan(r["sample_hist"][:n, b]).any()
    assert ost[2, OBSERVER_STATE["LAGS"]] == 1.0 and not ost[[0, 1, 3, 4], OBSERVER_STATE["LAGS"]].any()


# ---- 9. chaining ----
@pytest.mark.parametrize("nw", [1, 4])
def test_one_rollout_of_six_ticks_is_two_of_three_that_hand_over_the_states(nw):
    A0, Tab, _ = er.start(N, S, nw, B)
    ob, se, nz = _rows()
    otab, sensor, nz, d = ob[:4], se[:4], np.ascontiguousarray(nz[:, :4]), er.disturbances(T, B, on=(1, 4))
    half = lambda a, k: np.ascontiguousarray(a[3 * k:3 * k + 3])
    A, st, ost = _copy(A0), np.zeros((B, 64)), np.zeros((B, 40))
    whole = eo.rollout(N, S, H, Tab.copy(), A, T, nw=nw, sensor=sensor, sensor_state=st, sensor_noise=nz, observer=otab, observer_state=ost, disturb=d, log_stages=N)
    C, sc, oc = _copy(A0), np.zeros((B, 64)), np.zeros((B, 40))
    parts = [eo.rollout(N, S, H, Tab.copy(), C, 3, nw=nw, sensor=sensor, sensor_state=sc, sensor_noise=half(nz, k), observer=otab, observer_state=oc, disturb=half(d, k), log_stages=N)
             for k in (0, 1)]
    assert whole["ticks_run"].tolist() == [T] * B and parts[0]["ticks_run"].tolist() == [3] * B
    for b in range(B):
        er.assert_arrays_equal(er.unstack(A, b), er.unstack(C, b), f"chained, stream {b}")
    assert np.array_equal(st, sc) and np.array_equal(ost, oc)
    for k in eo.HISTORIES:
        assert np.array_equal(whole[k], np.concatenate([parts[0][k], parts[1][k]]), equal_nan=True), k
    assert (parts[0]["observer_rec"][:, 0] + parts[1]["observer_rec"][:, 0] == T).all()
    # a second half that starts from a fresh observer state is another run for the rows with a gain below 1: its first tick takes the sample as it is
    E, se_, oe = _copy(A0), np.zeros((B, 64)), np.zeros((B, 40))
    eo.rollout(N, S, H, Tab.copy(), E, 3, nw=nw, sensor=sensor, sensor_state=se_, sensor_noise=half(nz, 0), observer=otab, observer_state=oe, disturb=half(d, 0), log_stages=N)
    fresh = eo.rollout(N, S, H, Tab.copy(), E, 3, nw=nw, sensor=sensor, sensor_state=se_, sensor_noise=half(nz, 1), observer=otab, observer_state=np.zeros((B, 40)), disturb=half(d, 1),
                       log_stages=N)
    same = [np.array_equal(fresh["hist"][:, b], parts[1]["hist"][:, b]) for b in range(B)]
    assert same == [True, False, False, False], same


# ---- 10. housekeeping ----
def test_argument_errors_of_the_entry():
    """an observer without a sensor table, an observer without its state, and what the sensors' entry refuses, with an observer table; the observer's outputs may be NULL"""
    A0, Tab, _ = er.start(N, S, 1, B)
    ob, se, _ = _rows()
    otab, sensor = ob[:4], se[:4]
    ok = dict(sensor=sensor, sensor_state=np.zeros((B, 64)), observer=otab, observer_state=np.zeros((B, 40)))
    for kw in (dict(ok, sensor=None, sensor_state=None), dict(ok, sensor=None), dict(ok, observer_state=None), dict(ok, sensor_state=None), dict(ok, ticks=0), dict(ok, simulate=False),
               dict(ok, goal_tol=-1.0), dict(ok, audit_tol=np.inf), dict(ok, log_stages=N + 1), dict(ok, update_flags=8)):
        A, kw = _copy(A0), dict(kw)
        assert eo.rollout(N, S, H, Tab.copy(), A, kw.pop("ticks", 2), want_rc=True, **kw) == 1, [k for k, v in kw.items() if v is None]
        for b in range(B):
            er.assert_arrays_equal(er.unstack(A0, b), er.unstack(A, b), "nothing runs")
        assert not ok["sensor_state"].any() and not ok["observer_state"].any()
    assert eo.rollout(N, S, H, Tab.copy(), _copy(A0), 1, want_rc=True, want_sample=False, want_observer_rec=False, want_observer_info=False, **ok) == 0
    assert eo.rollout(N, S, H, Tab.copy(), _copy(A0), 1, want_rc=True, sensor=sensor, sensor_state=np.zeros((B, 64))) == 0      # (no observer table: no state needed)
    L, NA, OA = eo.lib(), es.NArgs, eo.OArgs
    okf = lambda n, o: L.bmpc_emu_rollout_observer_ok(ctypes.byref(n), ctypes.byref(o))
    assert okf(NA(), OA()) == 1 and okf(NA(), OA(observer_state=1, sample_hist=1)) == 1 and okf(NA(sensor=1, sensor_state=1), OA(observer=1, observer_state=1)) == 1
    assert okf(NA(), OA(observer=1, observer_state=1)) == 0 and okf(NA(sensor=1, sensor_state=1), OA(observer=1)) == 0


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
    row, st, rec = eo.observer_slots()
    for first, prefix, d, kernel in (("BMPC_OBSERVER_LQ", "BMPC_OBSERVER_", OBSERVER, row), ("BMPC_OBSERVER_STATE_POST", "BMPC_OBSERVER_STATE_", OBSERVER_STATE, st),
                                     ("BMPC_OBSERVER_REC_SAMPLES", "BMPC_OBSERVER_REC_", OBSERVER_REC, rec)):
        e = {k[len(prefix):]: v for k, v in enum_of(first).items()}
        assert e == d and [v for k, v in sorted(d.items(), key=lambda kv: kv[1]) if k != "LEN"] == kernel, (prefix, e, d, kernel)
    assert (OBSERVER["LEN"], OBSERVER_STATE["LEN"], OBSERVER_REC["LEN"]) == (8, 40, 8) and eo.lib().bmpc_emu_observer_slot(0, -2) == 5
    # the records: RArgs keeps its 30 members and NArgs its six, OArgs is the five of the entry in their order, in both builds
    for nw in (1, 4):
        L = eo.lib(nw)
        assert len(er.RArgs._fields_) == 30 and len(es.NArgs._fields_) == 6 and L.bmpc_emu_observer_rargs_size() == er.lib(nw).bmpc_emu_rargs_size()
        assert L.bmpc_emu_observer_nargs_size() == es.lib(nw).bmpc_emu_nargs_size()
        assert [L.bmpc_emu_oargs_offset(name.encode()) for name, _ in eo.OArgs._fields_] == [getattr(eo.OArgs, name).offset for name, _ in eo.OArgs._fields_]
        assert [name for name, _ in eo.OArgs._fields_] == ["observer", "observer_state", "observer_info", "observer_rec", "sample_hist"] and L.bmpc_emu_oargs_offset(b"sensor") == -1
    from boundmpc_amd import _lib, build
    import boundmpc_amd
    syms = ("bmpc_stream_observer_len", "bmpc_stream_observer_state_len", "bmpc_stream_observer_rec_len", "bmpc_stream_rollout_observer", "bmpc_stream_observe")
    for sym in syms:
        assert sym in _lib.SIGNATURES and re.search(r"\b%s\(" % sym, header)
    assert len(_lib.SIGNATURES["bmpc_stream_rollout_observer"][1]) == len(_lib.SIGNATURES["bmpc_stream_rollout_sensor"][1]) + 5
    assert len(_lib.SIGNATURES["bmpc_stream_observe"][1]) == len(_lib.SIGNATURES["bmpc_stream_sense"][1]) + 5
    if os.path.exists(_lib.LIB_PATH):      # (a built tree: the symbols are exported; loading the library needs no GPU)
        L = ctypes.CDLL(_lib.LIB_PATH)
        assert all(hasattr(L, sym) for sym in syms) and (L.bmpc_stream_observer_len(), L.bmpc_stream_observer_state_len(), L.bmpc_stream_observer_rec_len()) == (8, 40, 8)
    units = [os.path.basename(u) for u in build.UNITS]
    assert "bmpc_rollout_observer.hip" in units and "bmpc_team_rollout_observer.hip" in units
    params = set(inspect.signature(bstream.StreamBatch.rollout).parameters)
    assert {"observer", "want_sample", "want_observer_rec"} <= params and all(hasattr(bstream.StreamBatch, m) for m in ("observe", "observer_reset", "observer_state"))
    assert bstream.ROLLOUT_ENTRIES[-1] == "bmpc_stream_rollout_plant"      # (they stay as they are)
    for name in ("OBSERVER", "OBSERVER_STATE", "OBSERVER_REC", "observer_table", "observer_check", "observe_robot", "unpack_observer_rec"):
        assert getattr(boundmpc_amd, name) is getattr(bstream, name)
    for text in (bstream.StreamBatch.rollout.__doc__, header, bstream.observe_robot.__doc__):      # the blind spot is documented where the rule is stated
        assert "spliced re-plan" in text and "not reset" in " ".join(text.split()).replace("never reset", "not reset")
    # the existing kernels expand the body without an observer line
    kernel = open(os.path.join(here, "..", "boundmpc_amd", "csrc", "bmpc_rollout_kernel.inl")).read()
    assert kernel.count("#define BMPCR_OB 0") == 2 and kernel.count("#define BMPCR_OB 1") == 1


def sanitizer_cases(nw):
    A0, Tab, _ = er.start(N, S, nw, B)
    ob, se, nz = _rows(3)
    sensor, nz3 = se[:4].copy(), np.ascontiguousarray(nz[:, :4])
    ident = np.tile(IDENT, (B, 1))
    lead = np.tile(ob[2], (B, 1)); hold = np.tile(se[2], (B, 1))
    gate = np.tile(ob[3], (B, 1)); gate[0, OBSERVER["LQ"]] = 2.0      # (stream 0: an invalid neighbour)
    big = nz3.copy(); big[1, :, 2] = 1000.0
    base = dict(N=N, S=S, h=H, T=Tab, A=A0, ticks=3)
    return [("identity", dict(base, sensor=sensor, observer=ident, sensor_noise=nz3, plant=_plant(), plant_state=bstream.plant_state_of(A0["rb"]), disturb=er.disturbances(3, B, on=(1,)))),
            ("lead + hold", dict(base, sensor=hold, observer=lead, sensor_noise=nz3)),
            ("gate", dict(base, sensor=np.tile(se[3], (B, 1)), observer=gate, sensor_noise=big))]


@pytest.mark.parametrize("nw", [1, 4])
def test_the_observer_text_is_clean_under_the_sanitizers(nw):
    """the host program with its own main, built with -fsanitize=address,undefined on exact-size buffers and run as a child process (nothing is loaded into
    this interpreter, nothing preloaded); on teams under both wave orders: identity, LEAD + HOLD, and the gate with an invalid neighbour"""
    out = eo.run_sanitized(sanitizer_cases(nw), nw)
    print("\n".join(out))
    assert len(out) == 3 and all("rc 0 ran 8" in line and "DIFFERS" not in line for line in out)
    assert "[stream 0 ticks_run 3 sensor_info 0 observer_info 0 estimates 3 rejected 0]" in out[0] and "[stream 3 ticks_run 3 sensor_info 0 observer_info 0 estimates 3 rejected 0]" in out[1]
    assert "[stream 0 ticks_run 0 sensor_info 0 observer_info %d estimates 0 rejected 0]" % (1 << OBSERVER["LQ"]) in out[2]
    assert "[stream 1 ticks_run 3 sensor_info 0 observer_info 0 estimates 3 rejected 1]" in out[2]
